"""The host-side route of the spectra (csrc/spec_route.h, compiled here by itself with g++: no GPU, no HIP): which transform
a length goes to, how the rows are cut into workgroups, the LDS, and the sizes of the partial, row, spectrum and image
buffers.  The kinds are held to own_fft_len_ok / own_fft_mixed_len_ok restated here from their rule (a power of two,
or 2 3 5 7-smooth, between 16 and 8192, for the complex length n / 2 of an even n); everything else follows from what
csrc/spectrum.hip's kernels index.  The same sweep runs once more as a stand-alone program under AddressSanitizer and
UBSan (tests/san/spec_route_sweep.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, 'impdar_amd', 'csrc')
POW2, MIXED, ROCFFT = 0, 1, 2
LENGTHS = list(range(1, 2101)) + [4096, 8192, 10000, 16384, 16386, 20000, 40000]
ROWS = [1, 2, 255, 256, 257, 4096, 10000, 16384]
needs_gxx = pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not installed')


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('specroute'))
    src, so = os.path.join(tmp, 'spec_route_probe.cpp'), os.path.join(tmp, 'libspecroute.so')
    with open(src, 'w') as f:
        f.write('#define SPEC_ROUTE_PROBE 1\n#include "spec_route.h"\n')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-shared', '-fPIC', '-I', CSRC, src, '-o', so])
    lib = C.CDLL(so)
    lib.impdar_spec_route_full_probe.argtypes = [C.c_int, C.c_longlong, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    return lib


def route(lib, n, rows):
    ints, longs = (C.c_int * 8)(), (C.c_longlong * 8)()
    rc = lib.impdar_spec_route_full_probe(n, rows, ints, longs)
    r = dict(zip(('kind', 'M', 'logm', 'bins', 'identity', 'threads', 'ok'), list(ints)))
    r.update(zip(('workgroups', 'rows_per_wg', 'lds', 'partial', 'rowbuf', 'spectrum', 'image'), list(longs)))
    r['rc'] = rc
    return r


def smooth(m):
    for p in (2, 3, 5, 7):
        while m % p == 0:
            m //= p
    return m == 1


def expected_kind(n):
    m = n // 2
    if n % 2 == 0 and 16 <= m <= 8192:
        if m & (m - 1) == 0:
            return POW2
        if smooth(m):
            return MIXED
    return ROCFFT


def pad(i):
    return i + (i >> 5)


@needs_gxx
def test_kind_of_every_length(lib):
    for n in LENGTHS:
        assert route(lib, n, 7)['kind'] == expected_kind(n), n
    # the lengths of the FS* fixtures and of the benchmark line
    assert [expected_kind(n) for n in (32, 36, 30, 63, 22, 7, 100, 1022, 1024, 4096, 16384, 16386, 2, 1, 10000)] == \
        [POW2, MIXED, ROCFFT, ROCFFT, ROCFFT, ROCFFT, MIXED, ROCFFT, POW2, POW2, POW2, ROCFFT, ROCFFT, ROCFFT, MIXED]


@needs_gxx
def test_rows_are_covered_exactly_once(lib):
    for n in LENGTHS:
        for rows in ROWS:
            r = route(lib, n, rows)
            assert r['rc'] == 0 and r['ok'] == 1, (n, rows)
            wg, per = r['workgroups'], r['rows_per_wg']
            assert wg >= 1 and per >= 1
            # block w = [w per, min(rows, (w + 1) per)): the last block is not empty and ends at the last row
            assert (wg - 1) * per < rows <= wg * per, (n, rows, wg, per)
    # a large radargram's traces: as many workgroups as stay resident, each with several rows
    r = route(lib, 4096, 10000)
    assert r['workgroups'] <= 256 * 8 and r['workgroups'] * r['rows_per_wg'] >= 10000 and r['rows_per_wg'] >= 5


@needs_gxx
def test_launch_fits_a_compute_unit(lib):
    for n in LENGTHS:
        r = route(lib, n, 300)
        assert r['lds'] <= 160 * 1024, n
        assert r['bins'] == n // 2 + 1 and r['M'] == n // 2
        assert r['identity'] == (1 if n == 1 else 0)
        if r['kind'] == ROCFFT:
            assert r['lds'] == 0 and r['threads'] == 256 and r['workgroups'] <= 1024
        else:
            M, th = r['M'], r['threads']
            assert th == (1024 if M >= 4096 else 512 if M >= 2048 else 256 if M >= 1024 else 64)      # own_fft_launch's
            assert (1 << r['logm']) >= M > (1 << r['logm']) // 2
            # the padded row, a spare slot, and the tree of the mean
            assert r['lds'] == (pad(M) + 1) * 16 + th * 8
            # a thread's bins k = tid + j threads, k <= M, fit its accumulators
            assert -(-(M + 1) // th) <= (16 if th == 64 else 9)
            assert r['workgroups'] <= 256 * min(8, 160 * 1024 // r['lds'], 2048 // th)
    assert route(lib, 16384, 300)['lds'] == (8192 + 256 + 1) * 16 + 8192           # the largest: one workgroup per CU
    assert 2 * route(lib, 16384, 300)['lds'] > 160 * 1024


@needs_gxx
def test_buffer_sizes(lib):
    for n in LENGTHS:
        for rows in ROWS:
            r = route(lib, n, rows)
            assert r['partial'] == r['workgroups'] * r['bins']
            assert r['rowbuf'] == rows * n
            assert r['image'] == rows * r['bins']
            assert r['spectrum'] == (2 * rows * r['bins'] if r['kind'] == ROCFFT else 0)


@needs_gxx
def test_refuses_empty(lib):
    assert route(lib, 0, 5)['rc'] != 0 and route(lib, 5, 0)['rc'] != 0 and route(lib, -4, 5)['rc'] != 0


@needs_gxx
@pytest.mark.skipif(os.path.exists('/dev/kfd'), reason='sanitizer job is for the CPU container (never on the GPU box)')
def test_sweep_under_sanitizers(tmp_path):
    """Host code only, in a program of its own: the sanitizers' runtime is linked into it."""
    exe = str(tmp_path / 'spec_route_sweep')
    subprocess.check_call(['g++', '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-I', CSRC, os.path.join(ROOT, 'tests', 'san', 'spec_route_sweep.cpp'), '-o', exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:]
    assert '%d routes hold' % (len(LENGTHS) * len(ROWS)) in out.stdout


def test_spectrum_unit_decides_nothing_itself():
    """spectrum.hip takes kind, threads, workgroups, rows per workgroup, LDS and every buffer size from the route."""
    text = open(os.path.join(CSRC, 'spectrum.hip')).read()
    assert '#include "spec_route.h"' in text
    for word in ('own_fft_len_ok', 'own_fft_mixed_len_ok'):
        assert word not in text, word
    header = open(os.path.join(CSRC, 'spec_route.h')).read()
    assert 'hip_runtime' not in header and '#include <hip' not in header
    assert np.all([w in text for w in ('R.workgroups', 'R.rows_per_wg', 'R.lds', 'R.threads', 'R.partial_doubles')])
