"""The host-side route of the complex-trace attributes (csrc/attr_route.h over csrc/spec_route.h, compiled here by itself with
g++: no GPU, no HIP): every refusal with its wording, and the kind of route, the threads, the LDS and the scratch sizes at the
GPU suite's shapes."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import attr_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, 'impdar_amd', 'csrc')
pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not installed')

IKEYS = ('kind', 'M', 'threads', 'trivial', 'ok', 'pairs')
LKEYS = ('workgroups', 'rows_per_wg', 'lds', 'rowbuf', 'spectrum', 'quad', 'flags', 'out_pitch', 'tiles_x', 'tiles_y')
LDS_MAX = 160 * 1024

MAIN = r'''
#define ATTR_ROUTE_PROBE
#include "attr_route.h"
#include <cstdio>
#include <cmath>
#include <cstring>
// every refusal and a walk over many shapes: what a sanitizer has to see
int main()
{
    int bad = 0;
    bad += attr_refusal(100, 8, 1, 1, 1.0) != nullptr;
    bad += attr_refusal(100, 8, 4, 1, 1.0) == nullptr;
    bad += attr_refusal(100, 8, 3, 2, 1.0) == nullptr;
    bad += attr_refusal(100, 8, 1, 3, 1.0) == nullptr;
    bad += attr_refusal(100, 8, 3, 3, NAN) == nullptr;
    bad += attr_refusal(0, 8, 1, 1, 1.0) == nullptr;
    long long sum = 0;
    for (int n = 1; n <= 17000; n += (n < 200 ? 1 : 97))
        for (int t = 1; t <= 5000; t = t * 3 + 1)
            for (int smooth = 1; smooth <= 3; smooth += 2) {
                const AttrRoute A = attr_route(n, t, ATTR_FREQUENCY, smooth);
                if (!A.ok) { ++bad; continue; }
                if (A.spec.kind != SPEC_ROCFFT && ((A.spec.M + A.spec.threads - 1) / A.spec.threads > attr_row_acc(A.spec.threads) ||
                                                   A.spec.lds > (size_t)SPEC_LDS_MAX || A.spec.lds < (size_t)(spec_pad(A.spec.M) + 1) * 16)) ++bad;
                sum += (long long)A.out_pitch + (long long)strlen(A.label);
            }
    printf("bad %d sum %lld\n", bad, sum);
    return bad != 0;
}
'''


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('attrroute'))
    src, so = os.path.join(tmp, 'attr_route_probe.cpp'), os.path.join(tmp, 'libattrroute.so')
    with open(src, 'w') as f:
        f.write('#define ATTR_ROUTE_PROBE\n#include "attr_route.h"\n')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-shared', '-fPIC', '-I', CSRC, src, '-o', so])
    lib = C.CDLL(so)
    lib.attr_probe_refusal.restype = C.c_char_p
    lib.attr_probe_refusal.argtypes = [C.c_int] * 4 + [C.c_double]
    lib.attr_probe_route.restype = C.c_char_p
    lib.attr_probe_route.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    return lib


def refusal(lib, snum=100, tnum=8, kind=1, smooth=1, dt=1.0e-9):
    why = lib.attr_probe_refusal(snum, tnum, kind, smooth, dt)
    return None if why is None else why.decode()


def route(lib, snum, tnum, kind=1, smooth=1):
    ints, longs = np.zeros(8, dtype=np.int32), np.zeros(10, dtype=np.int64)
    label = lib.attr_probe_route(snum, tnum, kind, smooth, ints.ctypes.data_as(C.POINTER(C.c_int)), longs.ctypes.data_as(C.POINTER(C.c_longlong)))
    return dict(zip(IKEYS, ints.tolist()), label=label.decode(), **dict(zip(LKEYS, longs.tolist())))


def own_pad(i):
    return i + (i >> 5)


def test_every_refusal_has_its_reason(lib):
    for kind in range(4):
        assert refusal(lib, kind=kind) is None
    assert refusal(lib, kind=-1) == refusal(lib, kind=4) == 'kind must be 0 (quadrature), 1 (envelope), 2 (phase) or 3 (frequency)'
    for smooth in (0, -1, 2, 254, 256, 257):
        assert refusal(lib, kind=3, smooth=smooth) == 'smooth must be odd and lie in 1 .. 255', smooth
    for smooth in (1, 3, 9, 255):
        assert refusal(lib, kind=3, smooth=smooth) is None
    for kind in (0, 1, 2):
        assert refusal(lib, kind=kind, smooth=3) == 'smooth above 1 goes with kind 3 (frequency) alone'
    for dt in (0.0, -1.0e-9, float('nan'), float('inf'), -float('inf')):
        assert refusal(lib, kind=3, dt=dt) == 'dt must be finite and positive', dt
        assert refusal(lib, kind=1, dt=dt) is None           # (read for the frequency alone)
    assert refusal(lib, snum=0) == refusal(lib, tnum=0) == refusal(lib, snum=-3) == 'empty radargram'
    # the order of the contract's list: the kind first, the radargram last
    assert refusal(lib, snum=0, kind=7).startswith('kind must be')
    assert refusal(lib, snum=0, kind=3, smooth=2).startswith('smooth must be')


@pytest.mark.parametrize('case', R.CASES + [(32, 2101, R.OWN_POW2, 64), (4096, 10000, R.OWN_POW2, 512), (10000, 4096, R.OWN_MIXED, 1024)], ids=R.case_id)
def test_route_at_the_gpu_suites_shapes(lib, case):
    n, tnum, kind, threads = case
    A = route(lib, n, tnum)
    assert A['ok'] == 1 and A['kind'] == kind and A['M'] == n // 2 and A['trivial'] == int(n <= 2)
    assert A['tiles_x'] == -(-tnum // 32) and A['tiles_y'] == -(-n // 32)
    assert A['rowbuf'] == n * tnum
    # the traces are cut into blocks in order, none empty, the last one possibly short
    assert (A['workgroups'] - 1) * A['rows_per_wg'] < tnum <= A['workgroups'] * A['rows_per_wg']
    if kind == R.ROCFFT:
        bins = n // 2 + 1
        assert A['spectrum'] == 2 * tnum * bins and A['quad'] == n * tnum and A['flags'] == tnum and A['pairs'] == 0
        assert A['out_pitch'] == 2 * bins                                   # the attribute rows lie where the spectrum was
        assert route(lib, n, tnum, 3, 9)['out_pitch'] == n                  # ... the smoothed frequency over the x rows
        assert ('rocFFT' in A['label']) == (n > 2) and 'attr_global_kernel' in A['label']
    else:
        M = n // 2
        assert A['threads'] == threads == (1024 if M >= 4096 else 512 if M >= 2048 else 256 if M >= 1024 else 64)
        assert -(-M // threads) <= A['pairs'] == (16 if threads == 64 else 8)
        assert A['lds'] == (own_pad(M) + 1) * 16 + threads * 8 <= LDS_MAX
        assert A['lds'] >= n * 8                                            # the window sums read the row as n plain doubles
        assert A['spectrum'] == A['quad'] == A['flags'] == 0 and A['out_pitch'] == n
        assert route(lib, n, tnum, 3, 9)['out_pitch'] == n
        assert 'attr_rows_kernel' in A['label'] and ('mixed' in A['label']) == (kind == R.OWN_MIXED)
    if (n, tnum) == (32, 2100):
        assert A['rows_per_wg'] == 2 and A['workgroups'] == 1050
    if (n, tnum) == (32, 2101):
        assert A['rows_per_wg'] == 2 and A['workgroups'] == 1051             # a last block of one trace
    if n == 16384:
        assert A['lds'] > 128 * 1024                                        # one workgroup per compute unit


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The route header in a program of its own, with -fsanitize=address,undefined where the compiler has the run times."""
    src, exe = str(tmp_path / 'attr_route_main.cpp'), str(tmp_path / 'attr_route_main')
    with open(src, 'w') as f:
        f.write(MAIN)
    base = ['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-I', CSRC, src, '-o', exe]
    if subprocess.call(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith('bad 0 '), out.stdout[-2000:]


@pytest.mark.skipif(not os.path.exists(os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')), reason='hipcc not installed')
def test_every_new_header_compiles_alone(tmp_path):
    """attr_route.h and attr_kernels.h as the only include of a translation unit (host and device pass)."""
    procs = []
    for h in ('attr_route.h', 'attr_kernels.h'):
        src = str(tmp_path / (h[:-2] + '_alone.hip'))
        with open(src, 'w') as f:
            f.write('#include "%s"\n' % h)
        procs.append((h, subprocess.Popen([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '--offload-arch=gfx950', '-std=c++17', '-fsyntax-only',
                                           '-I', CSRC, src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for h, pr in procs:
        log = pr.communicate(timeout=600)[0]
        assert pr.returncode == 0, (h, log[-2000:])


def test_the_unit_takes_everything_from_the_route():
    text = open(os.path.join(CSRC, 'attr.hip')).read()
    assert 'attr_refusal(' in text and 'attr_route(' in text and 'host_form' in text
    assert text.count('static int attr_check(') == 1 and text.count('attr_check(ctx') == 2        # one check, called by both forms
    route_h = open(os.path.join(CSRC, 'attr_route.h')).read()
    assert '#include <hip' not in route_h and 'spec_route(' in route_h
    kernels = open(os.path.join(CSRC, 'attr_kernels.h')).read()
    assert 'atomicAdd' not in kernels and 'atomicAdd' not in text


def test_the_library_probe_agrees(lib):
    """impdar_attr_route_probe of the built library (no device call) against the header compiled here."""
    from impdar_amd import _hip
    out = np.zeros(8, dtype=np.int32)
    for n, tnum, kind, threads in R.CASES:
        rc = _hip.load().impdar_attr_route_probe(n, tnum, 1, 1, out.ctypes.data_as(C.POINTER(C.c_int)))
        assert rc == 0, _hip.last_error()
        A = route(lib, n, tnum)
        assert out[:6].tolist() == [A['kind'], A['threads'], A['workgroups'], A['rows_per_wg'], A['lds'], A['trivial']], (n, tnum)
    assert _hip.load().impdar_attr_route_probe(0, 3, 1, 1, out.ctypes.data_as(C.POINTER(C.c_int))) == _hip.ERR_ARG
    assert 'empty radargram' in _hip.last_error()
