"""The host-side route of a deconvolution / autocorrelation call (csrc/decon_route.h over csrc/decon_core.h, compiled here by
itself with g++: no GPU, no HIP): every refusal with its reason, the lag table without a duplicate or a lag of the gap, and the
plan -- chunks and blocks that cover their range once, scratch bytes -- at the GPU suite's shapes."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import decon_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, 'impdar_amd', 'csrc')
pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not installed')

PROBE = r'''
#include "decon_route.h"
extern "C" const char *decon_probe_refusal(int snum, int tnum, int s0, int s1, int oplen, int gap, double prewhiten, int design)
{
    return decon_refusal(snum, tnum, s0, s1, oplen, gap, prewhiten, design);
}
extern "C" const char *decon_probe_acorr_refusal(int snum, int tnum, int s0, int s1, int maxlag) { return acorr_refusal(snum, tnum, s0, s1, maxlag); }
// out: the lag of every row; returns the number of rows
extern "C" int decon_probe_lags(int oplen, int gap, int *out)
{
    const DeconLags L = decon_lags(oplen, gap);
    for (int j = 0; j < decon_lag_count(L); ++j) {
        out[j] = decon_row_lag(L, j);
        if (decon_lag_row(L, out[j]) != j) return -1;
    }
    return decon_lag_count(L);
}
// chunks[3 q ...]: row0, lag0, count of every chunk; returns their number
extern "C" int decon_probe_chunks(int acorr, int a, int b, int *chunks)
{
    const DeconPlan P = acorr ? acorr_plan(a + 1, 1, 0, a + 1, a) : decon_plan(a + b, 1, 0, a + b, a, b, 0);
    for (int q = 0; q < P.lag_chunks; ++q) {
        const DeconChunk c = decon_chunk(P.lags, q);
        chunks[3 * q] = c.row0;
        chunks[3 * q + 1] = c.lag0;
        chunks[3 * q + 2] = c.count;
    }
    return P.lag_chunks;
}
extern "C" const char *decon_probe_plan(int snum, int tnum, int s0, int s1, int oplen, int gap, int design, long long *out)
{
    const DeconPlan P = decon_plan(snum, tnum, s0, s1, oplen, gap, design);
    const long long v[] = {P.nlags, P.groups, P.lag_chunks, P.tap_chunks, P.sample_blocks, P.apply_blocks, P.solve_systems, P.solve_groups,
                           P.mean_blocks, (long long)P.acorr_lds, (long long)P.apply_lds, (long long)P.solve_lds, (long long)P.off_op,
                           (long long)P.off_mean, (long long)P.off_dead, (long long)P.scratch_bytes, DECON_C, DECON_TG, DECON_THREADS,
                           DECON_SOLVE_TRACES, DECON_MEAN_BLOCK};
    for (unsigned i = 0; i < sizeof v / sizeof v[0]; ++i) out[i] = v[i];
    return P.label;
}
'''
KEYS = ('nlags', 'groups', 'lag_chunks', 'tap_chunks', 'sample_blocks', 'apply_blocks', 'solve_systems', 'solve_groups', 'mean_blocks',
        'acorr_lds', 'apply_lds', 'solve_lds', 'off_op', 'off_mean', 'off_dead', 'scratch_bytes', 'C', 'TG', 'THREADS', 'SOLVE_TRACES',
        'MEAN_BLOCK')


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('deconroute'))
    src, so = os.path.join(tmp, 'decon_route_probe.cpp'), os.path.join(tmp, 'libdeconroute.so')
    with open(src, 'w') as f:
        f.write(PROBE)
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-shared', '-fPIC', '-I', CSRC, src, '-o', so])
    lib = C.CDLL(so)
    lib.decon_probe_refusal.restype = C.c_char_p
    lib.decon_probe_refusal.argtypes = [C.c_int] * 6 + [C.c_double, C.c_int]
    lib.decon_probe_acorr_refusal.restype = C.c_char_p
    lib.decon_probe_plan.restype = C.c_char_p
    return lib


def refusal(lib, snum=100, tnum=8, s0=0, s1=None, oplen=8, gap=2, prewhiten=0.1, design=0):
    why = lib.decon_probe_refusal(snum, tnum, s0, snum if s1 is None else s1, oplen, gap, prewhiten, design)
    return None if why is None else why.decode()


def plan(lib, snum, tnum, oplen, gap, window=None, design=0):
    s0, s1 = R.window_of(snum, window)
    out = np.zeros(len(KEYS), dtype=np.int64)
    label = lib.decon_probe_plan(snum, tnum, s0, s1, oplen, gap, design, out.ctypes.data_as(C.POINTER(C.c_longlong)))
    return dict(zip(KEYS, out.tolist()), label=label.decode())


def test_every_refusal_has_its_reason(lib):
    assert refusal(lib) is None
    assert refusal(lib, oplen=0) == refusal(lib, oplen=257) == 'oplen must lie in 1 .. 256'
    assert refusal(lib, snum=600, oplen=256) is None
    assert refusal(lib, gap=0) == 'gap must be at least 1'
    for s0, s1 in ((-1, 50), (50, 50), (60, 50), (0, 101)):
        assert refusal(lib, s0=s0, s1=s1) == 'the window must satisfy 0 <= s0 < s1 <= snum', (s0, s1)
    assert refusal(lib, s0=10, s1=20, oplen=8, gap=2) is None           # gap + oplen == s1 - s0
    assert refusal(lib, s0=10, s1=20, oplen=8, gap=3) == "gap + oplen must not exceed the window's length"
    assert refusal(lib, s0=10, s1=20, oplen=9, gap=2) == "gap + oplen must not exceed the window's length"
    for p in (-1e-9, float('nan'), float('inf'), -float('inf')):
        assert refusal(lib, prewhiten=p) == 'prewhiten must be finite and not negative', p
    assert refusal(lib, prewhiten=0.0) is None
    assert refusal(lib, design=2) == refusal(lib, design=-1) == 'design must be 0 (each) or 1 (mean)'
    assert refusal(lib, design=1) is None
    assert refusal(lib, snum=0) == refusal(lib, tnum=0) == 'empty radargram'
    ac = lib.decon_probe_acorr_refusal
    assert ac(100, 8, 0, 100, 99) is None and ac(100, 8, 0, 100, 0) is None
    assert ac(100, 8, 0, 100, 100) == ac(100, 8, 10, 30, 20) == b"maxlag must be below the window's length"
    assert ac(100, 8, 10, 30, 19) is None
    assert ac(100, 8, 0, 100, -1) == b'maxlag must not be negative'
    assert ac(100, 8, 30, 30, 1) == b'the window must satisfy 0 <= s0 < s1 <= snum'


@pytest.mark.parametrize('oplen,gap', [(8, 3), (8, 8), (8, 10), (8, 200), (1, 1), (1, 5), (256, 1), (256, 255), (256, 256), (256, 300),
                                       (64, 65), (31, 36)])
def test_lag_table_has_no_duplicate_and_no_lag_of_the_gap(lib, oplen, gap):
    out = np.zeros(2 * oplen, dtype=np.int32)
    n = lib.decon_probe_lags(oplen, gap, out.ctypes.data_as(C.POINTER(C.c_int)))
    assert n >= 0, 'decon_lag_row is not the inverse of decon_row_lag'
    got = out[:n].tolist()
    assert got == R.lag_list(oplen, gap)
    assert len(set(got)) == n
    if gap > oplen + 1:
        assert not set(range(oplen, gap)) & set(got)
    # the chunks cover the rows once, in order, none empty, none across the two runs
    chunks = np.zeros(3 * 16, dtype=np.int32)
    q = lib.decon_probe_chunks(0, oplen, gap, chunks.ctypes.data_as(C.POINTER(C.c_int)))
    rows = []
    for row0, lag0, count in chunks[:3 * q].reshape(q, 3).tolist():
        assert 1 <= count <= R.C
        assert [got[row0 + i] for i in range(count)] == list(range(lag0, lag0 + count))
        rows += list(range(row0, row0 + count))
    assert rows == list(range(n))


@pytest.mark.parametrize('maxlag', [0, 1, 63, 64, 65, 128, 1000])
def test_autocorrelogram_chunks(lib, maxlag):
    chunks = np.zeros(3 * 32, dtype=np.int32)
    q = lib.decon_probe_chunks(1, maxlag, 0, chunks.ctypes.data_as(C.POINTER(C.c_int)))
    rows = []
    for row0, lag0, count in chunks[:3 * q].reshape(q, 3).tolist():
        assert 1 <= count <= R.C and row0 == lag0
        rows += list(range(row0, row0 + count))
    assert rows == list(range(maxlag + 1))


@pytest.mark.parametrize('design', [0, 1], ids=['each', 'mean'])
@pytest.mark.parametrize('case', R.CASES + [R.BIG, (4096, 10000, 32, 8, None), (4096, 10000, 256, 8, None)], ids=R.case_id)
def test_plan_at_the_gpu_suites_shapes(lib, case, design):
    snum, tnum, oplen, gap, window = case
    s0, s1 = R.window_of(snum, window)
    P = plan(lib, snum, tnum, oplen, gap, window, design)
    assert P['C'] == R.C and P['THREADS'] == 256 and P['TG'] * 8 == P['THREADS']
    nl = len(R.lag_list(oplen, gap))
    assert P['nlags'] == nl
    # the tiles cover their ranges once and none is empty
    assert (P['groups'] - 1) * P['TG'] < tnum <= P['groups'] * P['TG']
    assert (P['sample_blocks'] - 1) * R.C < s1 - s0 <= P['sample_blocks'] * R.C
    assert (P['apply_blocks'] - 1) * R.C < snum <= P['apply_blocks'] * R.C
    assert (P['tap_chunks'] - 1) * R.C < oplen <= P['tap_chunks'] * R.C
    systems = 1 if design else tnum
    assert P['solve_systems'] == systems and (P['solve_groups'] - 1) * P['SOLVE_TRACES'] < systems <= P['solve_groups'] * P['SOLVE_TRACES']
    assert P['mean_blocks'] == ((tnum + P['MEAN_BLOCK'] - 1) // P['MEAN_BLOCK'] if design else 0)
    # LDS: below the 64 KiB a launch may ask for without an attribute
    assert P['acorr_lds'] == (3 * R.C - 1) * P['TG'] * 8 == P['apply_lds'] and P['acorr_lds'] <= 65536
    assert P['solve_lds'] == 5 * oplen * P['SOLVE_TRACES'] * 8 <= 65536
    # scratch: the lag table and the operators, (|lags| + oplen) tnum doubles, then the mean's sums and the flags
    assert P['off_op'] == nl * tnum * 8 and P['off_mean'] == (nl + oplen) * tnum * 8
    mean_doubles = (P['mean_blocks'] + 1) * nl + oplen if design else 0
    assert P['off_dead'] - P['off_mean'] == (mean_doubles * 8 + 15) // 16 * 16
    assert P['scratch_bytes'] - P['off_dead'] == ((tnum + 1) * 4 + 15) // 16 * 16
    assert ('decon_mean_kernel' in P['label']) == bool(design) and 'decon_acorr_kernel' in P['label'] and 'decon_apply_kernel' in P['label']


@pytest.mark.skipif(not os.path.exists(os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')), reason='hipcc not installed')
def test_every_new_header_compiles_alone(tmp_path):
    """decon_core.h, decon_route.h and decon_kernels.h as the only include of a translation unit (host and device pass)."""
    procs = []
    for h in ('decon_core.h', 'decon_route.h', 'decon_kernels.h'):
        src = str(tmp_path / (h[:-2] + '_alone.hip'))
        with open(src, 'w') as f:
            f.write('#include "%s"\n' % h)
        procs.append((h, subprocess.Popen([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '--offload-arch=gfx950', '-std=c++17', '-fsyntax-only',
                                           '-I', CSRC, src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for h, pr in procs:
        log = pr.communicate(timeout=600)[0]
        assert pr.returncode == 0, (h, log[-2000:])


def test_the_unit_takes_everything_from_the_route():
    text = open(os.path.join(CSRC, 'decon.hip')).read()
    assert 'decon_refusal(' in text and 'acorr_refusal(' in text and 'decon_plan(' in text and 'acorr_plan(' in text
    assert text.count('static int decon_check(') == 1 and text.count('decon_check(ctx') == 2      # one check, called by both forms
    assert 'host_form' in text and 'rw_dispatch' in text
    kernels = open(os.path.join(CSRC, 'decon_kernels.h')).read()
    assert 'atomicAdd' not in kernels and 'atomicAdd' not in text
