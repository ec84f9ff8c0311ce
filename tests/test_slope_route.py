"""The host-side route of the layer-slope steps (csrc/slope_route.h, compiled here by itself with g++: no GPU, no HIP): every
refusal with its wording, the radii and the weight table, the launch geometry, the LDS and the scratch sizes."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import slope_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, 'impdar_amd', 'csrc')
pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not installed')

IKEYS = ('rz', 'rx', 'ok', 'row_threads', 'col_threads', 'gather_threads', 'col_tx', 'col_seg')
LKEYS = ('row_blocks_x', 'row_blocks', 'row_lds', 'col_blocks_x', 'col_blocks_z', 'col_blocks', 'col_lds', 'gather_blocks', 'plane_bytes',
         'field_bytes', 'inplace_bytes')
LDS_MAX = 160 * 1024

MAIN = r'''
#define SLOPE_ROUTE_PROBE
#include "slope_route.h"
#include <cstdio>
// every refusal, every radius' weight table and a walk over many shapes: what a sanitizer has to see
int main()
{
    int bad = 0;
    bad += slope_refusal(100, 8, 0, 2.0, 8.0, 4.0) != nullptr;
    bad += slope_refusal(100, 8, 6, 2.0, 8.0, 4.0) == nullptr;
    bad += slope_refusal(100, 8, 0, NAN, 8.0, 4.0) == nullptr;
    bad += slope_refusal(100, 8, 0, 2.0, 16.5, 4.0) == nullptr;
    bad += slope_refusal(100, 8, 0, 2.0, 8.0, 0.0) == nullptr;
    bad += slope_refusal(0, 8, 0, 2.0, 8.0, 4.0) == nullptr;
    bad += dipsmooth_refusal(100, 8, 33, true, NAN, NAN, NAN) == nullptr;
    bad += dipsmooth_refusal(100, 8, 32, true, NAN, NAN, NAN) != nullptr;
    double w[2 * SLOPE_MAX_R + 1];
    double total = 0;
    for (double s = 0.0; s <= 16.0; s += 0.125) {
        int r = -1;
        slope_weights(s, w, &r);
        if (r != (int)(4.0 * s + 0.5) || r > SLOPE_MAX_R) ++bad;
        for (int i = 0; i <= 2 * r; ++i) total += w[i];
    }
    long long sum = 0;
    for (int n = 1; n <= 9000; n += (n < 200 ? 1 : 97))
        for (int t = 1; t <= 20000; t = t * 3 + 1)
            for (double s = 0.0; s <= 16.0; s += 4.0) {
                const SlopeRoute S = slope_route(n, t, s, 16.0 - s, 4);
                if (!S.ok || S.row_lds > (size_t)SLOPE_LDS_MAX || S.col_lds > (size_t)SLOPE_LDS_MAX) { ++bad; continue; }
                if (S.row_blocks_x * SLOPE_ROW_TX < t || S.col_blocks_x * SLOPE_COL_TX < t || S.col_blocks_z * SLOPE_COL_SEG < n) ++bad;
                sum += S.row_blocks + S.col_blocks + S.gather_blocks;
            }
    printf("bad %d sum %lld total %.3f\n", bad, sum, total);
    return bad != 0;
}
'''


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('sloperoute'))
    src, so = os.path.join(tmp, 'slope_route_probe.cpp'), os.path.join(tmp, 'libsloperoute.so')
    with open(src, 'w') as f:
        f.write('#define SLOPE_ROUTE_PROBE\n#include "slope_route.h"\n')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-shared', '-fPIC', '-I', CSRC, src, '-o', so])
    lib = C.CDLL(so)
    lib.slope_probe_refusal.restype = C.c_char_p
    lib.slope_probe_refusal.argtypes = [C.c_int] * 3 + [C.c_double] * 3
    lib.dipsmooth_probe_refusal.restype = C.c_char_p
    lib.dipsmooth_probe_refusal.argtypes = [C.c_int] * 4 + [C.c_double] * 3
    lib.slope_probe_weights.restype = C.c_int
    lib.slope_probe_weights.argtypes = [C.c_double, C.POINTER(C.c_double)]
    lib.slope_probe_route.restype = C.c_int
    lib.slope_probe_route.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    return lib


def refusal(lib, snum=100, tnum=8, kind=0, sigma_z=2.0, sigma_x=8.0, max_slope=4.0):
    why = lib.slope_probe_refusal(snum, tnum, kind, sigma_z, sigma_x, max_slope)
    return None if why is None else why.decode()


def refusal_ds(lib, snum=100, tnum=8, half=4, given=0, sigma_z=2.0, sigma_x=8.0, max_slope=4.0):
    why = lib.dipsmooth_probe_refusal(snum, tnum, half, given, sigma_z, sigma_x, max_slope)
    return None if why is None else why.decode()


def route(lib, snum, tnum, sigma=(2.0, 8.0), elem=4):
    ints, longs = np.zeros(8, dtype=np.int32), np.zeros(11, dtype=np.int64)
    lib.slope_probe_route(snum, tnum, sigma[0], sigma[1], elem, ints.ctypes.data_as(C.POINTER(C.c_int)), longs.ctypes.data_as(C.POINTER(C.c_longlong)))
    return dict(zip(IKEYS, ints.tolist()), **dict(zip(LKEYS, longs.tolist())))


def python_reason(call):
    with pytest.raises(ValueError) as e:
        call()
    return str(e.value)


def test_every_refusal_has_its_reason_and_python_words_it_the_same(lib):
    from impdar_amd import slope as S
    for kind in range(6):
        assert refusal(lib, kind=kind) is None
    why = 'kind must be 0 (slope), 1 (dip), 2 (coherence), 3 (jzz), 4 (jzx) or 5 (jxx)'
    assert refusal(lib, kind=-1) == refusal(lib, kind=6) == why
    assert python_reason(lambda: S.check_slope((100, 8), 6)).startswith(why)
    assert python_reason(lambda: S.check_slope((100, 8), 'power')).startswith(why)
    why = 'sigma must be finite and lie in 0 .. 16'
    for bad in (-0.5, 16.001, float('nan'), float('inf')):
        assert refusal(lib, sigma_z=bad) == refusal(lib, sigma_x=bad) == refusal_ds(lib, sigma_z=bad) == refusal_ds(lib, sigma_x=bad) == why, bad
        assert python_reason(lambda: S.check_slope((100, 8), 0, (bad, 1.0))).startswith(why)
        assert python_reason(lambda: S.check_dipsmooth((100, 8), 4, (1.0, bad))).startswith(why)
        assert refusal_ds(lib, given=1, sigma_z=bad, sigma_x=bad) is None          # (not read with a given slope)
    for good in (0.0, 0.5, 16.0):
        assert refusal(lib, sigma_z=good, sigma_x=good) is None
    why = 'max_slope must be finite and positive'
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        assert refusal(lib, max_slope=bad) == refusal_ds(lib, max_slope=bad) == why
        assert python_reason(lambda: S.check_slope((100, 8), 0, (2.0, 8.0), bad)).startswith(why)
        assert python_reason(lambda: S.check_dipsmooth((100, 8), 4, (2.0, 8.0), bad)).startswith(why)
    why = 'half must lie in 1 .. 32'
    for bad in (0, -1, 33):
        assert refusal_ds(lib, half=bad) == refusal_ds(lib, half=bad, given=1) == why
        assert python_reason(lambda: S.check_dipsmooth((100, 8), bad)).startswith(why)
    assert refusal_ds(lib, half=1) is None and refusal_ds(lib, half=32) is None
    why = 'empty radargram'
    for shape in ((0, 8), (100, 0)):
        assert refusal(lib, *shape) == refusal_ds(lib, *shape) == why
        assert python_reason(lambda: S.check_slope(shape)).startswith(why)
        assert python_reason(lambda: S.check_dipsmooth(shape, 4)).startswith(why)
    assert refusal(lib, 1, 1) is None and refusal_ds(lib, 1, 1) is None
    # a grid past 2^31 blocks: the row pass has one block per row and 256 traces
    assert refusal(lib, 2 ** 31 - 1, 257) == refusal_ds(lib, 2 ** 31 - 1, 257) == 'radargram too large: a grid would pass 2^31 blocks'
    assert refusal(lib, 2 ** 30, 256) is None


def test_constants_are_the_yardsticks(lib):
    r = route(lib, 100, 100)
    assert (r['row_threads'], r['col_tx'], r['col_seg']) == (R.ROW_TX, R.COL_TX, R.COL_SEG)
    assert r['col_threads'] % r['col_tx'] == 0 and r['col_seg'] % (r['col_threads'] // r['col_tx']) == 0
    assert python_max() == (16.0, 32)


def python_max():
    from impdar_amd import slope as S
    return S.MAX_SIGMA, S.MAX_HALF


def test_radii_and_weights(lib):
    w = np.zeros(2 * R.MAX_R + 1)
    for sigma in [0.0, 0.1, 0.124, 0.125, 0.5, 1.0, 2.0, 3.0, 4.0, 7.9, 8.0, 15.9, 16.0] + [0.37 * k for k in range(1, 43)]:
        r = lib.slope_probe_weights(sigma, w.ctypes.data_as(C.POINTER(C.c_double)))
        assert r == int(4 * sigma + 0.5) == R.radius(sigma) and r <= R.MAX_R
        got = w[:2 * r + 1]
        want = R.weights(sigma)
        ulp = np.spacing(want)
        assert np.all(np.abs(got - want) <= 2 * ulp), sigma
        assert abs(float(np.sum(got.astype(np.longdouble))) - 1.0) <= 4 * np.spacing(1.0), sigma
        assert np.array_equal(got, got[::-1])
        if r == 0:
            assert got[0] == 1.0
        else:
            from scipy.ndimage import _filters
            # SciPy forms the exponent as (-0.5 / sigma^2) i^2: two more roundings of a number of size <= 8.5, each one worth that
            # many ulp of the weight
            ref = _filters._gaussian_kernel1d(sigma, 0, r)
            assert np.all(np.abs(got - ref) <= 20 * np.spacing(ref)), sigma
    assert route(lib, 50, 50, (16.0, 16.0))['rz'] == R.MAX_R


@pytest.mark.parametrize('sigma', R.SIGMAS + (R.WIDE[1],), ids=str)
def test_geometry_lds_and_scratch(lib, sigma):
    shapes = list(R.CASES) + [R.WIDE[0], (4096, 10000), (1, 100000), (100000, 1)]
    for snum, tnum in shapes:
        for elem in (4, 8):
            r = route(lib, snum, tnum, sigma, elem)
            assert r['ok'] == 1 and (r['rz'], r['rx']) == (R.radius(sigma[0]), R.radius(sigma[1]))
            assert r['row_blocks_x'] == -(-tnum // R.ROW_TX) and r['row_blocks'] == r['row_blocks_x'] * snum
            assert r['col_blocks_x'] == -(-tnum // R.COL_TX) and r['col_blocks_z'] == -(-snum // R.COL_SEG)
            assert r['col_blocks'] == r['col_blocks_x'] * r['col_blocks_z']
            assert r['gather_blocks'] == -(-(snum * tnum) // r['gather_threads'])
            assert max(r['row_blocks'], r['col_blocks'], r['gather_blocks']) < 2 ** 31
            assert r['row_lds'] == 3 * (R.ROW_TX + 2 * r['rx']) * 8 <= LDS_MAX
            assert r['col_lds'] == (R.COL_SEG + 2 * r['rz']) * R.COL_TX * 8 <= LDS_MAX
            assert r['plane_bytes'] == 24 * snum * tnum and r['field_bytes'] == 8 * snum * tnum and r['inplace_bytes'] == elem * snum * tnum
    assert route(lib, 4096, 10000)['plane_bytes'] == 983040000           # 0.98 GB at the headline shape


def test_route_header_under_sanitizers(tmp_path):
    """The header's own code (refusals, weights, route) in a stand-alone program under the address and undefined-behaviour
    sanitizers."""
    src, exe = str(tmp_path / 'slope_route_main.cpp'), str(tmp_path / 'slope_route_main')
    with open(src, 'w') as f:
        f.write(MAIN)
    base = ['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-I', CSRC, src, '-o', exe]
    if subprocess.call(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base)             # (a compiler without the run times: the program still has to pass)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith('bad 0 '), out.stdout[-2000:]
