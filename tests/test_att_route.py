"""The host-side route of the attenuation window search (csrc/att_route.h, compiled here by itself with g++: no GPU, no
HIP): what impdar_att_search_plan and impdar_att_search accept and reject before any device work, the launch and the
device bytes."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, 'impdar_amd', 'csrc')
needs_gxx = pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not installed')
pytestmark = needs_gxx

INDEX, DEPTH = 0, 1
KEYS = ('threads', 'workgroups', 'parts', 'chunk', 'in_doubles', 'out_doubles', 'out_ints', 'scratch_bytes')


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('attroute'))
    src, so = os.path.join(tmp, 'att_route_probe.cpp'), os.path.join(tmp, 'libattroute.so')
    with open(src, 'w') as f:
        f.write('#define ATT_ROUTE_PROBE 1\n#include "att_route.h"\n')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-shared', '-fPIC', '-I', CSRC, src, '-o', so])
    lib = C.CDLL(so)
    lib.impdar_att_route_full_probe.argtypes = [C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_double, C.c_double, C.c_longlong,
                                                C.c_longlong, C.c_longlong, C.c_longlong, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
    return lib


def route(lib, flavour, n, nn, ncent, win_init=100., win_step=100., probe=-1, probe_cap=0, j0=0, first=0, z=None):
    longs = (C.c_longlong * 8)()
    p = None if z is None else np.ascontiguousarray(z, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    rc = lib.impdar_att_route_full_probe(flavour, n, nn, ncent, win_init, win_step, probe, probe_cap, j0, first, p, longs)
    r = dict(zip(KEYS, list(longs)))
    r['rc'] = rc
    return r


def test_accepted_sizes_and_their_launch(lib):
    for flavour in (INDEX, DEPTH):
        for n, nn, ncent in ((1, 1, 1), (2, 2, 1), (400, 30, 380), (1000, 63, 950), (1000, 64, 5), (1000, 65, 5), (10000, 30, 9900),
                             (10000, 128, 7), (10000, 129, 7), (10000, 255, 7), (10000, 256, 7), (10000, 1000, 7), (1 << 40, 30, (1 << 31) - 1)):
            for probe, cap in ((-1, 0), (0, 1), (ncent - 1, 37)):
                r = route(lib, flavour, n, nn, ncent, probe=probe, probe_cap=cap)
                assert r['rc'] == 0, (flavour, n, nn, ncent, probe)
                # one workgroup of 256 threads per centre; a thread owns one rate and one of `parts` parts of a window
                assert r['threads'] == 256 and r['workgroups'] == ncent
                assert r['chunk'] == min(nn, 256) and r['parts'] == max(1, 256 // nn) and r['parts'] * r['chunk'] <= 256
                assert r['in_doubles'] == 2 * n + nn + (ncent if flavour == DEPTH else 0)
                assert r['out_doubles'] == ncent * nn + 2 * ncent + cap * nn + 1 and r['out_ints'] == ncent
                # 10 blocks, each rounded up to 16 bytes
                need = 8 * (r['in_doubles'] + r['out_doubles']) + 4 * ncent
                assert need <= r['scratch_bytes'] <= need + 10 * 16
    # a probe's row bound is not looked at without a probe
    assert route(lib, INDEX, 400, 30, 380, probe=-1, probe_cap=1 << 62) == route(lib, INDEX, 400, 30, 380)


def test_rejected_sizes(lib):
    for flavour in (INDEX, DEPTH):
        for n, nn, ncent in ((0, 30, 5), (-1, 30, 5), (400, 0, 5), (400, -2, 5), (400, 30, 0), (400, 30, -7),
                             (400, 30, 1 << 31),                        # more centres than a launch has workgroups
                             (1 << 62, 30, 5), (400, 1 << 62, 5),       # byte counts beyond 64 bits
                             (400, 1 << 40, 1 << 30)):                  # ncent x nn x 8 beyond 64 bits
            r = route(lib, flavour, n, nn, ncent)
            assert r['rc'] == 1 and r['workgroups'] == 0 and r['scratch_bytes'] == 0, (flavour, n, nn, ncent)
    assert route(lib, 2, 400, 30, 5)['rc'] == 1 and route(lib, -1, 400, 30, 5)['rc'] == 1
    # the probe's table beyond 64 bits
    assert route(lib, INDEX, 400, 1 << 20, 5, probe=0, probe_cap=1 << 41)['rc'] == 1


def test_widths(lib):
    for wi, ws, rc in ((2, 1, 0), (3, 1, 0), (100, 100, 0), (21, 7, 0), (1, 1, 1), (0, 1, 1), (-4, 1, 1), (2, 0, 1), (2, -1, 1), (2.5, 1, 1),
                       (4, 1.5, 1), (float('nan'), 1, 1), (4, float('nan'), 1), (float('inf'), 1, 1), (4, float('inf'), 1), (2.0 ** 62, 1, 1)):
        assert route(lib, INDEX, 400, 30, 5, win_init=wi, win_step=ws)['rc'] == rc, (wi, ws)
    # (the sizes alone; with z in hand the step is also held against the depth range: test_depth_walk_is_bounded)
    for wi, ws, rc in ((0.1, 0.1, 0), (1e-9, 1e-300, 0), (1.5, 2.5, 0), (0.0, 0.1, 1), (0.1, 0.0, 1), (-0.1, 0.1, 1), (0.1, -0.1, 1),
                       (float('nan'), 0.1, 1), (0.1, float('nan'), 1), (float('inf'), 0.1, 1), (0.1, float('inf'), 1)):
        assert route(lib, DEPTH, 400, 30, 5, win_init=wi, win_step=ws)['rc'] == rc, (wi, ws)


def test_probe_index_and_rows(lib):
    for probe, cap, rc in ((-1, 0, 0), (-7, 0, 0), (0, 1, 0), (4, 9, 0), (5, 9, 1), (1 << 40, 9, 1), (0, 0, 1), (2, -3, 1)):
        assert route(lib, INDEX, 400, 30, 5, probe=probe, probe_cap=cap)['rc'] == rc, (probe, cap)


def test_rate_index_first_trace_and_depth_order(lib):
    for j0, rc in ((0, 0), (29, 0), (30, 1), (-1, 1)):
        assert route(lib, INDEX, 400, 30, 5, j0=j0)['rc'] == rc
    for first, rc in ((0, 0), (10, 0), (1 << 50, 0), (-1, 1), ((1 << 63) - 3, 1)):
        assert route(lib, INDEX, 400, 30, 5, first=first)['rc'] == rc
    assert route(lib, DEPTH, 400, 30, 5, first=-1)['rc'] == 0                                  # (the depth form has no first trace)
    z = np.array([0.1, 0.2, 0.2, 0.35, 1.0])
    assert route(lib, DEPTH, 5, 30, 2, 0.1, 0.1, z=z)['rc'] == 0                               # equal neighbours are accepted
    assert route(lib, DEPTH, 5, 30, 2, 0.1, 0.1, z=z[::-1])['rc'] == 1
    nan = z.copy()
    nan[2] = np.nan
    assert route(lib, DEPTH, 5, 30, 2, 0.1, 0.1, z=nan)['rc'] == 1
    assert route(lib, INDEX, 5, 30, 2, 2, 1, z=z[::-1])['rc'] == 0                             # the index form takes the pick's own order


def test_depth_walk_is_bounded(lib):
    """A depth walk is accepted only when it must end: finite ends of z, a step that still moves a width of twice the depth
    range when halved, and no more than 2^20 steps across the range."""
    z = np.array([1.0, 1.2, 1.5, 2.0])
    for ws, rc in ((0.1, 0), (1e-5, 0), (2.0 ** -20, 0), (2.0 ** -20 * (1 - 1e-9), 1), (1e-9, 1),      # 2^20 steps across 1.0
                   (1e-17, 1), (2.0 ** -52, 1), (1e-300, 1)):                                          # absorbed by a width of 2.0
        assert route(lib, DEPTH, 4, 30, 2, 0.2, ws, z=z)['rc'] == rc, ws
    wide = np.array([0.0, 2.0 ** 60])
    assert route(lib, DEPTH, 2, 30, 2, 1.0, 2.0 ** 41, z=wide)['rc'] == 0                              # 2^19 steps, far above an ulp of 2^61
    assert route(lib, DEPTH, 2, 30, 2, 1.0, 2.0 ** 39, z=wide)['rc'] == 1                              # 2^21 steps
    huge = np.array([0.0, 1e300])
    assert route(lib, DEPTH, 2, 30, 2, 1.0, 1e295, z=huge)['rc'] == 0 and route(lib, DEPTH, 2, 30, 2, 1.0, 1.0, z=huge)['rc'] == 1
    for bad in (np.array([1.0, 1.5, np.inf]), np.array([-np.inf, 1.5, 2.0]), np.array([-np.inf, np.inf]), np.array([-1.7e308, 1.7e308])):
        assert route(lib, DEPTH, len(bad), 30, 2, 0.2, 0.1, z=bad)['rc'] == 1, bad
    assert route(lib, DEPTH, 3, 30, 2, 0.2, 0.1, z=np.array([1.5, 1.5, 1.5]))['rc'] == 0                # no range: no window is visited
    # the index form walks integers over n elements: its z may hold anything
    assert route(lib, INDEX, 3, 30, 2, 2, 1, z=np.array([1.0, np.inf, 0.5]))['rc'] == 0


def test_unit_decides_nothing_itself():
    """attsearch.hip takes threads, workgroups, parts and every check from the route; the library's plan call is the route's."""
    text = open(os.path.join(CSRC, 'attsearch.hip')).read()
    assert '#include "att_route.h"' in text
    assert text.count('dim3((unsigned)R.workgroups), dim3(R.threads)') == 2
    assert text.count('att_route(flavour, n, nn, ncent, win_init, win_step, probe, probe_cap)') == 2
    assert 'att_call_ok(R, j0, first)' in text and 'att_depths_bad(z, n)' in text and 'att_depth_walk_bad(z[0], z[n - 1], win_step)' in text and 'A.parts = R.parts' in text and 'A.chunk = R.chunk' in text
    header = open(os.path.join(CSRC, 'att_route.h')).read()
    assert 'hip/' not in header and '__global__' not in header
