"""The host-side route of the GPS time-offset search (csrc/gps_route.h, compiled here by itself with g++: no GPU, no HIP):
what impdar_gps_cc_plan and impdar_gps_cc accept and reject before any device work, the launch and the device bytes."""
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


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('gpsroute'))
    src, so = os.path.join(tmp, 'gps_route_probe.cpp'), os.path.join(tmp, 'libgpsroute.so')
    with open(src, 'w') as f:
        f.write('#define GPS_ROUTE_PROBE 1\n#include "gps_route.h"\n')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-shared', '-fPIC', '-I', CSRC, src, '-o', so])
    lib = C.CDLL(so)
    lib.impdar_gps_route_full_probe.argtypes = [C.c_longlong, C.c_longlong, C.c_longlong, C.c_int, C.c_longlong,
                                                C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
    return lib


def route(lib, ngps, tnum, ncand, extrapolate=0, probe=-1, gps_t=None):
    longs = (C.c_longlong * 6)()
    p = None if gps_t is None else np.ascontiguousarray(gps_t, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    rc = lib.impdar_gps_route_full_probe(ngps, tnum, ncand, extrapolate, probe, p, longs)
    r = dict(zip(('threads', 'workgroups', 'in_doubles', 'out_doubles', 'scratch_bytes', 'bad_fix'), list(longs)))
    r['rc'] = rc
    return r


def test_accepted_sizes_and_their_launch(lib):
    for ngps, tnum, ncand in ((2, 1, 1), (2, 2, 3), (5, 3, 7), (64, 257, 5), (3000, 300, 1001), (100000, 10000, 5001),
                              (2, 1, (1 << 31) - 1), (1 << 40, 1 << 20, 1 << 20)):
        for ex in (0, 1):
            r = route(lib, ngps, tnum, ncand, ex)
            assert r['rc'] == 0, (ngps, tnum, ncand)
            # one workgroup of 256 threads per candidate
            assert r['threads'] == 256 and r['workgroups'] == ncand
            assert r['in_doubles'] == 3 * ngps + 3 * tnum + ncand and r['out_doubles'] == 2 * ncand + 2 * tnum
            # 11 blocks, each rounded up to 16 bytes
            need = 8 * (r['in_doubles'] + r['out_doubles'])
            assert need <= r['scratch_bytes'] <= need + 11 * 16


def test_rejected_sizes(lib):
    for ngps, tnum, ncand in ((1, 5, 5), (0, 5, 5), (-3, 5, 5), (5, 0, 5), (5, -1, 5), (5, 5, 0), (5, 5, -2),
                              (5, 5, 1 << 31),                       # more candidates than a launch has workgroups
                              (1 << 62, 5, 5), (5, 1 << 62, 5),       # byte counts beyond 64 bits
                              (5, 1 << 61, (1 << 31) - 1)):           # ncand x tnum beyond 64 bits
        r = route(lib, ngps, tnum, ncand)
        assert r['rc'] == 1 and r['workgroups'] == 0 and r['scratch_bytes'] == 0, (ngps, tnum, ncand)
    assert route(lib, 5, 5, 5, extrapolate=2)['rc'] == 1 and route(lib, 5, 5, 5, extrapolate=-1)['rc'] == 1


def test_probe_index(lib):
    for probe, rc in ((-1, 0), (-7, 0), (0, 0), (4, 0), (5, 1), (1 << 40, 1)):
        assert route(lib, 5, 5, 5, probe=probe)['rc'] == rc, probe


def test_gps_times(lib):
    t = np.array([1.0, 2.0, 2.0, 3.5, 10.0])
    assert route(lib, 5, 3, 2, gps_t=t) == dict(route(lib, 5, 3, 2), rc=0, bad_fix=0)        # equal neighbours are accepted
    down = t.copy()
    down[3] = 1.5
    r = route(lib, 5, 3, 2, gps_t=down)
    assert r['rc'] == 1 and r['bad_fix'] == 4                                               # 1-based: fix 3
    for k in range(5):
        nan = t.copy()
        nan[k] = np.nan
        r = route(lib, 5, 3, 2, gps_t=nan)
        assert r['rc'] == 1 and r['bad_fix'] == k + 1
    assert route(lib, 2, 3, 2, gps_t=np.array([-np.inf, np.inf]))['rc'] == 0


def test_unit_decides_nothing_itself():
    """gpstrack.hip takes threads, workgroups and every check from the route; the library's plan call is the route's."""
    text = open(os.path.join(CSRC, 'gpstrack.hip')).read()
    assert '#include "gps_route.h"' in text
    assert 'dim3((unsigned)R.workgroups), dim3(R.threads)' in text
    assert text.count('gps_route(ngps, tnum, ncand, extrapolate)') == 2 and 'gps_times_bad(gps_t, ngps)' in text
    header = open(os.path.join(CSRC, 'gps_route.h')).read()
    assert 'hip/' not in header and '__global__' not in header
