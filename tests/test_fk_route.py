"""The host-side route of an f-k call (csrc/fk_route.h, compiled here by itself with g++: no GPU, no HIP): the transforms are
those of a Stolt call at the size, the filtered radargram has snum rows at odd and even snum, the odd ones through an inverse
plan beside Stolt's, the kernel strings name the route, and a fan that is none is refused with a reason."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import stolt_route_cases as SC
from stolt_route_cases import ROCFFT, ROWS, WKX

PROBE = r'''
#include "fk_route.h"
static StoltKnobs knobs(const int *k)
{
    StoltKnobs K;
    K.use2d = k[0] != 0;
    K.no_own = k[1] != 0;
    K.want_mixed = k[2] != 0;
    return K;
}
// out[3]: route, output rows, an inverse plan beside Stolt's
extern "C" void fk_probe_route(int snum, int tnum, const double *kx, const int *k, int *out)
{
    const FkRoute r = fk_route(snum, tnum, kx, knobs(k));
    out[0] = r.route;
    out[1] = r.out_rows;
    out[2] = r.own_inverse_plan;
}
extern "C" const char *fk_probe_label(int snum, int tnum, int route, int power)
{
    return fk_kernel_label(stolt_shape(0, snum, tnum, (StoltRoute)route), power != 0);
}
extern "C" const char *fk_probe_refusal(int snum, int tnum, double va_lo, double va_hi, double taper, int mode, int dip)
{
    return fk_fan_refusal(snum, tnum, va_lo, va_hi, taper, mode, dip);
}
'''


@pytest.fixture(scope='module')
def libs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('fkroute'))
    src, lib = os.path.join(tmp, 'fk_route_probe.cpp'), os.path.join(tmp, 'libfkroute.so')
    with open(src, 'w') as f:
        f.write(PROBE)
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-shared', '-fPIC', '-I', SC.CSRC, src, '-o', lib])
    fk = C.CDLL(lib)
    fk.fk_probe_label.restype = C.c_char_p
    fk.fk_probe_refusal.restype = C.c_char_p
    fk.fk_probe_refusal.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int]
    return fk, SC.probe(tmp)


def fk_route(fk, c):
    kx, k = SC.kx_of(c), np.array(SC.knob_flags(c['knob']), dtype=np.int32)
    out = np.zeros(3, dtype=np.int32)
    fk.fk_probe_route(c['snum'], c['tnum'], kx.ctypes.data_as(C.POINTER(C.c_double)), k.ctypes.data_as(C.POINTER(C.c_int)),
                      out.ctypes.data_as(C.POINTER(C.c_int)))
    return out.tolist()


# the GPU suite's shapes (tests/test_fk_gpu.py) with the route each is there for
GPU_SHAPES = [(64, 64, None, ROWS), (32, 16, None, WKX), (96, 160, 'mixed', ROWS), (96, 75, 'mixed', WKX), (32, 1280, None, ROWS),
              (63, 65, None, ROCFFT), (100, 96, None, ROCFFT), (2, 64, None, ROCFFT), (128, 3, None, ROCFFT)]


@pytest.mark.parametrize('c', SC.CASES, ids=SC.IDS)
def test_route_is_stolts_and_every_row_comes_back(libs, c):
    fk, stolt = libs
    route, rows, beside = fk_route(fk, c)
    assert route == SC.shape(stolt, c)['route']
    assert rows == c['snum']
    assert beside == c['snum'] % 2
    assert not beside or route == ROCFFT            # (odd snum runs on rocFFT alone)


@pytest.mark.parametrize('snum,tnum,word,want', GPU_SHAPES)
def test_the_gpu_suites_shapes_reach_every_route(libs, snum, tnum, word, want):
    fk, _ = libs
    route, rows, beside = fk_route(fk, SC.case(snum, tnum, knob=word))
    assert (route, rows, beside) == (want, snum, snum % 2)


def test_labels_name_the_kernel_and_the_route(libs):
    fk, _ = libs
    seen = set()
    for snum, tnum, route in ((64, 64, ROWS), (96, 160, ROWS), (32, 16, WKX), (96, 75, WKX), (100, 96, ROCFFT)):
        for power in (0, 1):
            label = fk.fk_probe_label(snum, tnum, route, power).decode()
            seen.add(label)
            kernel = {(ROWS, 0): 'fk_fan_rows', (WKX, 0): 'fk_fan_wkx', (ROCFFT, 0): 'fk_fan_kxw', (ROWS, 1): 'fk_power_t',
                      (WKX, 1): 'fk_power_wkx', (ROCFFT, 1): 'fk_power_t'}[(route, power)]
            assert label.startswith(kernel + ' (')
            assert ('rocFFT' in label) == (route == ROCFFT)
            assert ('traces first' in label) == (route == ROWS)
            assert ('mixed radix' in label) == (route != ROCFFT and (snum, tnum) in ((96, 160), (96, 75)))
    assert len(seen) == 10


HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_every_header_of_the_unit_compiles_alone(tmp_path):
    """What csrc/fk.hip includes, each as the only include of a translation unit (host and device pass, syntax only); the two
    host-only ones and the weight also with g++."""
    procs = []
    for h in ('fk_weight.h', 'fk_route.h', 'fk_kernels.h', 'stolt_stages.h'):
        src = str(tmp_path / (h[:-2] + '_alone.hip'))
        with open(src, 'w') as f:
            f.write('#include "%s"\n' % h)
        procs.append((h, subprocess.Popen([HIPCC, '--offload-arch=gfx950', '-std=c++17', '-fsyntax-only', '-I', SC.CSRC, src],
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for h in ('fk_weight.h', 'fk_route.h'):
        src = str(tmp_path / (h[:-2] + '_alone.cpp'))
        with open(src, 'w') as f:
            f.write('#include "%s"\n' % h)
        procs.append((h + ' (g++)', subprocess.Popen(['g++', '-std=c++17', '-Wall', '-Werror', '-fsyntax-only', '-I', SC.CSRC, src],
                                                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    failed = {}
    for h, pr in procs:
        log = pr.communicate(timeout=600)[0]
        if pr.returncode != 0:
            failed[h] = log[-2000:]
    assert not failed, '\n'.join('%s:\n%s' % kv for kv in sorted(failed.items()))


NAN = float('nan')


@pytest.mark.parametrize('args', [
    (8, 8, NAN, NAN, 0.1, 0, 0),
    (8, 8, 0.0, NAN, 0.1, 0, 0), (8, 8, -1.0, NAN, 0.1, 0, 0), (8, 8, math.inf, NAN, 0.1, 0, 0),
    (8, 8, NAN, 0.0, 0.1, 0, 0), (8, 8, NAN, math.inf, 0.1, 0, 0),
    (8, 8, 1.0, NAN, -0.1, 0, 0), (8, 8, 1.0, NAN, 1.0, 0, 0), (8, 8, 1.0, NAN, NAN, 0, 0),
    (8, 8, 1.0, 1.1, 0.1, 0, 0), (8, 8, 2.0, 1.0, 0.0, 0, 0),
    (1, 8, 1.0, NAN, 0.1, 0, 0), (8, 1, 1.0, NAN, 0.1, 0, 0),
    (8, 8, 1.0, NAN, 0.1, 2, 0), (8, 8, 1.0, NAN, 0.1, 0, 3), (8, 8, 1.0, NAN, 0.1, -1, 0), (8, 8, 1.0, NAN, 0.1, 0, -1),
])
def test_what_is_no_fan_is_refused_with_a_reason(libs, args):
    fk, _ = libs
    why = fk.fk_probe_refusal(*args)
    assert why and len(why) > 8


@pytest.mark.parametrize('args', [
    (2, 2, 1.0, NAN, 0.0, 0, 0), (8, 8, NAN, 1.0, 0.5, 1, 2), (8, 8, 1.0, 4.0, 0.5, 0, 1), (8, 8, 4.0, 4.0, 0.0, 1, 0),
    (63, 65, 1.0e8, 1.0e9, 0.1, 0, 0),
])
def test_a_fan_is_taken(libs, args):
    fk, _ = libs
    assert fk.fk_probe_refusal(*args) is None
