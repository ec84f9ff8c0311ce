"""The cases of the Stolt call's host-side route (test infrastructure, shared by tests/test_stolt_route.py and
tests/test_stolt_route_gpu.py): sizes, wavenumber axes and values of IMPDAR_STOLT_FFT that reach every branch of
csrc/stolt_route.h, the header compiled by itself with g++ behind a few extern "C" wrappers, and one call of a case through the
library.  What the library reported on the GPU for the cases marked gpu, at the commit before the route was split out of
csrc/stolt.hip, is in tests/stolt_route_recorded.json."""
import contextlib
import ctypes as C
import json
import os

import numpy as np

RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'stolt_route_recorded.json')
ROCFFT, WKX, ROWS = 0, 1, 2
VELS = 1.68e8 * np.array([0.8, 0.9, 1.0, 1.1, 1.25])
HT, VT = 7, 11
KNOB = 'IMPDAR_STOLT_FFT'
WORDS = (None, 'own', 'mixed', 'rocfft', '1d', 'fastest')          # ('fastest': a word the library does not know)


def case(snum, tnum, dtype='float32', knob=None, kx='fft', scan=None, gpu=False, note=''):
    """scan: None, or the max_batch of a scan of the five VELS."""
    name = '%dx%d-%s' % (snum, tnum, dtype) + ('-' + knob if knob else '') + ('-bent' if kx == 'bent' else '') + \
           ('-scan%d' % scan if scan is not None else '')
    return dict(id=name, snum=snum, tnum=tnum, dtype=dtype, knob=knob, kx=kx, scan=scan, gpu=gpu, note=note)


def _cases():
    out = []
    # the smallest shapes at which each route is reached (gpu): power of two on both sides of tnum >= 64; odd snum; a small size
    # that is no power of two; a length above 1024; the knob; an odd number of traces
    out.append(case(64, 64, scan=2, gpu=True))
    out.append(case(64, 64, 'float64', gpu=True))
    out.append(case(64, 32, scan=0, gpu=True))
    out.append(case(65, 50, scan=0, gpu=True))
    out.append(case(100, 48, gpu=True))
    out.append(case(96, 2400, scan=0, gpu=True))
    out.append(case(96, 160, knob='mixed', gpu=True))
    out.append(case(96, 160, gpu=True))
    out.append(case(96, 1125, gpu=True))
    out.append(case(96, 2400, kx='bent', gpu=True))
    out.append(case(64, 64, knob='rocfft', gpu=True))
    out.append(case(64, 64, knob='1d', gpu=True))
    # every word of the knob at a power-of-two size and at one that is none
    for word in WORDS:
        for snum, tnum in ((64, 64), (96, 160)):
            if (word, snum) not in ((None, 64), ('rocfft', 64), ('1d', 64), (None, 96), ('mixed', 96)):
                out.append(case(snum, tnum, knob=word))
    # power-of-two sizes on both sides of own_fft_len_ok: of snum (rows), of snum / 2 and of tnum ([w][kx])
    out += [case(8192, 64), case(16384, 64), case(32768, 64), case(16, 64), case(32, 64), case(64, 8), case(64, 16), case(64, 16384)]
    # the rows route is taken at power-of-two sizes without the kx[k] == -kx[tnum - k] check of the mixed-radix
    # branch.  The parent does so and this case pins it; the fix turns its expected route into [w][kx] on purpose.
    out.append(case(64, 64, kx='bent', note='ADVICE round 6'))
    out.append(case(64, 64, knob='mixed', kx='bent', note='ADVICE round 6'))
    # sizes that are no power of two: the gate at 1024 on either axis, and the rows form refused for each of its reasons -- an odd
    # tnum (above), tnum < 64, snum out of the kernel's range, kx not antisymmetric (above), a prime factor above 7 in tnum / 2 or
    # in snum (the [w][kx] form is refused with it)
    out += [case(1500, 64), case(1024, 96), case(96, 1024), case(1080, 96), case(96, 1080)]
    out += [case(120, 60, knob='mixed'), case(9600, 64), case(96, 1144), case(1100, 64), case(96, 160, knob='mixed', kx='bent')]
    out += [case(88, 160, knob='mixed'), case(96, 176, knob='mixed'), case(96, 20, knob='mixed'), case(20, 96, knob='mixed')]
    # odd and even sizes on both axes (the shape), and the smallest the entry points take
    out += [case(65, 51), case(64, 51), case(2, 1), case(3, 2, 'float64')]
    return out


CASES = _cases()
IDS = [c['id'] for c in CASES]
GPU_CASES = [c for c in CASES if c['gpu']]
assert len(set(IDS)) == len(IDS)

# The batches of a scan: (snum, tnum, dtype, knob, nv, max_batch).  4096 x 4096 on the rows route: the budget decides; then
# nv, max_batch (a ragged last batch) and STOLT_SCAN_MAX_BATCH; rocFFT (no spectra of the scan's own); the smallest snum.
SCAN_CASES = [(4096, 4096, 'float32', None, 64, 0), (4096, 4096, 'float64', None, 64, 0), (4096, 4096, 'float32', None, 64, 7),
              (64, 64, 'float32', None, 5, 0), (64, 64, 'float32', None, 5, 2), (64, 64, 'float64', None, 3000, 0),
              (64, 32, 'float32', None, 5, 0), (65, 50, 'float64', None, 5, 0), (4096, 4096, 'float32', 'rocfft', 64, 0),
              (2, 1, 'float32', None, 5, 0), (96, 2400, 'float32', None, 9, 4)]


def kx_of(c):
    """The wavenumbers of a case: mig_hip._kx on synth.geometry's unit trace spacing; 'bent': one of them off its mirror image."""
    kx = np.ascontiguousarray(2. * np.pi * np.fft.fftfreq(c['tnum'], d=1.0))
    if c['kx'] == 'bent' and c['tnum'] > 1:
        kx[1] *= 1.01
    return kx


def knob_flags(word):
    """(use2d, no_own, want_mixed) of a value of IMPDAR_STOLT_FFT, as stolt_prepare read it."""
    return int(word != '1d'), int(word == 'rocfft'), int(word == 'mixed')


# ---- the host-only header compiled by itself
PROBE = r'''
#include "stolt_route.h"
static StoltKnobs knobs(const int *k)
{
    StoltKnobs K;
    K.use2d = k[0] != 0;
    K.no_own = k[1] != 0;
    K.want_mixed = k[2] != 0;
    return K;
}
// out[10]: route, m, nz, nout, hs, use_own, mixed, elements of X, of F / K, of Y
extern "C" void stolt_probe_shape(int dtype, int snum, int tnum, const double *kx, const int *k, long long *out)
{
    const StoltShape s = stolt_shape(dtype, snum, tnum, stolt_route(snum, tnum, kx, knobs(k)));
    const long long v[10] = {s.route, s.m, s.nz, s.nout, s.hs, s.use_own, s.mixed, (long long)s.x_elems, (long long)s.spec_elems, (long long)s.y_elems};
    for (int i = 0; i < 10; ++i) out[i] = v[i];
}
// out[5]: plane, iplane, bytes per velocity, B, batches
extern "C" void stolt_probe_scan(int dtype, int snum, int tnum, const double *kx, const int *k, int nv, int max_batch, long long *out)
{
    const StoltShape s = stolt_shape(dtype, snum, tnum, stolt_route(snum, tnum, kx, knobs(k)));
    const StoltScanPlan p = stolt_scan_plan(s, dtype ? 8 : 4, nv, max_batch);
    const long long v[5] = {(long long)p.plane, (long long)p.iplane, (long long)p.per, p.B, p.batches};
    for (int i = 0; i < 5; ++i) out[i] = v[i];
}
extern "C" const char *stolt_probe_label(int snum, int tnum, int route, int scan)
{
    return stolt_kernel_label(stolt_shape(0, snum, tnum, (StoltRoute)route), scan != 0);
}
// a, b: owner, dtype, snum, tnum, use2d, no_own, route
extern "C" int stolt_probe_key_eq(const long long *a, const long long *b)
{
    const StoltPlanKey x{(const void *)a[0], (int)a[1], (int)a[2], (int)a[3], a[4] != 0, a[5] != 0, (int)a[6]};
    const StoltPlanKey y{(const void *)b[0], (int)b[1], (int)b[2], (int)b[3], b[4] != 0, b[5] != 0, (int)b[6]};
    return x == y;
}
extern "C" long long stolt_probe_budget() { return (long long)STOLT_SCAN_BUDGET_BYTES; }
extern "C" int stolt_probe_max_batch() { return STOLT_SCAN_MAX_BATCH; }
'''
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'impdar_amd', 'csrc')


def probe(tmpdir):
    import subprocess
    src, lib = os.path.join(tmpdir, 'stolt_route_probe.cpp'), os.path.join(tmpdir, 'libstoltroute.so')
    with open(src, 'w') as f:
        f.write(PROBE)
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-shared', '-fPIC', '-I', CSRC, src, '-o', lib])
    lib = C.CDLL(lib)
    lib.stolt_probe_label.restype = C.c_char_p
    lib.stolt_probe_budget.restype = C.c_longlong
    return lib


_dp, _ip, _lp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_longlong)
SHAPE = ('route', 'm', 'nz', 'nout', 'hs', 'use_own', 'mixed', 'x_elems', 'spec_elems', 'y_elems')
SCAN = ('plane', 'iplane', 'per', 'B', 'batches')


def _args(c):
    kx, k = kx_of(c), np.array(knob_flags(c['knob']), dtype=np.int32)
    return (int(c['dtype'] == 'float64'), c['snum'], c['tnum'], kx.ctypes.data_as(_dp), k.ctypes.data_as(_ip)), (kx, k)


def shape(lib, c):
    out = np.zeros(len(SHAPE), dtype=np.int64)
    args, alive = _args(c)
    lib.stolt_probe_shape(*args, out.ctypes.data_as(_lp))
    return dict(zip(SHAPE, out.tolist()))


def scan_plan(lib, c, nv, max_batch):
    out = np.zeros(len(SCAN), dtype=np.int64)
    args, alive = _args(c)
    lib.stolt_probe_scan(*args, int(nv), int(max_batch), out.ctypes.data_as(_lp))
    return dict(zip(SCAN, out.tolist()))


def label(lib, snum, tnum, route, scan):
    return lib.stolt_probe_label(snum, tnum, route, int(scan)).decode()


def labels_of(lib, c):
    """What the metrics line of case c must say: (kernel of the single call, kernel of its scan, B of its scan); None without a scan."""
    r = shape(lib, c)['route']
    if c['scan'] is None:
        return label(lib, c['snum'], c['tnum'], r, False), None, None
    return label(lib, c['snum'], c['tnum'], r, False), label(lib, c['snum'], c['tnum'], r, True), scan_plan(lib, c, len(VELS), c['scan'])['B']


# ---- one call of a case through the library (GPU)
@contextlib.contextmanager
def knob(word):
    old = os.environ.pop(KNOB, None)
    if word is not None:
        os.environ[KNOB] = word
    try:
        yield
    finally:
        os.environ.pop(KNOB, None)
        if old is not None:
            os.environ[KNOB] = old


def last_metrics():
    from impdar_amd import _hip
    buf = C.create_string_buffer(1024)
    _hip.check(_hip.load().impdar_ctx_last_metrics(_hip.context(), buf, len(buf)), 'metrics')
    return json.loads(buf.value.decode())


def run(c):
    """One migrate('stolt') of a noise radargram under the case's knob -- with its own wavenumbers through the C entry point
    that migrate calls -- and the case's scan of the five VELS: (kernel, scan kernel, B) of the metrics lines, as labels_of."""
    from impdar_amd import _hip, synth, velscan
    from impdar_amd.lib.RadarData import RadarData
    snum, tnum = c['snum'], c['tnum']
    geo = synth.geometry(snum, tnum)
    d = RadarData(None)
    d.data, d.snum, d.tnum = synth.noise_radargram(snum, tnum, seed=snum + tnum).astype(c['dtype']), snum, tnum
    d.travel_time, d.dist, d.trace_int, d.dt = geo['travel_time'], geo['dist'], geo['trace_int'], geo['dt']
    with knob(c['knob']):
        scan_kernel = batch = None
        if c['scan'] is not None:
            velscan.stolt_velocity_scan(d, VELS, htaper=HT, vtaper=VT, max_batch=c['scan'])
            m = last_metrics()
            scan_kernel, batch = m['kernel'], m['B']
        if c['kx'] == 'fft':
            d.migrate('stolt', vel=1.68e8, htaper=HT, vtaper=VT)
        else:
            kx, ws = kx_of(c), np.ascontiguousarray(2. * np.pi * np.fft.rfftfreq(snum, d=geo['dt']))
            out = np.empty((2 * (snum // 2), tnum), dtype=c['dtype'])
            _hip.check(_hip.load().impdar_stolt(_hip.context(), d.data.ctypes.data_as(C.c_void_p), _hip.dtype_code(d.data.dtype), snum, tnum,
                                                kx.ctypes.data_as(_dp), ws.ctypes.data_as(_dp), 1.68e8, float(HT), float(VT),
                                                out.ctypes.data_as(C.c_void_p)), 'impdar_stolt')
        return last_metrics()['kernel'], scan_kernel, batch
