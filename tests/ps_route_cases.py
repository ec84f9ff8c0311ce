"""The recorded-choice cases of the phase shift (test infrastructure, shared by tests/test_ps_route.py and
tests/test_ps_route_gpu.py): the smallest shapes that reach every branch of the host-side route (csrc/ps_route.h), the
inputs of each, and one call of impdar_phaseshift_dev with its metrics line.  What the library reported for each case at
the commit before the route was split out is in tests/ps_route_recorded.json."""
import ctypes as C
import json
import os

import numpy as np

RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ps_route_recorded.json')
FIELDS = ('kernel', 'hermitian_walk', 'frequencies', 'transforms', 'long_runs', 'spectrum')
SNUM, DT, DX = 128, 1.0e-8, 1.0
VELOCITIES = ('const', 'tab3', 'tab6', 'many', 'gradient')
KNOBS = ('IMPDAR_PS_MFMA', 'IMPDAR_PS_FFT', 'IMPDAR_PS_HERMITIAN', 'IMPDAR_PS_TEST_EDGE_OVERFLOW')


def _cases():
    out = []
    # every velocity structure and dtype at the default knobs: 64 own transforms, 96 rocFFT's, 512 the row order; nt 192 the complex walk
    for tnum, nt in ((64, 256), (96, 256), (512, 256), (64, 192)):
        for dtype in ('float32', 'float64'):
            for vel in VELOCITIES:
                out.append(dict(tnum=tnum, nt=nt, dtype=dtype, vel=vel, env={}))
    # the knobs, one at a time off the default
    envs = [{'IMPDAR_PS_MFMA': v} for v in ('0', '2', '3', '6', '7')] + [{'IMPDAR_PS_FFT': v} for v in ('strided', 'rocfft')] + \
           [{'IMPDAR_PS_HERMITIAN': '0'}, {'IMPDAR_PS_TEST_EDGE_OVERFLOW': '1'}]
    for env in envs:
        for dtype, vel in (('float32', 'const'), ('float32', 'tab3'), ('float32', 'gradient'), ('float64', 'tab3')):
            out.append(dict(tnum=64, nt=256, dtype=dtype, vel=vel, env=env))
    # the runs kernels of the vector path where their launch order is made
    for dtype in ('float32', 'float64'):
        out.append(dict(tnum=512, nt=256, dtype=dtype, vel='tab3', env={'IMPDAR_PS_MFMA': '0'}))
    return out


def case_id(c):
    return '-'.join(['t%d' % c['tnum'], 'n%d' % c['nt'], c['dtype'], c['vel']] + ['%s=%s' % (k[len('IMPDAR_PS_'):], v) for k, v in sorted(c['env'].items())])


CASES = _cases()
IDS = [case_id(c) for c in CASES]
assert len(CASES) <= 80 and len(set(IDS)) == len(IDS)


def velocity(kind, snum=SNUM, dt=DT):
    """A scalar, or the per-step profile of length snum that getVelocityProfile hands on for a (v, z) table."""
    from oracle import mig_oracle
    tt_us = np.arange(snum) * dt * 1.0e6
    Rp = 1.9e8 * tt_us[-1] * 1e-6 / 2.
    if kind == 'const':
        return 1.69e8
    if kind == 'tab3':
        tab = np.array([[1.69e8, 0.], [1.69e8, 0.2 * Rp], [1.8e8, 0.5 * Rp], [1.9e8, 1.2 * Rp]])
    elif kind == 'tab6':
        tab = np.stack([np.linspace(1.69e8, 2.1e8, 7), np.linspace(0., 1.2 * Rp, 7)], axis=1)
    elif kind == 'many':
        # more than 64 runs of constant velocity in 5 of the 8 sixteen-step tiles (float64 keeps the runs schedule, float32 does not)
        v = np.full(snum, 1.69e8 + 0.4e8)
        v[:72] = 1.69e8 + 0.4e8 * np.arange(72) / 72.
        return np.ascontiguousarray(v)
    else:
        assert kind == 'gradient'
        return np.ascontiguousarray(1.69e8 + 0.5e8 * np.linspace(0., 1., snum))
    return np.ascontiguousarray(mig_oracle.get_velocity_profile(tt_us, tab), dtype=np.float64)


def axes(tnum, nt, dt=DT, dx=DX):
    return 2. * np.pi * np.fft.fftfreq(tnum, d=dx), 2. * np.pi * np.fft.fftfreq(nt, d=dt)


def run(hip, c, snum=SNUM):
    """One impdar_phaseshift_dev call of case c under the knobs in the environment: (metrics, image)."""
    lib, ctx = hip.load(), hip.context()
    kx, ws = axes(c['tnum'], c['nt'])
    tt = np.ascontiguousarray(np.arange(snum) * DT * 1.0e6)
    vel = velocity(c['vel'])
    vm = None if np.ndim(vel) == 0 else vel
    x = np.random.default_rng(c['tnum'] + c['nt']).standard_normal((snum, c['tnum'])).astype(c['dtype'])
    dp = C.POINTER(C.c_double)
    d_in = hip.DeviceArray.from_host(ctx, x)
    d_out = hip.DeviceArray(ctx, d_in.shape, d_in.dtype)
    try:
        hip.check(lib.impdar_phaseshift_dev(ctx, d_in.ptr, hip.dtype_code(x.dtype), snum, c['tnum'], c['nt'], kx.ctypes.data_as(dp),
                                            ws.ctypes.data_as(dp), C.c_double(DT), tt.ctypes.data_as(dp),
                                            C.c_double(float(vel) if vm is None else 0.0), vm.ctypes.data_as(dp) if vm is not None else None,
                                            0 if vm is None else snum, C.c_double(10.), C.c_double(12.), d_out.ptr), 'impdar_phaseshift_dev')
        buf = C.create_string_buffer(1024)
        hip.check(lib.impdar_ctx_last_metrics(ctx, buf, len(buf)), 'metrics')
        img = d_out.to_host()
    finally:
        d_in.free()
        d_out.free()
    return json.loads(buf.value.decode()), img


# ---- the host-only route (csrc/ps_route.h) compiled by itself, as tests/series_scheme.py does with the series planner
ATTEMPTS = ('SERIES', 'NUFFT', 'RUNS', 'MFMA', 'SMOOTH', 'VECTOR')
KERNELS = {'SERIES': ('ps_series_kernel',), 'NUFFT': ('ps_nufft_kernel',), 'RUNS': ('ps_runs_kernel',), 'MFMA': ('ps_mfma_kernel',),
           'SMOOTH': ('ps_smooth32_kernel', 'ps_smooth_kernel'),
           'VECTOR': ('ps_vz32_kernel', 'ps_vz64_kernel', 'ps_kernel (per step)', 'ps_kernel (constant velocity)')}


def probe(tmpdir):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, lib = os.path.join(tmpdir, 'ps_route_probe.cpp'), os.path.join(tmpdir, 'libpsroute.so')
    with open(src, 'w') as f:
        f.write('#define PS_ROUTE_PROBE 1\n#include "ps_route.h"\n')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(root, 'impdar_amd', 'csrc'), src, '-o', lib])
    return C.CDLL(lib)


def route(lib, dtype, snum, kx, ws, vel, dt=DT, k0=0, nk=None, tk_out=False, env=None, rows=False):
    """ps_route (and, with rows, ps_row_order) on one call's inputs under the knobs in env: a dict of what it decided."""
    env = env or {}
    tnum, nt = len(kx), len(ws)
    kx, ws = np.ascontiguousarray(kx, dtype=np.float64), np.ascontiguousarray(ws, dtype=np.float64)
    tt = np.ascontiguousarray(np.arange(snum) * dt * 1.0e6)
    vm = None if np.ndim(vel) == 0 else np.ascontiguousarray(vel, dtype=np.float64)
    ints, dbls, kz = np.zeros(16, dtype=np.int32), np.zeros(2), np.zeros(4, dtype=np.int32)
    w, kinds, alts, rowmap = np.zeros(nt), np.zeros(8, dtype=np.int32), np.zeros(8), np.zeros(tnum, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    fft = {None: 0, 'own': 0, 'strided': 1, 'rocfft': 2}[env.get('IMPDAR_PS_FFT')]
    rc = lib.impdar_ps_route_probe(int(np.dtype(dtype) == np.float64), snum, tnum, nt, kx.ctypes.data_as(dp), ws.ctypes.data_as(dp), C.c_double(dt),
                                   tt.ctypes.data_as(dp), C.c_double(0.0 if vm is not None else float(vel)),
                                   vm.ctypes.data_as(dp) if vm is not None else None, 0 if vm is None else snum, k0, tnum if nk is None else nk,
                                   int(tk_out), fft, int(env.get('IMPDAR_PS_HERMITIAN', '1')), int(env.get('IMPDAR_PS_MFMA', '1')),
                                   int('IMPDAR_PS_TEST_EDGE_OVERFLOW' in env), int(rows), ints.ctypes.data_as(ip), dbls.ctypes.data_as(dp),
                                   kz.ctypes.data_as(ip), w.ctypes.data_as(dp), kinds.ctypes.data_as(ip), alts.ctypes.data_as(dp), rowmap.ctypes.data_as(ip))
    assert rc == 0, rc
    names = ('herm', 'nf', 'fstride', 'nzero', 'use_own', 'use_sched', 'runs', 'long_runs', 'long_runs_metric', 'nufft_first', 'kx_antisym',
             'half_front', 'nattempts', 'nrows', 'vfinite')
    r = {k: int(v) for k, v in zip(names, ints)}
    for k in ('herm', 'use_own', 'use_sched', 'nufft_first', 'kx_antisym', 'half_front', 'vfinite'):
        r[k] = bool(r[k])
    r.update(nufft_ms=float(dbls[0]), runs_ms=float(dbls[1]), k_zero=[int(k) for k in kz[:r['nzero']]], w=w[:r['nf']].copy(),
             attempts=[ATTEMPTS[k] for k in kinds[:r['nattempts']]], alts=[float(a) for a in alts[:r['nattempts']]],
             rowmap=[int(k) for k in rowmap[:r['nrows']]])
    return r
