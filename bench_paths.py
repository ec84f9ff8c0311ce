#!/usr/bin/env python3
"""Secondary measurements (not the driver's bench contract): Stolt f-k at
BASELINE config 2 (4096x4096 float32), phase-shift at config 5 (8192x8192,
constant v and 1-D v(z)), the v(x,z) finite-difference branch (256x512) and the band-pass / re-spacing steps in front of a
migration at config-3 size (4096x10000 float32, resident in HBM, plus the
three-step chain with and without residency), the horizontal filters (hfilt, adaptive
hfilt at windows 10 and 1000), denoise (Wiener and median at several windows) and the horizontal frequency
filters (hbp, lp, hp; float64, as constant_space hands them on) at the same size, resident, the sample-axis steps
(nmo, pretrigger crop, elev_correct), the gains (rangegain, agc), the trace-axis steps (reverse, hcrop, restack) and
winavg_hfilt beside a device-to-device copy of equal bytes, and Stolt at the headline radargram's shape (4096 samples x 10000
traces, no power of two: the library's own mixed-radix row transforms against rocFFT's plans, steady state and the first call
of a fresh process), and ApRES range conversion and stacking at an unattended deployment's size (40 bursts x 20 chirps x 40001
samples, float64), and the time-offset search of kinematic GPS control (10000 traces, 100000 fixes, the reference's five passes),
each through the product path on one MI355X.
Prints one JSON line per path.  Host wall time includes H2D/D2H of the
radargram (the entry points take host buffers).  Each line carries a
``cpu_baseline``: the NumPy oracle (a port of the reference's algorithm in
closed form, far faster than the reference's Python loops) timed on the host
cores of the same box on a bounded sample, with the sample stated.  Kernel
times: run under ``rocprofv3 --kernel-trace --stats`` (profiles/r01_paths_*)."""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, __import__('os').path.dirname(__import__('os').path.abspath(__file__)))


FIELD = (4096, 10000)           # snum x tnum of the "stolt 4096 x 10000" line: the headline radargram's shape


SPECTRA = (4096, 10000)                      # snum, tnum of the "spectra" line


def stolt_first_call_child():
    """`bench_paths.py --stolt-first-call`: a fresh process, as `impproc migrate file.mat` is -- import, context, the FIRST Stolt
    call of the process on a host array under the IMPDAR_STOLT_FFT of the environment, a second call for contrast.  One JSON line."""
    import contextlib
    import ctypes
    import io
    from impdar_amd import _hip, synth
    from impdar_amd.lib.RadarData import RadarData
    snum, tnum = FIELD
    geo = synth.geometry(snum, tnum)
    x = np.random.default_rng(0).standard_normal((snum, tnum)).astype(np.float32)
    _hip.load()
    _hip.context()
    walls = []
    for _ in range(2):
        d = RadarData(None)
        d.data, d.snum, d.tnum = x, snum, tnum
        d.travel_time, d.dist, d.trace_int, d.dt = geo['travel_time'], geo['dist'], geo['trace_int'], geo['dt']
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            d.migrate('stolt', vel=1.68e8, htaper=100, vtaper=1000)
        walls.append((time.perf_counter() - t0) * 1e3)
    buf = ctypes.create_string_buffer(1024)
    _hip.check(_hip.load().impdar_ctx_last_metrics(_hip.context(), buf, len(buf)), 'metrics')
    print(json.dumps({"first_call_ms": walls[0], "second_call_ms": walls[1], "kernel": json.loads(buf.value.decode())['kernel'],
                      "finite": bool(np.isfinite(d.data).all())}))


APRES = (40, 20, 40001, 2, 4000.)           # bnum, cnum, snum, pad factor, max_range of the "apres range" line
APRES_HEADER = dict(bandwidth=2.e8, fc=3.e8, chirp_grad=2. * np.pi * 2.e8, ci=3.e8 / np.sqrt(3.18), lambdac=3.e8 / np.sqrt(3.18) / 3.e8)


def apres_holder(bnum, cnum, snum, seed=5):
    """Raw chirps of the "apres range" line: a DC offset, white noise and three tones with a random phase per chirp."""
    from impdar_amd import apres as apm
    rng = np.random.default_rng(seed)
    dat = apm.Apres()
    dat.bnum, dat.cnum, dat.snum = bnum, cnum, snum
    t = np.arange(snum)
    dat.data = 1.25 + 0.3 * rng.standard_normal((bnum, cnum, snum))
    for f, a in ((0.013, 1.), (0.071, 0.5), (0.19, 0.2)):
        dat.data += a * np.cos(2 * np.pi * f * t + rng.uniform(-np.pi, np.pi, (bnum, cnum, 1)))
    for k, v in APRES_HEADER.items():
        setattr(dat.header, k, v)
    return dat


def apres_first_call_child():
    """`bench_paths.py --apres-first-call`: a fresh process -- import, context, the FIRST range conversion of the process on host
    arrays (2 bursts of the line's shape: rocFFT builds its kernels for the row length at run time, whatever the batch), a second
    for contrast.  One JSON line."""
    from impdar_amd import _hip, apres as apm
    bnum, cnum, snum, p, max_range = APRES
    raw = apres_holder(2, cnum, snum).data
    _hip.load()
    _hip.context()
    walls = []
    for _ in range(2):
        dat = apres_holder(2, cnum, snum)
        dat.data = raw
        t0 = time.perf_counter()
        apm.apres_range(dat, p, max_range)
        walls.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"first_call_ms": walls[0], "second_call_ms": walls[1], "chirps": 2 * cnum,
                      "finite": bool(np.isfinite(dat.data.view(np.float64)).all())}))


def apres_first_call():
    """The first-call child of the "apres range" line against an empty rocFFT kernel database, then one against the database it left."""
    import os
    import subprocess
    import tempfile
    recs = []
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, HOME=tmp, XDG_CACHE_HOME=os.path.join(tmp, 'xdg'), ROCFFT_RTC_CACHE_PATH=os.path.join(tmp, 'rocfft_kernel_cache.db'))
        for _ in range(2):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--apres-first-call'], capture_output=True, text=True,
                                   timeout=240, env=env)
                line = [l for l in r.stdout.splitlines() if l.startswith('{"first_call_ms"')]
                recs.append(json.loads(line[-1]) if line else {"error": (r.stderr or r.stdout)[-300:]})
            except Exception as exc:
                recs.append({"error": "%s: %s" % (type(exc).__name__, exc)})
    return {"cold": recs[0], "warm_cache": recs[1]}


def spectra_first_call_child():
    """`bench_paths.py --spectra-first-call`: a fresh process -- import, context, upload, the FIRST vertical spectrum of the process
    on the resident radargram of the "spectra" line (nothing to compile or plan at an own-transform length), a second for contrast."""
    from impdar_amd import _hip, spectra
    snum, tnum = SPECTRA
    x = np.random.default_rng(11).standard_normal((snum, tnum)).astype(np.float32)
    t0 = time.perf_counter()
    _hip.load()
    d_x = _hip.DeviceArray.from_host(_hip.context(), x)
    up = (time.perf_counter() - t0) * 1e3
    walls = []
    for _ in range(2):
        t0 = time.perf_counter()
        out = spectra.mean_spectrum_dev(d_x, 0)
        walls.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"first_call_ms": walls[0], "second_call_ms": walls[1], "load_context_upload_ms": up,
                      "finite": bool(np.isfinite(out).all())}))


def spectra_first_call():
    import os
    import subprocess
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--spectra-first-call'], capture_output=True, text=True, timeout=240)
        line = [l for l in r.stdout.splitlines() if l.startswith('{"first_call_ms"')]
        return json.loads(line[-1]) if line else {"error": (r.stderr or r.stdout)[-300:]}
    except Exception as exc:
        return {"error": "%s: %s" % (type(exc).__name__, exc)}


def stolt_first_calls(children=3):
    """The first-call children of the "stolt 4096 x 10000" line, started before this process touches the GPU.  Per form
    (the default route: the own mixed-radix transforms; IMPDAR_STOLT_FFT=rocfft: the plans) one process against an empty rocFFT
    kernel database (`cold`), then `children` more against the database it left (`warm_cache`: what every later process pays)."""
    import os
    import subprocess
    import tempfile
    out = {}
    for form, knob in (('mixed', None), ('rocfft', 'rocfft')):
        with tempfile.TemporaryDirectory() as tmp:
            env = dict(os.environ, HOME=tmp, XDG_CACHE_HOME=os.path.join(tmp, 'xdg'), ROCFFT_RTC_CACHE_PATH=os.path.join(tmp, 'rocfft_kernel_cache.db'))
            env.pop('IMPDAR_STOLT_FFT', None)
            if knob:
                env['IMPDAR_STOLT_FFT'] = knob
            recs = []
            for _ in range(1 + children):
                try:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--stolt-first-call'], capture_output=True, text=True,
                                       timeout=240, env=env)
                    line = [l for l in r.stdout.splitlines() if l.startswith('{"first_call_ms"')]
                    recs.append(json.loads(line[-1]) if line else {"error": (r.stderr or r.stdout)[-300:]})
                except Exception as exc:
                    recs.append({"error": "%s: %s" % (type(exc).__name__, exc)})
            warm = [r['first_call_ms'] for r in recs[1:] if 'first_call_ms' in r]
            out[form] = {"cold": recs[0], "warm_cache": recs[1:], "warm_cache_first_call_ms": warm,
                         "warm_cache_median_ms": float(np.median(warm)) if warm else None,
                         "warm_cache_spread_ms": (max(warm) - min(warm)) if warm else None}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--stolt-first-call', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--apres-first-call', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--spectra-first-call', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--stolt', type=int, default=4096)
    ap.add_argument('--phsh', type=int, default=8192)
    ap.add_argument('--chain', type=str, default='4096x10000', help='snum x tnum of the band-pass / re-spacing lines')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--skip', default='')
    ap.add_argument('--no-cpu', action='store_true')
    args = ap.parse_args()
    if args.stolt_first_call:
        return stolt_first_call_child()
    if args.apres_first_call:
        return apres_first_call_child()
    if args.spectra_first_call:
        return spectra_first_call_child()
    field_first = stolt_first_calls() if 'field' not in args.skip else None        # (children first: this process has not opened the GPU yet)
    apres_first = apres_first_call() if 'apres' not in args.skip else None
    spectra_first = spectra_first_call() if 'spectra' not in args.skip else None
    from impdar_amd import _hip, synth
    from impdar_amd.lib.RadarData import RadarData
    from impdar_amd.lib import migrationlib
    import contextlib
    import io
    _hip.load()
    assert _hip.device_count() > 0

    def dat_of(data, geo):
        d = RadarData(None)
        d.data, (d.snum, d.tnum) = data, data.shape
        d.travel_time, d.dist, d.trace_int, d.dt = geo['travel_time'], geo['dist'], geo['trace_int'], geo['dt']
        return d

    def timed(fn, make):
        best = None
        for _ in range(args.reps + 1):           # first call pays rocFFT plan creation
            d = make()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                fn(d)
            el = time.perf_counter() - t0
            best = el if best is None else min(best, el)
        return best, d

    def cpu(fn, label):
        if args.no_cpu:
            return None
        from oracle import mig_oracle                      # the checker, timed as the CPU baseline
        t0 = time.perf_counter()
        fn(mig_oracle)
        el = time.perf_counter() - t0
        return {"seconds": el, "kind": "port", "cores": 1, "sample": label}

    rng = np.random.default_rng(0)
    if 'stolt' not in args.skip:
        n = args.stolt
        geo = synth.geometry(n, n)
        x = rng.standard_normal((n, n)).astype(np.float32)
        el, d = timed(lambda d: migrationlib.migrationStolt(d, htaper=100, vtaper=1000), lambda: dat_of(x.copy(), geo))
        cb = cpu(lambda o: o.stolt(x, geo['dt'], geo['trace_int'], geo['dist'], 1.68e8, 100, 1000),
                 "NumPy oracle, same %dx%d float32 radargram, one process" % (n, n))
        print(json.dumps({"path": "stolt", "config": "%dx%d float32 (BASELINE config 2)" % (n, n),
                          "host_seconds": el, "traces_per_s": n / el, "finite": bool(np.isfinite(d.data).all()),
                          "algorithmic_bytes": 40 * n * n, "reference_seconds_same_size": 100.30,
                          "cpu_baseline": cb}), flush=True)
    if 'field' not in args.skip:
        # Stolt at the headline radargram's shape, resident: the default route (R2C / C2R of 10000 on the mixed-radix kernel, C2C of 4096
        # on the power-of-two one) against IMPDAR_STOLT_FFT=rocfft (what ran at this size before), the calls alternated in this
        # process after warm-up; device time from the HIP events of each call; bytes from config 2's pass model (40 B per sample)
        import ctypes
        import os
        snum, tnum = FIELD
        ctx, lib = _hip.context(), _hip.load()
        geo = synth.geometry(snum, tnum)
        xf = rng.standard_normal((snum, tnum)).astype(np.float32)
        d_x = _hip.DeviceArray.from_host(ctx, xf)
        d_o = _hip.DeviceArray(ctx, (snum, tnum), np.float32)
        kx_keep, p_kx = _hip.as_dp(2. * np.pi * np.fft.fftfreq(tnum, d=float(np.mean(geo['trace_int']))))
        ws_keep, p_ws = _hip.as_dp(2. * np.pi * np.fft.rfftfreq(snum, d=geo['dt']))       # (the arrays stay alive with the pointers)
        buf = ctypes.create_string_buffer(1024)
        saved = os.environ.pop('IMPDAR_STOLT_FFT', None)

        def call(knob):
            if knob:
                os.environ['IMPDAR_STOLT_FFT'] = knob
            else:
                os.environ.pop('IMPDAR_STOLT_FFT', None)
            _hip.check(lib.impdar_stolt_dev(ctx, d_x.ptr, _hip.F32, snum, tnum, p_kx, p_ws, 1.68e8, 100., 1000., d_o.ptr), 'impdar_stolt_dev')
            _hip.check(lib.impdar_ctx_last_metrics(ctx, buf, len(buf)), 'metrics')
            return json.loads(buf.value.decode())

        forms = (('mixed', None), ('rocfft', 'rocfft'))
        images, kernels, ms = {}, {}, {'mixed': [], 'rocfft': []}
        for form, knob in forms:                     # warm-up: code objects, rocFFT's plans, buffers
            for _ in range(2):
                kernels[form] = call(knob)['kernel']
            images[form] = d_o.to_host().astype(np.float64)
        for _ in range(max(10, args.reps)):
            for form, knob in forms:
                ms[form].append(call(knob)['device_ms'])
        if saved is not None:
            os.environ['IMPDAR_STOLT_FFT'] = saved
        d_x.free()
        d_o.free()
        algo = 40 * snum * tnum
        rec = {"path": "stolt 4096 x 10000 float32", "config": "%dx%d float32, resident (snum x tnum: the headline radargram's shape)" % (snum, tnum),
               "algorithmic_bytes": algo, "rel_l2_mixed_vs_rocfft": float(np.linalg.norm(images['mixed'] - images['rocfft']) / np.linalg.norm(images['rocfft'])),
               "finite": bool(np.isfinite(images['mixed']).all()), "first_call": field_first}
        for form, _ in forms:
            t = float(np.median(ms[form]))
            rec[form] = {"kernel": kernels[form], "device_ms": t, "device_ms_spread": max(ms[form]) - min(ms[form]), "device_ms_all": ms[form],
                         "ns_per_sample": t * 1e6 / (snum * tnum),
                         "roofline": {"bound": "hbm", "achieved": algo / t / 1e6, "peak": 8000.0, "unit": "GB/s", "frac": algo / t / 1e6 / 8000.0}}
        rec["power_of_two_record_ns_per_sample"] = 0.27e6 / 4096 ** 2         # config 2: 0.27 ms at 4096 x 4096
        print(json.dumps(rec), flush=True)
    if 'fk' not in args.skip:
        # The f-k fan filter, resident, at config 2 and at the headline radargram's shape, against impdar_stolt_dev at the same
        # size in the same run (the same passes with the stretch in the middle), the calls alternated after warm-up; device
        # times from the HIP events of each call, the fan kernel alone from the pair around it (metrics line: kernel_ms); its
        # bytes are one read and one write of the half spectrum; NumPy fft2 / ifft2 with a ready weight on one core.
        import ctypes
        from impdar_amd import fk as fklib
        ctx, lib = _hip.context(), _hip.load()
        buf = ctypes.create_string_buffer(1024)

        def last():
            _hip.check(lib.impdar_ctx_last_metrics(ctx, buf, len(buf)), 'metrics')
            return json.loads(buf.value.decode())
        for snum, tnum in ((args.stolt, args.stolt), FIELD):
            geo = synth.geometry(snum, tnum)
            xf = rng.standard_normal((snum, tnum)).astype(np.float32)
            d_x = _hip.DeviceArray.from_host(ctx, xf)
            d_o = _hip.DeviceArray(ctx, (snum, tnum), np.float32)
            kx = 2. * np.pi * np.fft.fftfreq(tnum, d=float(np.mean(geo['trace_int'])))
            ws = 2. * np.pi * np.fft.rfftfreq(snum, d=geo['dt'])
            v0 = float(np.mean(geo['trace_int'])) / geo['dt']
            fan = fklib.check_fan((snum, tnum), va_lo=0.8 * v0, va_hi=5.0 * v0, taper=0.2)

            def call(which):
                if which == 'fk':
                    fklib.fan_dev(d_x, kx, ws, fan, out=d_o)
                else:
                    _hip.check(lib.impdar_stolt_dev(ctx, d_x.ptr, _hip.F32, snum, tnum, _hip.as_dp(kx)[1], _hip.as_dp(ws)[1], 1.68e8, 100., 1000.,
                                                    d_o.ptr), 'impdar_stolt_dev')
                return last()
            ms, kms, kernels = {'fk': [], 'stolt': []}, [], {}
            for which in ('fk', 'stolt'):
                for _ in range(2):
                    kernels[which] = call(which)['kernel']
            finite = bool(np.isfinite(d_o.to_host()).all())
            for _ in range(max(10, args.reps)):
                for which in ('fk', 'stolt'):
                    m = call(which)
                    ms[which].append(m['device_ms'])
                    if which == 'fk':
                        kms.append(m['kernel_ms'])
            d_x.free()
            d_o.free()
            on_rows = 'fk_fan_rows' in kernels['fk']
            half = (tnum // 2 + 1) * snum if on_rows else (snum // 2 + 1) * tnum
            fan_bytes = 2 * half * 8
            cb = None
            if not args.no_cpu:
                M = np.ones((snum, tnum), dtype=np.float32)
                t0 = time.perf_counter()
                np.fft.ifft2(M * np.fft.fft2(xf)).real
                cb = {"seconds": time.perf_counter() - t0, "kind": "numpy", "cores": 1, "sample": "numpy.fft fft2 / ifft2, weight ready, one process"}
            t, tk, ts = float(np.median(ms['fk'])), float(np.median(kms)), float(np.median(ms['stolt']))
            print(json.dumps({"path": "fk fan %d x %d float32" % (snum, tnum), "config": "%dx%d float32, resident" % (snum, tnum),
                              "kernel": kernels['fk'], "finite": finite, "device_ms": t, "device_ms_spread": max(ms['fk']) - min(ms['fk']),
                              "device_ms_all": ms['fk'],
                              "fan_kernel": {"ms": tk, "ms_spread": max(kms) - min(kms), "bytes": fan_bytes,
                                             "roofline": {"bound": "hbm", "achieved": fan_bytes / tk / 1e6, "peak": 8000.0, "unit": "GB/s",
                                                          "frac": fan_bytes / tk / 1e6 / 8000.0}},
                              "stolt_same_run": {"kernel": kernels['stolt'], "device_ms": ts, "device_ms_spread": max(ms['stolt']) - min(ms['stolt']),
                                                 "device_ms_all": ms['stolt']},
                              "fk_over_stolt": t / ts, "cpu_baseline": cb}), flush=True)
    if 'decon' not in args.skip:
        # Predictive deconvolution at the headline radargram's shape, resident, out of place: oplen 32 and 256 at gap 8, design
        # 'mean', and the autocorrelogram of 65 lags, the calls alternated after warm-up with a device copy of the radargram's
        # bytes between them as the yardstick of the run; device and stage times from the HIP events of each call (metrics
        # line).  Floors: (|lags| + oplen) fmas per sample against the float64 vector peak, three passes against HBM.
        import ctypes
        from impdar_amd import decon as dclib
        ctx, lib = _hip.context(), _hip.load()
        buf = ctypes.create_string_buffer(1024)
        snum, tnum = FIELD
        xf = rng.standard_normal((snum, tnum)).astype(np.float32)
        d_x = _hip.DeviceArray.from_host(ctx, xf)
        d_o = _hip.DeviceArray(ctx, (snum, tnum), np.float32)
        PEAK_F64, PEAK_HBM = 78.6e12, 8.0e12
        confs = {'oplen32': dict(oplen=32, gap=8, design='each'), 'oplen256': dict(oplen=256, gap=8, design='each'),
                 'mean': dict(oplen=32, gap=8, design='mean'), 'acorr': dict(maxlag=64)}

        def call(name):
            c = confs[name]
            if name == 'acorr':
                dclib.acorr_dev(d_x, dclib.check_acorr((snum, tnum), c['maxlag']))
            else:
                dclib.decon_dev(d_x, dclib.check_decon((snum, tnum), c['oplen'], c['gap'], 0.1, None, c['design']), out=d_o)
            _hip.check(lib.impdar_ctx_last_metrics(ctx, buf, len(buf)), 'metrics')
            return json.loads(buf.value.decode())

        def copy_ms():
            # a device copy that moves the three passes' bytes (1.5 radargrams read, 1.5 written): ten enqueued back to back
            # per sample, the host clock around them and one synchronise, so that the launches hide behind the copies
            n64 = snum * tnum * 3 // 4
            a, b = _hip.DeviceArray(ctx, (n64, 1), np.float64), _hip.DeviceArray(ctx, (n64, 1), np.float64)
            lib.impdar_dev_memset(ctx, a.ptr, 0, n64 * 8)
            out = []
            for _ in range(12):
                lib.impdar_ctx_sync(ctx)
                t0 = time.perf_counter()
                for _ in range(10):
                    lib.impdar_cast_dev(ctx, a.ptr, _hip.F64, b.ptr, _hip.F64, ctypes.c_size_t(n64))
                lib.impdar_ctx_sync(ctx)
                out.append((time.perf_counter() - t0) * 100.0)
            a.free()
            b.free()
            return out[2:]
        ms = {k: [] for k in confs}
        stages = {k: {'acorr_ms': [], 'solve_ms': [], 'apply_ms': []} for k in confs}
        kernels = {}
        for k in confs:
            for _ in range(2):
                kernels[k] = call(k)['kernel']
        finite = bool(np.isfinite(d_o.to_host()).all())
        for _ in range(max(10, args.reps)):
            for k in confs:
                m = call(k)
                ms[k].append(m['device_ms'])
                for s in stages[k]:
                    if s in m:
                        stages[k][s].append(m[s])
        cp = copy_ms()
        d_x.free()
        d_o.free()
        cb = None
        if not args.no_cpu:
            import os
            sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tests'))
            import decon_ref
            t0 = time.perf_counter()
            decon_ref.decon(xf[:, :100], 32, 8, 0.1, None, 'each', 'ref')
            el = time.perf_counter() - t0
            cb = {"seconds": el * tnum / 100.0, "kind": "numpy", "cores": 1,
                  "sample": "NumPy / SciPy restatement (tests/decon_ref.py, ref) of oplen 32, gap 8 on 100 traces: %.3f s, extrapolated by trace count" % el}
        for k, c in confs.items():
            t = float(np.median(ms[k]))
            nl = c['maxlag'] + 1 if k == 'acorr' else len(set(range(c['oplen'])) | set(range(c['gap'], c['gap'] + c['oplen'])))
            fmas = snum * tnum * (nl + (0 if k == 'acorr' else c['oplen']))
            nbytes = snum * tnum * 4 * (1 if k == 'acorr' else 3)
            rec = {"path": "decon 4096 x 10000 float32" if k == 'oplen32' else "decon 4096 x 10000 float32, %s" % k,
                   "config": "%dx%d float32, resident, %s" % (snum, tnum, ', '.join('%s=%s' % kv for kv in sorted(c.items()))),
                   "kernel": kernels[k], "finite": finite, "device_ms": t, "device_ms_spread": max(ms[k]) - min(ms[k]), "device_ms_all": ms[k],
                   "stages": {s: {"ms": float(np.median(v)), "ms_spread": max(v) - min(v)} for s, v in stages[k].items() if v},
                   "fmas": fmas, "fma_floor_ms": 2 * fmas / PEAK_F64 * 1e3, "bytes": nbytes, "hbm_floor_ms": nbytes / 6.3e12 * 1e3,
                   "frac_f64_vector_peak": 2 * fmas / (t * 1e-3) / PEAK_F64, "frac_hbm_peak": nbytes / (t * 1e-3) / PEAK_HBM,
                   "copy_same_run": {"ms": float(np.median(cp)), "ms_spread": max(cp) - min(cp), "bytes": 3 * snum * tnum * 4},
                   "cpu_baseline": cb if k == 'oplen32' else None}
            print(json.dumps(rec), flush=True)
    if 'attr' not in args.skip:
        # Complex-trace attributes at the headline radargram's shape, resident, out of place: envelope, phase, frequency and the
        # frequency smoothed over 9 samples, the calls alternated after warm-up, device times from the HIP events of each call
        # (metrics line).  The compulsory bytes are one read and one write of the radargram; a device copy of the same bytes in
        # the same run is the yardstick.  CPU: scipy.signal.hilbert and NumPy on one core (tests/attr_ref.py, ref) on 100 traces.
        import ctypes
        from impdar_amd import attributes as atlib
        ctx, lib = _hip.context(), _hip.load()
        buf = ctypes.create_string_buffer(1024)
        snum, tnum = FIELD
        dt_s = 2.5e-9
        xf = rng.standard_normal((snum, tnum)).astype(np.float32)
        d_x = _hip.DeviceArray.from_host(ctx, xf)
        d_o = _hip.DeviceArray(ctx, (snum, tnum), np.float32)
        confs = {'envelope': ('envelope', 1), 'phase': ('phase', 1), 'frequency': ('frequency', 1), 'frequency smooth 9': ('frequency', 9)}

        def call(name):
            kind, smooth = confs[name]
            atlib.attr_dev(d_x, atlib.check_attr((snum, tnum), kind, smooth, dt_s), out=d_o)
            _hip.check(lib.impdar_ctx_last_metrics(ctx, buf, len(buf)), 'metrics')
            return json.loads(buf.value.decode())

        def copy_ms():
            # a device copy that reads one radargram and writes one: ten enqueued back to back per sample, the host clock around
            # them and one synchronise, so that the launches hide behind the copies
            n64 = snum * tnum // 2
            a, b = _hip.DeviceArray(ctx, (n64, 1), np.float64), _hip.DeviceArray(ctx, (n64, 1), np.float64)
            lib.impdar_dev_memset(ctx, a.ptr, 0, n64 * 8)
            out = []
            for _ in range(12):
                lib.impdar_ctx_sync(ctx)
                t0 = time.perf_counter()
                for _ in range(10):
                    lib.impdar_cast_dev(ctx, a.ptr, _hip.F64, b.ptr, _hip.F64, ctypes.c_size_t(n64))
                lib.impdar_ctx_sync(ctx)
                out.append((time.perf_counter() - t0) * 100.0)
            a.free()
            b.free()
            return out[2:]
        ms = {k: [] for k in confs}
        kernels, finite = {}, {}
        for k in confs:
            for _ in range(2):
                kernels[k] = call(k)['kernel']
            finite[k] = bool(np.isfinite(d_o.to_host()).all())
        for _ in range(max(10, args.reps)):
            for k in confs:
                ms[k].append(call(k)['device_ms'])
        cp = copy_ms()
        d_x.free()
        d_o.free()
        cbs = {k: None for k in confs}
        if not args.no_cpu:
            import os
            sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tests'))
            import attr_ref
            attr_ref.attr_ref(xf[:64, :2], 'envelope')          # (SciPy's import is not part of the figure)
            for k, (kind, smooth) in confs.items():
                t0 = time.perf_counter()
                attr_ref.attr_ref(xf[:, :100], kind, smooth, dt_s)
                el = time.perf_counter() - t0
                cbs[k] = {"seconds": el * tnum / 100.0, "kind": "numpy", "cores": 1,
                          "sample": "scipy.signal.hilbert + NumPy (tests/attr_ref.py, ref) on 100 traces: %.3f s, extrapolated by trace count" % el}
        nbytes = 2 * snum * tnum * 4
        for k in confs:
            t = float(np.median(ms[k]))
            print(json.dumps({"path": "attributes 4096 x 10000 float32, %s" % k,
                              "config": "%dx%d float32, resident, out of place, kind=%s, smooth=%d" % ((snum, tnum) + confs[k]),
                              "kernel": kernels[k], "finite": finite[k], "device_ms": t, "device_ms_spread": max(ms[k]) - min(ms[k]),
                              "device_ms_all": ms[k], "bytes": nbytes, "frac_hbm_peak": nbytes / (t * 1e-3) / 8.0e12,
                              "copy_same_run": {"ms": float(np.median(cp)), "ms_spread": max(cp) - min(cp), "bytes": nbytes},
                              "cpu_baseline": cbs[k]}), flush=True)
    if 'slope' not in args.skip:
        # Layer slopes at the headline radargram's shape, resident, out of place: the slope field at sigma = (2, 8), dipsmooth with
        # half 4 on a given slope, and the two together (no slope given), the calls alternated after warm-up, device times from the
        # HIP events of each call (metrics line).  Compulsory bytes: the field reads the radargram and writes float64; dipsmooth
        # reads the radargram and the float64 slope and writes the radargram; the two together read and write the radargram.  A
        # device copy of the same bytes in the same run is the yardstick.  CPU: np.gradient, scipy.ndimage.gaussian_filter and
        # NumPy on one core (tests/slope_ref.py, ref) on 100 traces.
        import ctypes
        from impdar_amd import slope as sllib
        ctx, lib = _hip.context(), _hip.load()
        buf = ctypes.create_string_buffer(1024)
        snum, tnum = FIELD
        sigma, half, max_slope = (2.0, 8.0), 4, 4.0
        xf = rng.standard_normal((snum, tnum)).astype(np.float32)
        d_x = _hip.DeviceArray.from_host(ctx, xf)
        d_o = _hip.DeviceArray(ctx, (snum, tnum), np.float32)
        d_p = _hip.DeviceArray(ctx, (snum, tnum), np.float64)
        count = snum * tnum
        confs = {'slope field': 4 * count + 8 * count, 'dipsmooth, slope given': 4 * count + 8 * count + 4 * count,
                 'dipsmooth, own slope': 4 * count + 4 * count}

        def call(name):
            if name == 'slope field':
                sllib.slope_dev(d_x, sllib.check_slope((snum, tnum), 'slope', sigma, max_slope), d_p)
            elif name == 'dipsmooth, slope given':
                sllib.dipsmooth_dev(d_x, sllib.check_dipsmooth((snum, tnum), half, sigma, max_slope, d_p), d_p, out=d_o)
            else:
                sllib.dipsmooth_dev(d_x, sllib.check_dipsmooth((snum, tnum), half, sigma, max_slope), None, out=d_o)
            _hip.check(lib.impdar_ctx_last_metrics(ctx, buf, len(buf)), 'metrics')
            return json.loads(buf.value.decode())

        def copy_ms(nbytes):
            # a device copy that moves `nbytes` in all: ten enqueued back to back per sample, the host clock around them and one
            # synchronise, so that the launches hide behind the copies
            n64 = nbytes // 16
            a, b = _hip.DeviceArray(ctx, (n64, 1), np.float64), _hip.DeviceArray(ctx, (n64, 1), np.float64)
            lib.impdar_dev_memset(ctx, a.ptr, 0, n64 * 8)
            out = []
            for _ in range(12):
                lib.impdar_ctx_sync(ctx)
                t0 = time.perf_counter()
                for _ in range(10):
                    lib.impdar_cast_dev(ctx, a.ptr, _hip.F64, b.ptr, _hip.F64, ctypes.c_size_t(n64))
                lib.impdar_ctx_sync(ctx)
                out.append((time.perf_counter() - t0) * 100.0)
            a.free()
            b.free()
            return out[2:]
        ms = {k: [] for k in confs}
        kernels, finite = {}, {}
        for k in confs:
            for _ in range(2):
                kernels[k] = call(k)['kernel']
            finite[k] = bool(np.isfinite((d_p if k == 'slope field' else d_o).to_host()).all())
        for _ in range(max(10, args.reps)):
            for k in confs:
                ms[k].append(call(k)['device_ms'])
        cps = {k: copy_ms(nb) for k, nb in confs.items()}
        d_x.free()
        d_o.free()
        d_p.free()
        cbs = {k: None for k in confs}
        if not args.no_cpu:
            import os
            sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tests'))
            import slope_ref
            part = xf[:, :100]
            slope_ref.slope_ref(xf[:64, :8], 'slope', sigma)            # (SciPy's import is not part of the figure)
            t0 = time.perf_counter()
            p_cpu = slope_ref.slope_ref(part, 'slope', sigma, max_slope)
            t_field = time.perf_counter() - t0
            t0 = time.perf_counter()
            slope_ref.dipsmooth_ref(part, half, p_cpu)
            t_mean = time.perf_counter() - t0
            for k, el in (('slope field', t_field), ('dipsmooth, slope given', t_mean), ('dipsmooth, own slope', t_field + t_mean)):
                cbs[k] = {"seconds": el * tnum / 100.0, "kind": "numpy", "cores": 1,
                          "sample": "np.gradient + scipy.ndimage.gaussian_filter + NumPy (tests/slope_ref.py, ref) on 100 traces: %.3f s, "
                                    "extrapolated by trace count" % el}
        for k, nbytes in confs.items():
            t, cp = float(np.median(ms[k])), cps[k]
            print(json.dumps({"path": "layer slopes 4096 x 10000 float32, %s" % k,
                              "config": "%dx%d float32, resident, out of place, sigma=(2, 8), half=%d, max_slope=4" % (snum, tnum, half),
                              "kernel": kernels[k], "finite": finite[k], "device_ms": t, "device_ms_spread": max(ms[k]) - min(ms[k]),
                              "device_ms_all": ms[k], "bytes": nbytes, "frac_hbm_peak": nbytes / (t * 1e-3) / 8.0e12,
                              "copy_same_run": {"ms": float(np.median(cp)), "ms_spread": max(cp) - min(cp), "bytes": nbytes},
                              "times_copy": t / float(np.median(cp)), "cpu_baseline": cbs[k]}), flush=True)
    if 'vscan' not in args.skip:
        # The Stolt velocity scan at config 2, resident: 32 velocities in one impdar_stolt_scan_dev call against what a user does
        # without it -- 32 impdar_stolt_dev calls, each image downloaded and reduced to the same three sums per row in NumPy.
        # Device times from the HIP events of each call (the scan's stages from its own events: metrics line); bytes of the back
        # half per velocity on the traces-first route, E = 4: the stretch writes a spectrum (E snum tnum; the shared spectrum it
        # reads is counted as cache traffic, not HBM), the inverse C2C and the transpose read and write it, the C2R reads it and
        # writes the image, the reduction reads the image: 8 E snum tnum.
        import ctypes
        n, nv = args.stolt, 32
        ctx, lib = _hip.context(), _hip.load()
        geo = synth.geometry(n, n)
        xs = np.random.default_rng(0).standard_normal((n, n)).astype(np.float32)
        vels = np.ascontiguousarray(1.68e8 * np.linspace(0.7, 1.3, nv))
        kx_keep, p_kx = _hip.as_dp(2. * np.pi * np.fft.fftfreq(n, d=float(np.mean(geo['trace_int']))))
        ws_keep, p_ws = _hip.as_dp(2. * np.pi * np.fft.rfftfreq(n, d=geo['dt']))
        d_x = _hip.DeviceArray.from_host(ctx, xs)
        d_o = _hip.DeviceArray(ctx, (n, n), np.float32)
        sums = np.empty((nv, n, 3))
        buf = ctypes.create_string_buffer(1024)

        def metrics():
            _hip.check(lib.impdar_ctx_last_metrics(ctx, buf, len(buf)), 'metrics')
            return json.loads(buf.value.decode())

        def scan():
            _hip.check(lib.impdar_stolt_scan_dev(ctx, d_x.ptr, _hip.F32, n, n, p_kx, p_ws, _hip.as_dp(vels)[1], nv, 100., 1000., 0, n, 0,
                                                 _hip.as_dp(sums)[1], -1, None), 'impdar_stolt_scan_dev')
            return metrics()

        def single(v):
            _hip.check(lib.impdar_stolt_dev(ctx, d_x.ptr, _hip.F32, n, n, p_kx, p_ws, float(v), 100., 1000., d_o.ptr), 'impdar_stolt_dev')
            return metrics()['device_ms']

        for _ in range(2):                                   # warm-up: code objects, buffers
            scan()
            single(vels[0])
        recs, singles, loops, loop_dev = [], [], [], []
        for _ in range(max(5, args.reps)):                   # the two forms alternated in this process
            recs.append(scan())
            singles.append(single(vels[nv // 2]))
        for _ in range(2):
            t0 = time.perf_counter()
            dev, by_hand = 0., np.empty((nv, n, 3))
            for b, v in enumerate(vels):
                dev += single(v)
                img = d_o.to_host().astype(np.float64)
                x2 = img * img
                by_hand[b, :, 0], by_hand[b, :, 1], by_hand[b, :, 2] = np.abs(img).sum(axis=1), x2.sum(axis=1), (x2 * x2).sum(axis=1)
            loops.append((time.perf_counter() - t0) * 1e3)
            loop_dev.append(dev)
        t0 = time.perf_counter()
        scan()
        scan_wall = (time.perf_counter() - t0) * 1e3
        d_x.free()
        d_o.free()
        ms = [r['device_ms'] for r in recs]
        t = float(np.median(ms))
        med = lambda key: float(np.median([r[key] for r in recs]))
        back = med('stretch_ms') + med('inverse_ms') + med('focus_ms')
        algo = 8 * 4 * n * n * nv
        print(json.dumps({"path": "vscan %d x %d float32, %d velocities" % (n, n, nv), "config": "%dx%d float32, resident" % (n, n),
                          "kernel": recs[-1]['kernel'], "B": recs[-1]['B'], "nv": nv,
                          "device_ms": t, "device_ms_spread": max(ms) - min(ms), "device_ms_all": ms, "device_ms_per_velocity": t / nv,
                          "host_ms_one_call": scan_wall,
                          "split_ms": {"front": t - back, "stretch": med('stretch_ms'), "inverse_passes": med('inverse_ms'),
                                       "reduction": med('focus_ms')},
                          "single_call_device_ms": float(np.median(singles)), "single_call_device_ms_all": singles,
                          "algorithmic_bytes_back_half": algo,
                          "roofline": {"bound": "hbm", "achieved": algo / back / 1e6, "peak": 8000.0, "unit": "GB/s", "frac": algo / back / 1e6 / 8000.0,
                                       "note": "bytes of the back half (8 E snum tnum per velocity, the shared spectrum's reads not counted) over "
                                               "the time of the stretch, the inverse passes and the reduction"},
                          "by_hand": {"what": "%d impdar_stolt_dev calls, each followed by a download and NumPy sums" % nv,
                                      "host_ms": min(loops), "host_ms_all": loops, "device_ms_of_the_calls": float(np.median(loop_dev))},
                          "max_rel_diff_sums_vs_by_hand": float(np.max(np.abs(sums - by_hand) / by_hand)),
                          "finite": bool(np.isfinite(sums).all())}), flush=True)
    if 'phsh' not in args.skip:
        n = args.phsh
        geo = synth.geometry(n, n)
        x = rng.standard_normal((n, n)).astype(np.float32)
        el, d = timed(lambda d: migrationlib.migrationPhaseShift(d, vel=1.69e8), lambda: dat_of(x.copy(), geo))
        m = min(n, 1024)
        gs = synth.geometry(m, m)
        xs = x[:m, :m].astype(np.float64)
        cb = cpu(lambda o: o.phase_shift(xs, gs['dt'], gs['trace_int'], gs['travel_time'], gs['dist'], 1.69e8),
                 "NumPy oracle on a %dx%d corner (work scales with snum*nt*tnum: x%d for the full size)"
                 % (m, m, (n // m) ** 3))
        print(json.dumps({"path": "phase-shift const v", "config": "%dx%d float32" % (n, n), "host_seconds": el,
                          "traces_per_s": n / el, "finite": bool(np.isfinite(d.data).all()),
                          "rotate_accumulate_steps": float(n) ** 3, "cpu_baseline": cb}), flush=True)
        Rp = 1.9e8 * geo['travel_time'][-1] * 1e-6 / 2.
        tab = np.array([[1.69e8, 0.], [1.69e8, 0.2 * Rp], [1.8e8, 0.5 * Rp], [1.9e8, 1.2 * Rp]])
        el, d = timed(lambda d: migrationlib.migrationPhaseShift(d, vel=tab), lambda: dat_of(x.copy(), geo))
        m = min(n, 512)
        gs = synth.geometry(m, m)
        xs = x[:m, :m].astype(np.float64)
        Rs = 1.9e8 * gs['travel_time'][-1] * 1e-6 / 2.
        tabs = np.array([[1.69e8, 0.], [1.69e8, 0.2 * Rs], [1.8e8, 0.5 * Rs], [1.9e8, 1.2 * Rs]])
        cb = cpu(lambda o: o.phase_shift(xs, gs['dt'], gs['trace_int'], gs['travel_time'], gs['dist'], tabs),
                 "NumPy oracle on a %dx%d radargram (work scales with snum*nt*tnum: x%d for the full size)"
                 % (m, m, (n // m) ** 3))
        print(json.dumps({"path": "phase-shift v(z) Gazdag", "config": "%dx%d float32 (BASELINE config 5)" % (n, n),
                          "host_seconds": el, "traces_per_s": n / el, "finite": bool(np.isfinite(d.data).all()),
                          "rotate_accumulate_steps": float(n) ** 3, "reference_extrapolated_hours": 7.6,
                          "cpu_baseline": cb}), flush=True)
    if 'phsh64' not in args.skip:
        # the same layered table on float64 data (what a float64 .mat file gets): ps_vz64_kernel
        n = args.phsh
        geo = synth.geometry(n, n)
        x64 = rng.standard_normal((n, n))
        Rp = 1.9e8 * geo['travel_time'][-1] * 1e-6 / 2.
        tab = np.array([[1.69e8, 0.], [1.69e8, 0.2 * Rp], [1.8e8, 0.5 * Rp], [1.9e8, 1.2 * Rp]])
        el, d = timed(lambda d: migrationlib.migrationPhaseShift(d, vel=tab), lambda: dat_of(x64.copy(), geo))
        print(json.dumps({"path": "phase-shift v(z) Gazdag, float64 data", "config": "%dx%d float64" % (n, n),
                          "host_seconds": el, "traces_per_s": n / el, "finite": bool(np.isfinite(d.data).all()),
                          "rotate_accumulate_steps": float(n) ** 3}), flush=True)
        del x64, d
    if 'ffd' not in args.skip:
        # v(x,z) table: the Fourier finite-difference branch, a serial chain of snum * nt steps (one workgroup, the
        # row in LDS, for power-of-two trace counts up to 512)
        sn, tn = 256, 512
        geo = synth.geometry(sn, tn, dx=5.0)
        x = rng.standard_normal((sn, tn))
        Rp = 1.9e8 * geo['travel_time'][-1] * 1e-6 / 2.
        xs_ = np.linspace(0., geo['dist'][-1] * 1e3, 5)
        tab3 = np.array([(v + (2e5 * xx / xs_[-1] if z else 0.), z * Rp, xx) for xx in xs_
                         for v, z in ((1.69e8, 0.), (1.72e8, 0.6), (1.8e8, 1.3))])
        el, d = timed(lambda d: migrationlib.migrationPhaseShift(d, vel=tab3, htaper=10, vtaper=10), lambda: dat_of(x.copy(), geo))
        nt_ = 1 << int(np.ceil(np.log2(sn)))
        ms_, mt_ = 32, 64
        gs = synth.geometry(ms_, mt_, dx=5.0)
        Rs = 1.9e8 * gs['travel_time'][-1] * 1e-6 / 2.
        xq = np.linspace(0., gs['dist'][-1] * 1e3, 5)
        tabs3 = np.array([(v + (2e5 * xx / xq[-1] if z else 0.), z * Rs, xx) for xx in xq
                          for v, z in ((1.69e8, 0.), (1.72e8, 0.6), (1.8e8, 1.3))])
        cb = cpu(lambda o: o.phase_shift(x[:ms_, :mt_], gs['dt'], gs['trace_int'], gs['travel_time'], gs['dist'], tabs3, 10, 10),
                 "NumPy oracle on a %dx%d radargram: %d chain steps of %d traces (the full size has %d steps of %d)"
                 % (ms_, mt_, ms_ * ms_, mt_, sn * nt_, tn))
        print(json.dumps({"path": "phase-shift v(x,z) Fourier finite-difference", "config": "%dx%d float64" % (sn, tn),
                          "host_seconds": el, "chain_steps": sn * nt_, "us_per_step": el / (sn * nt_) * 1e6,
                          "finite": bool(np.isfinite(d.data).all()), "cpu_baseline": cb}), flush=True)
    if 'chain' not in args.skip:
        from impdar_amd import preproc
        from impdar_amd.lib.NoInitRadarData import NoInitRadarDataFiltering
        snum, tnum = (int(v) for v in args.chain.split('x'))
        ctx, lib = _hip.context(), _hip.load()
        x = rng.standard_normal((snum, tnum)).astype(np.float32)
        dist = np.hstack(([0.], np.cumsum(0.6 + 0.8 * rng.random(tnum - 1)))) / 1000.

        def dev_ms(fn, reps=10):
            fn()
            lib.impdar_ctx_sync(ctx)
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            lib.impdar_ctx_sync(ctx)
            return (time.perf_counter() - t0) / reps * 1e3

        def sample_cpu(fn, label):
            if args.no_cpu:
                return None
            t0 = time.perf_counter()
            fn()
            return {"seconds": time.perf_counter() - t0, "kind": "reference", "cores": 1, "sample": label}

        d_x = _hip.DeviceArray.from_host(ctx, x)
        spec = preproc.design_filter(1e-8, 2., 10.)
        ms = dev_ms(lambda: preproc.filter_dev(d_x, spec))
        L = snum + 6 * len(spec[1])
        algo = 2 * snum * tnum * 4 + 2 * L * tnum * 8        # read x, write/read the fp64 forward pass, write out
        m = min(tnum, 1000)
        from scipy import signal
        cb = sample_cpu(lambda: signal.filtfilt(spec[1], spec[2], x[:, :m], axis=0).astype(np.float32),
                        "scipy.signal.filtfilt (what the reference calls) on %d of %d traces" % (m, tnum))
        print(json.dumps({"path": "vertical_band_pass butter order 5 (filtfilt), resident", "config": "%dx%d float32" % (snum, tnum),
                          "device_ms": ms, "traces_per_s": tnum / ms * 1e3, "algorithmic_bytes": algo,
                          "roofline": {"bound": "hbm", "achieved": algo / ms / 1e6, "peak": 8000.0, "unit": "GB/s",
                                       "frac": algo / ms / 1e6 / 8000.0,
                                       "note": "serial fp64 recurrence along time, 21 non-fused operations per sample: "
                                               "issue-bound at 625 wavefronts, not HBM-bound"},
                          "cpu_baseline": cb}), flush=True)
        d_x.free()
        d_x = _hip.DeviceArray.from_host(ctx, x)
        plan = preproc.SpacingPlan(dist.copy(), 1.0)

        def lerp():
            o = plan.apply_dev(d_x)
            lib.impdar_ctx_sync(ctx)
            o.free()
        ms = dev_ms(lerp)
        algo = snum * tnum * 4 + snum * plan.n_new * 8
        from scipy.interpolate import interp1d
        ms_rows = min(snum, 256)
        cb = sample_cpu(lambda: interp1d(dist, x[:ms_rows])(plan.new_dists),
                        "scipy.interpolate.interp1d (what the reference calls) on %d of %d sample rows" % (ms_rows, snum))
        print(json.dumps({"path": "constant_space (linear re-spacing), resident", "config": "%dx%d float32 -> %d traces float64" % (snum, tnum, plan.n_new),
                          "device_ms": ms, "traces_per_s": tnum / ms * 1e3, "algorithmic_bytes": algo,
                          "roofline": {"bound": "hbm", "achieved": algo / ms / 1e6, "peak": 8000.0, "unit": "GB/s",
                                       "frac": algo / ms / 1e6 / 8000.0,
                                       "note": "includes the output allocation and the upload of the gather tables"},
                          "cpu_baseline": cb}), flush=True)
        d_x.free()

        # the steps that change the sample axis: nmo (row blend), a trace-wise pretrigger crop and elev_correct
        # (column shift).  Traffic model: input read once + float64 output written once; the yardstick is a plain
        # device-to-device copy that moves the same number of bytes, timed in the same run.
        from impdar_amd import vaxis
        import ctypes

        def copy_ms(nbytes):
            half = (nbytes // 2 + 7) // 8 * 8                 # a copy reads and writes: half the bytes each way
            a = _hip.DeviceArray(ctx, (half // 8, 1), np.float64)
            lib.impdar_dev_memset(ctx, a.ptr, 0, half)

            def call():                                       # what a step's call does around its kernel
                b = _hip.DeviceArray(ctx, (half // 8, 1), np.float64)
                lib.impdar_cast_dev(ctx, a.ptr, _hip.F64, b.ptr, _hip.F64, ctypes.c_size_t(half // 8))
                lib.impdar_ctx_sync(ctx)
                b.free()
            ms = dev_ms(call)
            a.free()
            return ms

        def vline(path, config, fn, algo, cb):
            def call():
                o = fn()
                lib.impdar_ctx_sync(ctx)
                o.free()
            ms = dev_ms(call)
            cms = copy_ms(algo)
            print(json.dumps({"path": path, "config": config, "device_ms": ms, "traces_per_s": tnum / ms * 1e3,
                              "algorithmic_bytes": algo, "copy_same_bytes_ms": cms, "time_over_copy": ms / cms,
                              "roofline": {"bound": "hbm", "achieved": algo / ms / 1e6, "peak": 8000.0, "unit": "GB/s",
                                           "frac": algo / ms / 1e6 / 8000.0,
                                           "note": "time per call (host clock around a device synchronise), not kernel "
                                                   "time: it includes the output allocation and the upload of the "
                                                   "tables; the copy of equal bytes is timed with the same allocation, "
                                                   "synchronise and free.  Bytes: input read once + float64 output "
                                                   "written once"},
                              "cpu_baseline": cb}), flush=True)

        tt = np.arange(snum) * 1e-2
        nmotime = vaxis.nmo_times(tt, 60.)
        new_tt = np.arange(tt.min(), nmotime.max(), 1e-2)
        mt = min(tnum, 200)
        for dtype in (np.float32, np.float64):
            xd = x.astype(dtype)
            d_x = _hip.DeviceArray.from_host(ctx, xd)
            tables = vaxis.RowLerpTables(nmotime, new_tt, vaxis.np_interp_convention(dtype))

            def nmo_loop():
                out = np.empty((len(new_tt), mt))
                for ti in range(mt):                              # the reference's per-trace loop, restated
                    out[:, ti] = interp1d(nmotime, xd[:, ti], kind='linear')(new_tt)
            cb = sample_cpu(nmo_loop, "one scipy interp1d per trace (the reference's loop) on %d of %d traces" % (mt, tnum))
            if cb:
                cb["seconds"] *= tnum / mt
                cb["sample"] += ", scaled to all"
            vline("nmo 60 m (row blend), resident", "%dx%d %s -> %d rows float64" % (snum, tnum, np.dtype(dtype).name, tables.n_out),
                  lambda: vaxis.row_lerp_dev(d_x, tables), snum * tnum * xd.itemsize + tables.n_out * tnum * 8, cb)
            d_x.free()
        d_x = _hip.DeviceArray.from_host(ctx, x)
        trig = (20 + np.cumsum(rng.integers(-1, 2, tnum)).clip(-15, 15)).astype(int)
        n_crop = snum - int(trig.min())

        def crop_loop():
            out = np.full((n_crop, mt), np.nan)
            for i in range(mt):
                out[:snum - trig[i], i] = x[trig[i]:, i]
        cb = sample_cpu(crop_loop, "one slice per trace (the reference's loop) on %d of %d traces" % (mt, tnum))
        if cb:
            cb["seconds"] *= tnum / mt
            cb["sample"] += ", scaled to all"
        vline("crop at a trace-wise pretrigger (column shift), resident", "%dx%d float32 -> %d rows float64" % (snum, tnum, n_crop),
              lambda: vaxis.col_shift_dev(d_x, trig, n_crop), snum * tnum * 4 + n_crop * tnum * 8, cb)
        elev = 1500. + 8. * np.sin(np.arange(tnum) / 300.) + 0.001 * np.arange(tnum)
        top_inds, max_samp, _ = vaxis.elev_shifts(elev, 1e-8, 1.69e8, tt)

        def elev_loop():
            out = np.full((snum + max_samp, mt), np.nan)
            for i in range(mt):
                out[top_inds[i]:top_inds[i] + snum, i] = x[:, i]
        cb = sample_cpu(elev_loop, "one slice per trace (the reference's loop) on %d of %d traces" % (mt, tnum))
        if cb:
            cb["seconds"] *= tnum / mt
            cb["sample"] += ", scaled to all"
        vline("elev_correct (column shift), resident", "%dx%d float32 -> %d rows float64" % (snum, tnum, snum + max_samp),
              lambda: vaxis.col_shift_dev(d_x, -top_inds, snum + max_samp), snum * tnum * 4 + (snum + max_samp) * tnum * 8, cb)
        d_x.free()

        # the gains, the steps that change the trace axis and winavg_hfilt, float32, resident.  The
        # yardstick is again a device-to-device copy of the bytes of the step's traffic model, timed in the same run:
        # with a fresh output array per call for the steps that make one (hcrop, restack), into a standing array for
        # the steps that work in place.
        from impdar_amd import gain as gainlib, hfilt as hfiltlib, taxis

        def copy_inplace_ms(nbytes):
            half = (nbytes // 2 + 7) // 8 * 8
            a = _hip.DeviceArray(ctx, (half // 8, 1), np.float64)
            b = _hip.DeviceArray(ctx, (half // 8, 1), np.float64)
            lib.impdar_dev_memset(ctx, a.ptr, 0, half)

            def call():
                lib.impdar_cast_dev(ctx, a.ptr, _hip.F64, b.ptr, _hip.F64, ctypes.c_size_t(half // 8))
                lib.impdar_ctx_sync(ctx)
            ms = dev_ms(call)
            a.free()
            b.free()
            return ms

        def gline(path, config, fn, algo, model, cb, makes_output):
            def call():
                o = fn()
                lib.impdar_ctx_sync(ctx)
                if makes_output:
                    o.free()
            ms = dev_ms(call)
            cms = copy_ms(algo) if makes_output else copy_inplace_ms(algo)
            print(json.dumps({"path": path, "config": config, "device_ms": ms, "traces_per_s": tnum / ms * 1e3,
                              "algorithmic_bytes": algo, "copy_same_bytes_ms": cms, "time_over_copy": ms / cms,
                              "roofline": {"bound": "hbm", "achieved": algo / ms / 1e6, "peak": 8000.0, "unit": "GB/s",
                                           "frac": algo / ms / 1e6 / 8000.0,
                                           "note": "time per call (host clock around a device synchronise), not kernel "
                                                   "time: it includes the upload of the tables%s; the copy of equal bytes "
                                                   "is timed the same way.  Bytes: %s"
                                                   % (" and the output allocation" if makes_output else "", model)},
                              "cpu_baseline": cb}), flush=True)

        def scaled(cb, factor):
            if cb:
                cb["seconds"] *= factor
                cb["sample"] += ", scaled to all"
            return cb

        E = 4
        cfg = "%dx%d float32" % (snum, tnum)
        tt = np.arange(snum) * 1e-2 + 0.01
        d_x = _hip.DeviceArray.from_host(ctx, x)
        trig = rng.integers(0, 30, tnum).astype(float)
        g_tab, start = gainlib.rangegain_tables(tt, trig, 0.02, snum, tnum)

        def rgain_loop():
            xs = x[:, :mt].copy()
            for i in range(mt):                                   # the reference's per-trace loop, restated
                xs[int(trig[i]) + 1:, i] *= tt[int(trig[i]) + 1:] * 0.02
        cb = scaled(sample_cpu(rgain_loop, "one in-place product per trace (the reference's loop) on %d of %d traces" % (mt, tnum)), tnum / mt)
        gline("rangegain, trace-wise trigger, resident", cfg, lambda: gainlib.rangegain_dev(d_x, g_tab, start), 2 * E * snum * tnum,
              "array read once + written once", cb, False)
        d_x.free()
        d_x = _hip.DeviceArray.from_host(ctx, x)
        ma = min(tnum, 500)

        def agc_loop():
            xs = x[:, :ma].copy()
            maxamp = np.zeros((snum,))
            for i in range(snum):                                 # the reference's per-sample loop, restated
                maxamp[i] = np.max(np.abs(xs[max(0, i - 25):min(i + 25, snum), :]))
            maxamp[maxamp == 0] = 1.0e-6
            xs *= (50 / np.atleast_2d(maxamp).transpose()).astype(xs.dtype)
        cb = scaled(sample_cpu(agc_loop, "one window maximum per sample (the reference's loop) on %d of %d traces" % (ma, tnum)), tnum / ma)
        gline("agc window 50, resident", cfg, lambda: gainlib.agc_dev(d_x, 25, 50), 3 * E * snum * tnum,
              "array read once for the row maxima, then read once + written once", cb, False)
        d_x.free()
        d_x = _hip.DeviceArray.from_host(ctx, x)
        cb = sample_cpu(lambda: np.ascontiguousarray(np.fliplr(x)), "np.fliplr made contiguous, all traces")
        gline("reverse, resident", cfg, lambda: taxis.reverse_dev(d_x), 2 * E * snum * tnum,
              "array read once + written once", cb, False)
        lo_c, hi_c = 1235, tnum
        cb = sample_cpu(lambda: np.ascontiguousarray(x[:, lo_c:hi_c]), "the slice made contiguous, all kept traces")
        gline("hcrop left at trace 1236, resident", "%s -> %d traces" % (cfg, hi_c - lo_c), lambda: taxis.col_range_dev(d_x, lo_c, hi_c),
              2 * E * snum * (hi_c - lo_c), "kept traces read once + written once", cb, True)
        for traces in (5, 101):
            n_new = tnum // traces
            mb = min(n_new, 200)

            def restack_loop():
                stack = np.zeros((snum, mb))
                for j in range(mb):                               # the reference's per-stack loop, restated
                    stack[:, j] = np.mean(x[:, j * traces:(j + 1) * traces], axis=1)
            cb = scaled(sample_cpu(restack_loop, "one mean per stack (the reference's loop) on %d of %d stacks" % (mb, n_new)), n_new / mb)
            gline("restack %d traces, resident" % traces, "%s -> %d traces float64" % (cfg, n_new), lambda: taxis.restack_dev(d_x, traces),
                  E * snum * tnum + 8 * snum * n_new, "input read once + float64 output written once", cb, True)
        scale = hfiltlib.taper(tt)
        for win in (51, 1001):
            lo_w, hi_w = hfiltlib.winavg_windows(tnum, win)

            def winavg_loop():
                out = np.zeros((snum, mt), dtype=x.dtype)
                for i in range(mt):                               # the reference's per-trace loop, restated
                    out[:, i] = x[:, i] - np.mean(x[:, lo_w[i]:hi_w[i]], axis=-1) * scale
            cb = scaled(sample_cpu(winavg_loop, "one window mean per trace (the reference's loop) on %d of %d traces" % (mt, tnum)), tnum / mt)
            gline("winavg_hfilt window %d, resident" % win, cfg, lambda: hfiltlib.winavg_dev(d_x, lo_w, hi_w, scale), 5 * E * snum * tnum,
                  "array read once + means written once, then means and array read once + array written once "
                  "(the fp64 prefix rows are scratch of the workgroup that wrote them)", cb, False)
        d_x.free()

        def chain(resident):
            d = NoInitRadarDataFiltering()
            d.data, (d.snum, d.tnum) = x.copy(), x.shape
            d.dt, d.dist = 1e-8, dist.copy()
            d.travel_time = np.arange(snum) * 1e-2
            for a in ['lat', 'long', 'x_coord', 'y_coord', 'decday', 'pressure', 'elev']:
                setattr(d, a, np.arange(tnum, dtype=float))
            d.trig = np.zeros(tnum)
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                if resident:
                    d.to_device()
                d.vertical_band_pass(2., 10.)
                d.constant_space(1.0)
                d.migrate('stolt', htaper=100, vtaper=1000)
                if resident:
                    d.from_device()
            return time.perf_counter() - t0, d
        for resident in (False, True):
            best = min(chain(resident)[0] for _ in range(args.reps + 1))
            print(json.dumps({"path": "chain vbp -> constant_space -> stolt, %s" % ("resident in HBM" if resident else "host buffers between steps"),
                              "config": "%dx%d float32 in, float64 out" % (snum, tnum), "host_seconds": best,
                              "traces_per_s": tnum / best}), flush=True)

    if 'hfilt' not in args.skip:
        # horizontal filters at the chain's size, resident: device time per call, bytes / time against HBM
        from impdar_amd import hfilt as hf
        snum, tnum = (int(v) for v in args.chain.split('x'))
        ctx, lib = _hip.context(), _hip.load()
        hrng = np.random.default_rng(5)
        x = hrng.standard_normal((snum, tnum)).astype(np.float32)
        x[40:60] += 1000.0
        scale = hf.taper(np.arange(snum) * 1e-2)
        d_x = _hip.DeviceArray.from_host(ctx, x)

        def hdev_ms(fn, reps=10):
            fn()
            lib.impdar_ctx_sync(ctx)
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            lib.impdar_ctx_sync(ctx)
            return (time.perf_counter() - t0) / reps * 1e3

        def hline(path, ms, algo, note, cb):
            print(json.dumps({"path": path, "config": "%dx%d float32" % (snum, tnum), "device_ms": ms,
                              "traces_per_s": tnum / ms * 1e3, "algorithmic_bytes": algo,
                              "roofline": {"bound": "hbm", "achieved": algo / ms / 1e6, "peak": 8000.0, "unit": "GB/s",
                                           "frac": algo / ms / 1e6 / 8000.0, "note": note},
                              "cpu_baseline": cb}), flush=True)

        lo, hi = hf.hfilt_bounds(0, tnum, tnum)
        ms = hdev_ms(lambda: hf.hfilt_dev(d_x, lo, hi, scale))
        cb = None
        if not args.no_cpu:
            t0 = time.perf_counter()
            avg = np.mean(x[:, lo:hi], axis=-1) * scale
            _ = x - np.atleast_2d(avg).transpose().astype(x.dtype)
            cb = {"seconds": time.perf_counter() - t0, "kind": "reference", "cores": 1,
                  "sample": "the reference's NumPy expression on all %d traces" % tnum}
        hline("hfilt (mean trace removed), resident", ms, 3 * snum * tnum * 4,
              "row mean read + row read/write; the second read of a row is expected from cache", cb)
        for window in (10, 1000):
            wlo, whi = hf.ahfilt_windows(tnum, window)
            ms = hdev_ms(lambda: hf.ahfilt_dev(d_x, wlo, whi, scale))
            cb = None
            if not args.no_cpu:
                from scipy.signal import filtfilt
                m = min(tnum, 200)
                t0 = time.perf_counter()
                out = np.zeros((snum, m), dtype=x.dtype)
                for i in range(m):                             # the reference's per-trace loop, restated
                    pk = x[:, wlo[i]:whi[i]].copy()
                    out[:, i] = x[:, i] - filtfilt([.25] * 4, 1, np.mean(pk, axis=-1)) * scale
                cb = {"seconds": (time.perf_counter() - t0) * tnum / m, "kind": "reference", "cores": 1,
                      "sample": "per-trace loop on %d of %d traces, scaled to all" % (m, tnum)}
            # pass 1: read x, write M; pass 2: read M and x, write x (fp64 prefix rows of pass 1 counted apart)
            hline("ahfilt window %d (adaptive), resident" % window, ms, 5 * snum * tnum * 4,
                  "two passes: windowed means from fp64 prefix rows (8 B/element more, largely cache-resident), "
                  "then the 7-tap stencil, taper and subtraction", cb)
        d_x.free()

    if 'denoise' not in args.skip:
        # Wiener and median denoise at the chain's size, float32 resident: device time per call
        from impdar_amd import denoise as dn
        snum, tnum = (int(v) for v in args.chain.split('x'))
        ctx, lib = _hip.context(), _hip.load()
        drng = np.random.default_rng(6)
        x = drng.standard_normal((snum, tnum)).astype(np.float32)
        x[40:60] += 1000.0
        d_x = _hip.DeviceArray.from_host(ctx, x)

        def ddev_ms(fn, reps=5):
            fn().free()
            lib.impdar_ctx_sync(ctx)
            outs = []
            t0 = time.perf_counter()
            for _ in range(reps):
                outs.append(fn())
            lib.impdar_ctx_sync(ctx)
            ms = (time.perf_counter() - t0) / reps * 1e3
            for o in outs:
                o.free()
            return ms

        def dline(path, ms, algo, bound, note, cb):
            rl = {"bound": bound, "note": note}
            if algo:
                rl.update({"achieved": algo / ms / 1e6, "peak": 8000.0, "unit": "GB/s", "frac": algo / ms / 1e6 / 8000.0})
            print(json.dumps({"path": path, "config": "%dx%d float32" % (snum, tnum), "device_ms": ms,
                              "traces_per_s": tnum / ms * 1e3, "algorithmic_bytes": algo, "roofline": rl,
                              "cpu_baseline": cb}), flush=True)

        def cpu_line(fn, what):
            if args.no_cpu:
                return None
            m = min(tnum, 200)
            t0 = time.perf_counter()
            fn(x[:, :m])
            return {"seconds": (time.perf_counter() - t0) * tnum / m, "kind": "reference", "cores": 1,
                    "sample": "%s on %d of %d traces, scaled to all" % (what, m, tnum)}

        from scipy.ndimage import median_filter
        from scipy.signal import wiener
        for win in ((1, 10), (5, 5), (21, 201)):
            ms = ddev_ms(lambda: dn.wiener_dev(d_x, win[0], win[1])[0])
            cb = cpu_line(lambda a: wiener(a, mysize=win), 'scipy.signal.wiener')
            # floor: pass 1 reads x, pass 2 reads x and writes float64 (16 B); the kept statistics add 20 B
            # written and about 40 B read per element
            dline("denoise wiener %dx%d, noise estimated, resident" % win, ms, 16 * snum * tnum, "hbm",
                  "byte floor of both passes (4 + 4 + 8 B/element); the fp64 window statistics kept between the "
                  "passes add about 60 B/element of traffic", cb)
        for win in ((1, 10), (5, 5), (3, 21), (11, 101)):
            small = win[0] * win[1] <= 64
            ms = ddev_ms(lambda: dn.median_dev(d_x, win[0], win[1]), reps=5 if small else 2)
            cb = cpu_line(lambda a: median_filter(a, size=win), 'scipy.ndimage.median_filter')
            dline("denoise median %dx%d, resident" % win, ms, 8 * snum * tnum, "compute",
                  ("register sorting network over the window gathered from an LDS tile" if small else
                   "radix select, 8 passes of N = %d keys per output" % (win[0] * win[1])), cb)
        d_x.free()


    if 'hpass' not in args.skip:
        # horizontal band pass / low pass / high pass at the chain's size, float64 resident (what constant_space
        # hands on): device time per call
        from impdar_amd import hpass as hp
        snum, tnum = (int(v) for v in args.chain.split('x'))
        ctx, lib = _hip.context(), _hip.load()
        prng = np.random.default_rng(7)
        x = prng.standard_normal((snum, tnum))
        d_x = _hip.DeviceArray.from_host(ctx, x)

        def pdev_ms(fn, reps=10):
            fn()
            lib.impdar_ctx_sync(ctx)
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            lib.impdar_ctx_sync(ctx)
            return (time.perf_counter() - t0) / reps * 1e3

        with contextlib.redirect_stdout(io.StringIO()):
            cases = [("horizontal_band_pass 5-100 m (butter 5 band, 11 coefficients)", hp.band_pass_design(5., 100., 1.0, tnum)),
                     ("lowpass 20 m (butter 3, 4 coefficients)", hp.pass_design('low', 20., 1.0, tnum, 1e-8)),
                     ("highpass 20 m (butter 5, 6 coefficients)", hp.pass_design('high', 20., 1.0, tnum, 1e-8))]
        for label, spec in cases:
            ms = pdev_ms(lambda: hp.filtfilt_dev(d_x, spec))
            pad = 3 * len(spec[0])
            steps = 2 * tnum + 3 * pad
            # read x, write and read the fp64 forward pass (tnum + 2 pad per row), write out: about 32 B/element
            algo = snum * (tnum * 8 + 2 * (tnum + 2 * pad) * 8 + tnum * 8)
            cb = None
            if not args.no_cpu:
                from scipy.signal import filtfilt
                m = min(snum, 64)
                t0 = time.perf_counter()
                filtfilt(spec[0], spec[1], x[:m], axis=1)
                cb = {"seconds": (time.perf_counter() - t0) * snum / m, "kind": "reference", "cores": 1,
                      "sample": "scipy.signal.filtfilt (what the reference calls) on %d of %d rows, scaled to all" % (m, snum)}
            print(json.dumps({"path": label + ", resident", "config": "%dx%d float64" % (snum, tnum), "device_ms": ms,
                              "traces_per_s": tnum / ms * 1e3, "algorithmic_bytes": algo, "ns_per_step": ms * 1e6 / steps,
                              "roofline": {"bound": "serial recurrence", "achieved": algo / ms / 1e6, "peak": 8000.0,
                                           "unit": "GB/s", "frac": algo / ms / 1e6 / 8000.0,
                                           "note": "serial fp64 recurrence along each row, %d dependent steps per row; "
                                                   "%d rows: bound by the step latency of one wavefront, not HBM"
                                                   % (steps, snum)},
                              "cpu_baseline": cb}), flush=True)
        d_x.free()

    if 'quadpol' not in args.skip:
        # the quad-pol chain at a field acquisition's size, resident: device time per step and for the three together
        # (host clock around a device synchronise, `reps` calls each: least, median, most), bytes / time against HBM,
        # and a device copy that moves the same number of bytes, timed the same way
        import ctypes
        from impdar_amd import quadpol as qpm
        n, n_thetas, nrange, ntheta = 19000, 100, 476, 11
        ctx, lib = _hip.context(), _hip.load()
        qrng = np.random.default_rng(11)
        amp = 10. ** (-3. * np.arange(n) / n)
        shh = amp * (qrng.standard_normal(n) + 1j * qrng.standard_normal(n))
        svv = shh * np.exp(0.03j * np.arange(n)) + 0.3 * amp * (qrng.standard_normal(n) + 1j * qrng.standard_normal(n))
        shv = 0.05 * amp * (qrng.standard_normal(n) + 1j * qrng.standard_normal(n) + (2. + 2.j))
        svh = shv + 0.01 * amp * (qrng.standard_normal(n) + 1j * qrng.standard_normal(n))
        thetas = np.linspace(0, np.pi, n_thetas)
        factors = (np.cos(thetas)**2., np.sin(thetas) * np.cos(thetas), np.sin(thetas)**2)
        grad = qpm.gradient_coefficients(np.arange(n) * 0.21)
        d_vec = [_hip.DeviceArray.from_host(ctx, v) for v in (shh, shv, svh, svv)]

        def spread(fn, reps=10):
            fn()
            ms = []
            for _ in range(reps):
                lib.impdar_ctx_sync(ctx)
                t0 = time.perf_counter()
                fn()
                lib.impdar_ctx_sync(ctx)
                ms.append((time.perf_counter() - t0) * 1e3)
            ms.sort()
            return {"min": ms[0], "median": ms[len(ms) // 2], "max": ms[-1]}

        def free(ds):
            for d in ds:
                d.free()

        def qp_chain():
            im = qpm.rotate_dev(d_vec, *factors)
            c = qpm.coherence_dev(im[0], im[3], nrange, ntheta)
            g = qpm.phase_gradient_dev(c, grad)
            lib.impdar_ctx_sync(ctx)
            free(list(im) + [c, g])

        def qp_copy(nbytes):
            half = (nbytes // 2 + 7) // 8 * 8
            a = _hip.DeviceArray(ctx, (half // 8, 1), np.float64)
            lib.impdar_dev_memset(ctx, a.ptr, 0, half)

            def call():
                b = _hip.DeviceArray(ctx, (half // 8, 1), np.float64)
                lib.impdar_cast_dev(ctx, a.ptr, _hip.F64, b.ptr, _hip.F64, ctypes.c_size_t(half // 8))
                lib.impdar_ctx_sync(ctx)
                b.free()
            ms = spread(call)
            a.free()
            return ms
        images = qpm.rotate_dev(d_vec, *factors)
        d_c = qpm.coherence_dev(images[0], images[3], nrange, ntheta)
        el = n * n_thetas
        bytes_of = {"rotation": 4 * n * 16 + 4 * el * 16, "coherence": 3 * el * 16, "phase_gradient": el * 16 + el * 8}
        def step(make):
            def call():
                o = make()
                lib.impdar_ctx_sync(ctx)
                free(o if isinstance(o, tuple) else [o])
            return spread(call)
        steps = {"rotation": step(lambda: qpm.rotate_dev(d_vec, *factors)),
                 "coherence": step(lambda: qpm.coherence_dev(images[0], images[3], nrange, ntheta)),
                 "phase_gradient": step(lambda: qpm.phase_gradient_dev(d_c, grad))}
        algo = sum(bytes_of.values())
        whole = spread(qp_chain)
        cms = qp_copy(algo)
        print(json.dumps({"path": "quadpol chain %d x %d complex128" % (n, n_thetas),
                          "config": "nrange %d, ntheta %d, resident" % (nrange, ntheta),
                          "device_ms": whole["median"], "device_ms_spread": whole,
                          "steps_ms": steps, "algorithmic_bytes": algo, "algorithmic_bytes_per_step": bytes_of,
                          "hbm_frac_per_step": {k: bytes_of[k] / steps[k]["median"] / 1e6 / 8000.0 for k in steps},
                          "copy_same_bytes_ms": cms, "time_over_copy": whole["median"] / cms["median"],
                          "roofline": {"bound": "hbm", "achieved": algo / whole["median"] / 1e6, "peak": 8000.0, "unit": "GB/s",
                                       "frac": algo / whole["median"] / 1e6 / 8000.0,
                                       "note": "time per call (host clock around a device synchronise), with the output "
                                               "allocations and table uploads; the copy is timed with the same allocation, "
                                               "synchronise and free.  Bytes: every input read once, every product written "
                                               "once; the coherence's window sums (32 B per element written and re-read "
                                               "about 2 nrange / bk + bk times from cache) are not counted"}}), flush=True)
        # the reference's full flow -- rotation, cpe axis, coherence, the coherence along the axis -- timed the same way;
        # find_cpe's three stages from the library's own events
        spec = qpm.lowpass_spec(0.1 * 0.5 / 1.0e-8, 1. / 1.0e-8)
        i0, i1 = int(np.argmin(abs(thetas - np.pi / 4.))), int(np.argmin(abs(thetas - 3. * np.pi / 4.)))
        cpe_stages = []

        def cpe_call():
            d = qpm.find_cpe_dev(images[1], spec, i0, i1)
            lib.impdar_ctx_sync(ctx)
            cpe_stages.append(qpm.find_cpe_last_ms(ctx))
            d.free()

        def qp_flow():
            im = qpm.rotate_dev(d_vec, *factors)
            idx = qpm.find_cpe_dev(im[1], spec, i0, i1)
            c = qpm.coherence_dev(im[0], im[3], nrange, ntheta)
            cc = qpm.cpe_gather_dev(c, idx)
            lib.impdar_ctx_sync(ctx)
            free(list(im) + [idx, c, cc])
        cpe_ms = spread(cpe_call)
        st = np.array(cpe_stages[1:])
        cpe_stage_ms = {k: {"min": float(st[:, i].min()), "median": float(np.median(st[:, i])), "max": float(st[:, i].max())}
                        for i, k in enumerate(("anomaly", "filter", "argmin"))}
        # anomaly: HV read, both planes written; filter: the planes read and written; argmin: the window read, an int32 written
        cpe_bytes = {"anomaly": 2 * el * 16, "filter": 2 * el * 16, "argmin": n * (i1 - i0) * 16 + n * 4}
        flow_bytes = {"rotation": bytes_of["rotation"], "find_cpe": sum(cpe_bytes.values()), "coherence": bytes_of["coherence"],
                      "gather": n * (16 + 4 + 16)}
        falgo = sum(flow_bytes.values())
        flow = spread(qp_flow)
        fcms = qp_copy(falgo)
        print(json.dumps({"path": "quadpol flow %d x %d complex128" % (n, n_thetas),
                          "config": "nrange %d, ntheta %d, Wn 0.1 of Nyquist, window [%d, %d), resident" % (nrange, ntheta, i0, i1),
                          "device_ms": flow["median"], "device_ms_spread": flow,
                          "find_cpe_ms": cpe_ms, "find_cpe_stages_ms": cpe_stage_ms, "find_cpe_bytes_per_stage": cpe_bytes,
                          "hbm_frac_per_stage": {k: cpe_bytes[k] / cpe_stage_ms[k]["median"] / 1e6 / 8000.0 for k in cpe_bytes},
                          "algorithmic_bytes": falgo, "algorithmic_bytes_per_step": flow_bytes,
                          "copy_same_bytes_ms": fcms, "time_over_copy": flow["median"] / fcms["median"],
                          "roofline": {"bound": "hbm", "achieved": falgo / flow["median"] / 1e6, "peak": 8000.0, "unit": "GB/s",
                                       "frac": falgo / flow["median"] / 1e6 / 8000.0,
                                       "note": "time per call (host clock around a device synchronise), with the output "
                                               "allocations and table uploads; the stages of find_cpe are device time between "
                                               "the library's events.  The filter is a serial fp64 recurrence along range over "
                                               "2 n_thetas columns: bound by step latency, not HBM"}}), flush=True)
        free(d_vec + list(images) + [d_c])

    if 'apres' not in args.skip:
        # ApRES range conversion and stacking at an unattended deployment's size, resident: device time per call (host clock around
        # a device synchronise, `reps` calls each: least, median, most), the conversion's three stages from the library's own
        # events, bytes / time against HBM, a device copy of the same number of bytes timed the same way, the chain through host
        # arrays, the first call of a fresh process, and the reference's per-chirp NumPy loop on one core
        import ctypes
        from impdar_amd import apres as apm
        bnum, cnum, snum, p, max_range = APRES
        rows, N = bnum * cnum, p * snum
        ctx, lib = _hip.context(), _hip.load()
        dat = apres_holder(bnum, cnum, snum)
        t = apm.range_tables(dat, p, max_range)
        raw = apm.raw_rows(dat)
        n, nf, nh = t.n, t.nf, N // 2 + 1
        d_raw = _hip.DeviceArray.from_host(ctx, raw)

        def aspread(fn, reps=5):
            fn()
            ms = []
            for _ in range(reps):
                lib.impdar_ctx_sync(ctx)
                t0 = time.perf_counter()
                fn()
                lib.impdar_ctx_sync(ctx)
                ms.append((time.perf_counter() - t0) * 1e3)
            ms.sort()
            return {"min": ms[0], "median": ms[len(ms) // 2], "max": ms[-1]}

        stages = []

        def range_call():
            out = apm.range_dev(d_raw, t)
            lib.impdar_ctx_sync(ctx)
            stages.append(apm.range_last_ms(ctx))
            for d in out:
                d.free()

        range_ms = aspread(range_call)
        st = np.array(stages[1:])
        stage_ms = {k: {"min": float(st[:, i].min()), "median": float(np.median(st[:, i])), "max": float(st[:, i].max())}
                    for i, k in enumerate(("prep", "transform", "post"))}
        products = apm.range_dev(d_raw, t)

        def stack_call():
            d = apm.stack_dev(products[1], 1, rows)
            lib.impdar_ctx_sync(ctx)
            d.free()

        stack_ms = aspread(stack_call)
        for d in products:
            d.free()
        bytes_of = {"prep": rows * snum * 8 + rows * N * 8, "transform": rows * N * 8 + rows * nh * 16,
                    "post": rows * nf * 16 + 2 * rows * n * 16 + rows * nf * 8, "stack": rows * n * 16 + n * 16}
        range_bytes = bytes_of["prep"] + bytes_of["transform"] + bytes_of["post"]

        def ap_copy(nbytes):
            half = (nbytes // 2 + 7) // 8 * 8
            a = _hip.DeviceArray(ctx, (half // 8, 1), np.float64)
            lib.impdar_dev_memset(ctx, a.ptr, 0, half)

            def call():
                b = _hip.DeviceArray(ctx, (half // 8, 1), np.float64)
                lib.impdar_cast_dev(ctx, a.ptr, _hip.F64, b.ptr, _hip.F64, ctypes.c_size_t(half // 8))
                lib.impdar_ctx_sync(ctx)
                b.free()
            ms = aspread(call)
            a.free()
            return ms
        copy_range, copy_stack = ap_copy(range_bytes), ap_copy(bytes_of["stack"])
        d_raw.free()

        def chain_call():
            c = apres_holder(1, 1, 2)
            c.bnum, c.cnum, c.snum, c.data = bnum, cnum, snum, dat.data
            apm.chain(c, p, max_range)
        t0 = time.perf_counter()
        chain_call()
        chain_first = (time.perf_counter() - t0) * 1e3
        chain_ms = []
        for _ in range(2):
            t0 = time.perf_counter()
            chain_call()
            chain_ms.append((time.perf_counter() - t0) * 1e3)

        cb = None
        if not args.no_cpu:
            sample = 20
            t0 = time.perf_counter()
            spec = np.zeros((sample, nf)).astype(np.cdouble)
            cor = np.zeros((sample, nf)).astype(np.cdouble)
            for ic in range(sample):                         # the reference's loop body, chirp by chirp
                chirp = raw[ic].copy()
                chirp = chirp - np.mean(chirp)
                chirp *= t.win
                f = (np.sqrt(2. * p) / len(chirp)) * np.fft.fft(chirp, N)
                f /= np.sqrt(np.mean(t.win**2.))
                spec[ic] = f[:nf]
                cor[ic] = np.exp(-1j * t.phiref) * f[:nf]
            el = time.perf_counter() - t0
            cb = {"what": "the reference's per-chirp NumPy loop (de-mean, window, numpy.fft.fft of the padded chirp, scale, reference "
                          "phasor) on one core", "sample": "%d of %d chirps, scaled" % (sample, rows), "ms": el * 1e3 * rows / sample}
        hbm = lambda b, ms: b / ms / 1e6 / 8000.0                                   # noqa: E731
        print(json.dumps({"path": "apres range %d x %d x %d float64, pad %d, %g m" % (bnum, cnum, snum, p, max_range),
                          "config": "N %d, %d of %d bins kept, blackman, resident" % (N, n, nf),
                          "device_ms": range_ms["median"], "device_ms_spread": range_ms, "stages_ms": stage_ms,
                          "stack_ms": stack_ms, "algorithmic_bytes": range_bytes, "algorithmic_bytes_per_stage": bytes_of,
                          "hbm_frac_per_stage": dict({k: hbm(bytes_of[k], stage_ms[k]["median"]) for k in stage_ms},
                                                     stack=hbm(bytes_of["stack"], stack_ms["median"])),
                          "copy_same_bytes_ms": {"range": copy_range, "stack": copy_stack},
                          "time_over_copy": {"range": range_ms["median"] / copy_range["median"],
                                             "stack": stack_ms["median"] / copy_stack["median"]},
                          "chain_host_ms": {"first": chain_first, "later": chain_ms,
                                            "moves": "%d MB up, %d MB down" % (raw.nbytes >> 20, (2 * rows * n * 16 + rows * nf * 8 + n * 16) >> 20)},
                          "first_call": apres_first,
                          "roofline": {"bound": "hbm", "achieved": range_bytes / range_ms["median"] / 1e6, "peak": 8000.0, "unit": "GB/s",
                                       "frac": hbm(range_bytes, range_ms["median"]),
                                       "note": "time per call (host clock around a device synchronise), with the output allocations and "
                                               "table upload; stages from events on the stream, summed over the chunks.  Bytes: prep reads "
                                               "the chirps and writes the padded rows, the transform reads those and writes N / 2 + 1 bins "
                                               "(its own passes over a row of this length are not counted), post reads nf bins and writes "
                                               "spec, data (n bins) and Rfine (nf bins); stacking reads data once"},
                          "cpu_baseline": cb}), flush=True)

        # ApRES load at the same size: an instrument's uint16 counts (synthesised in memory) to resident float64 chirps.  Per call
        # with spreads: today's route (the reference's host decode, then the float64 upload), the counts route (counts upload in
        # pieces + device decode), the decode kernel alone (one piece, the context's kernel timer) against HBM at 10 B per sample
        # and against a device copy of the same bytes; then .DAT files on a tmpfs path to the stacked profile on both routes
        import os
        import shutil
        import tempfile
        from impdar_amd.lib.ApresData import load_apres as la
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tests'))
        import apres_io_ref as io_ref
        total = rows * snum
        counts = np.random.default_rng(11).integers(0, 65536, size=total, dtype=np.uint16)
        d_volts = _hip.DeviceArray(ctx, (rows, snum), np.float64)
        cptr = counts.ctypes.data_as(ctypes.c_void_p)

        def host_route():
            d = _hip.DeviceArray.from_host(ctx, (counts.astype(float) * 2.5 / 2**16.).reshape(rows, snum))
            d.free()

        def counts_route():
            _hip.check(lib.impdar_apres_decode_dev(ctx, cptr, 0, total, 1., d_volts.ptr), 'impdar_apres_decode_dev')

        host_ms, counts_ms = aspread(host_route), aspread(counts_route)
        kernel = []
        for _ in range(6):                                   # the counts in one piece: the kernel stands alone between its events
            _hip.check(lib.impdar_apres_decode_pieces_dev(ctx, cptr, 0, total, 1., d_volts.ptr, total), 'impdar_apres_decode_pieces_dev')
            ms = ctypes.c_float()
            _hip.check(lib.impdar_ctx_last_kernel_ms(ctx, ctypes.byref(ms)), 'impdar_ctx_last_kernel_ms')
            kernel.append(ms.value)
        kernel = sorted(kernel[1:])
        kernel_ms = {"min": kernel[0], "median": kernel[len(kernel) // 2], "max": kernel[-1]}
        d_volts.free()
        copy_decode = ap_copy(total * 10)
        folder = tempfile.mkdtemp(dir='/dev/shm' if os.path.isdir('/dev/shm') else None)
        try:
            per = cnum * snum
            fns = [io_ref.write_dat(os.path.join(folder, 'b%02d.DAT' % b),
                                    [io_ref.burst_bytes(counts[b * per:(b + 1) * per], nsub=cnum, natt=1, snum=snum)]) for b in range(bnum)]

            def flow(drop_counts):
                t0 = time.perf_counter()
                acq = la.load_apres(fns)
                if drop_counts:
                    acq.data = acq.data                    # the float64 chirps on the host, as the reference holds them
                apm.chain(acq, p, max_range)
                return (time.perf_counter() - t0) * 1e3
            flow(False)
            flow_ms = {"counts": sorted(flow(False) for _ in range(3)), "float64": sorted(flow(True) for _ in range(3))}
        finally:
            shutil.rmtree(folder)
        print(json.dumps({"path": "apres load %d x %d x %d uint16" % (bnum, cnum, snum),
                          "config": "%d MB of counts to %d MB of resident float64 chirps" % ((total * 2) >> 20, (total * 8) >> 20),
                          "host_decode_upload_ms": host_ms, "counts_upload_device_decode_ms": counts_ms,
                          "device_ms": kernel_ms["median"], "device_ms_spread": kernel_ms,
                          "algorithmic_bytes": total * 10, "copy_same_bytes_ms": copy_decode,
                          "kernel_events_over_copy_host_clock": kernel_ms["median"] / copy_decode["median"],
                          "files_to_stacked_profile_ms": flow_ms,
                          "roofline": {"bound": "hbm", "achieved": total * 10 / kernel_ms["median"] / 1e6, "peak": 8000.0, "unit": "GB/s",
                                       "frac": hbm(total * 10, kernel_ms["median"]),
                                       "note": "the kernel alone from events on the stream, the counts uploaded in one piece; the copy of equal bytes on the "
                                               "host clock around its allocation, launch and synchronise, as on the other lines: not like for like, the "
                                               "quotient flatters the kernel; the two "
                                               "routes per call on the host clock around a device synchronise, the counts route in "
                                               "8 MiB pieces through two pinned slots; files on a tmpfs path where there is one"}}),
              flush=True)

    if 'autopick' not in args.skip:
        # layer picking on the resident radargram: 16 seeds walked over every trace (a chain of dependent steps per
        # seed and direction), then the two trace-parallel readers, the guided pick and the continuity index
        import ctypes
        from impdar_amd import picking
        snum, tnum = (int(v) for v in args.chain.split('x'))
        ctx, lib = _hip.context(), _hip.load()
        nseeds, dt = 16, 1.0e-8
        plength, FWW, scst, pol = 49, 17, 16, 1                        # PickParameters.freq_update(4) at this dt
        rows = np.arange(snum, dtype=np.float32)[:, None]
        cols = np.arange(tnum, dtype=np.float32)[None, :]
        z0 = (np.arange(nseeds) + 1) * (snum // (nseeds + 1))
        x = (0.05 * np.random.default_rng(9).standard_normal((snum, tnum))).astype(np.float32)
        for z in z0:                                                   # one Ricker-shaped layer per seed, gently dipping
            u = (rows - (z + 0.002 * cols + 2. * np.sin(cols / 9.))) / 6.
            x += (1. - 2. * u ** 2) * np.exp(-u ** 2)
        d_x = _hip.DeviceArray.from_host(ctx, x)
        t0 = tnum // 2
        seeds = (z0.tolist(), [t0] * nseeds)

        def spread(fn, reps=7):
            fn()
            ts = []
            for _ in range(reps):
                a = time.perf_counter()
                fn()
                lib.impdar_ctx_sync(ctx)
                ts.append((time.perf_counter() - a) * 1e3)
            return {"median": float(np.median(ts)), "min": min(ts), "max": max(ts), "reps": reps}

        def pcopy_ms(nbytes):
            half = (nbytes // 2 + 7) // 8 * 8                          # a copy reads and writes: half the bytes each way
            a = _hip.DeviceArray(ctx, (half // 8, 1), np.float64)
            b = _hip.DeviceArray(ctx, (half // 8, 1), np.float64)
            lib.impdar_dev_memset(ctx, a.ptr, 0, half)
            ms = spread(lambda: lib.impdar_cast_dev(ctx, a.ptr, _hip.F64, b.ptr, _hip.F64, ctypes.c_size_t(half // 8)))
            a.free()
            b.free()
            return ms

        auto_ms = spread(lambda: picking.auto_pick_dev(d_x, *seeds, plength, FWW, scst, pol))
        steps = max(t0 + 1, tnum - t0)                                 # the longer of a seed's two walks
        step_ns = auto_ms["median"] * 1e6 / steps
        mid = picking.midpoints(tnum, int(z0[3]), int(z0[3]) + 20)
        guided_ms = spread(lambda: picking.pick_dev(d_x, 0, mid, plength, FWW, scst, pol))
        guided_bytes = plength * tnum * 4
        s = np.zeros(tnum, dtype=np.int32)
        b = np.full(tnum, snum, dtype=np.int32)
        cont_ms = spread(lambda: picking.continuity_dev(d_x, s, b, None))
        cont_bytes = snum * tnum * 4
        copies = {"guided": pcopy_ms(guided_bytes), "continuity": pcopy_ms(cont_bytes)}
        cb = None
        if not args.no_cpu:
            m = min(tnum, 2000)

            def np_packet(trace, midpoint):                            # the reference's packet_pick, restated
                top = int(midpoint - plength / 2.)
                pk = trace[top:int(midpoint + plength / 2.)]
                c = int(np.argmax(pk[scst + 1:scst + FWW + 1] * pol) + scst + 1)
                t = int(np.argmin(pk[c - FWW:c] * pol)) + c - FWW if c > FWW else (0 if c <= 1 else int(np.argmin(pk[:c] * pol)))
                bo = int(np.argmin(pk[c + 1:c + FWW + 1] * pol)) + c + 1 if c + FWW < plength else plength - 1
                return t + top, c + top, bo + top, np.sum(pk[t:bo + 1] ** 2.) / (bo - t + 1)
            a = time.perf_counter()
            midpoint = int(z0[0])
            for j in range(m):                                         # one seed, one direction
                t, _, bo, _ = np_packet(x[:, j], midpoint)
                midpoint = (t + bo) // 2
            el = time.perf_counter() - a
            cb = {"seconds": el * tnum / m * nseeds, "kind": "reference", "cores": 1,
                  "sample": "the reference's per-trace loop restated in NumPy, one seed over %d of %d traces, scaled to %d seeds "
                            "over all" % (m, tnum, nseeds), "us_per_trace_and_seed": el / m * 1e6}
        d_x.free()
        print(json.dumps({"path": "autopick %d x %d float32, %d seeds" % (snum, tnum, nseeds),
                          "config": "plength %d, FWW %d, scst %d; every seed starts at trace %d: two walks of %d and %d steps, one "
                                    "wave each" % (plength, FWW, scst, t0, t0 + 1, tnum - t0),
                          "device_ms": auto_ms["median"], "device_ms_spread": auto_ms,
                          "trace_step": {"ns": step_ns, "cycles_at_2.4GHz": step_ns * 2.4, "hbm_miss_cycles_guide": 900,
                                         "note": "time per call over the steps of the longer walk: an upper bound on a step, "
                                                 "it holds the seed upload, the launch and the download of the picks"},
                          "guided_pick_ms": guided_ms, "continuity_ms": cont_ms,
                          "algorithmic_bytes": {"guided": guided_bytes, "continuity": cont_bytes},
                          "hbm_frac": {"guided": guided_bytes / guided_ms["median"] / 1e6 / 8000.0,
                                       "continuity": cont_bytes / cont_ms["median"] / 1e6 / 8000.0},
                          "copy_same_bytes_ms": copies,
                          "time_over_copy": {"guided": guided_ms["median"] / copies["guided"]["median"],
                                             "continuity": cont_ms["median"] / copies["continuity"]["median"]},
                          "roofline": {"bound": "latency", "note": "time per call (host clock around a device synchronise), with the "
                                       "table uploads and the download of the result.  The chain is bound by the latency of a "
                                       "step, not by bytes; the guided pick reads plength rows of every trace, the continuity "
                                       "index every sample once"},
                          "cpu_baseline": cb}), flush=True)

    if 'spectra' not in args.skip:
        # spectra of the resident radargram: the mean spectrum along the samples (ft: transpose + 10000 rows of 4096), along the
        # traces (hft: 4096 rows of 10000 = 2^4 5^4, the own mixed-radix transform) and the periodogram of every trace
        import ctypes
        import scipy.signal
        from impdar_amd import spectra
        snum, tnum = SPECTRA
        ctx, lib = _hip.context(), _hip.load()
        fs = 1.0e8
        x = np.random.default_rng(11).standard_normal((snum, tnum)).astype(np.float32)
        d_x = _hip.DeviceArray.from_host(ctx, x)

        def spread(fn, reps=7):
            fn()
            ts = []
            for _ in range(reps):
                a = time.perf_counter()
                fn()
                lib.impdar_ctx_sync(ctx)
                ts.append((time.perf_counter() - a) * 1e3)
            return {"median": float(np.median(ts)), "min": min(ts), "max": max(ts), "reps": reps}

        def pcopy_ms(nbytes):
            half = (nbytes // 2 + 7) // 8 * 8                          # a copy reads and writes: half the bytes each way
            a = _hip.DeviceArray(ctx, (half // 8, 1), np.float64)
            b = _hip.DeviceArray(ctx, (half // 8, 1), np.float64)
            lib.impdar_dev_memset(ctx, a.ptr, 0, half)
            ms = spread(lambda: lib.impdar_cast_dev(ctx, a.ptr, _hip.F64, b.ptr, _hip.F64, ctypes.c_size_t(half // 8)))
            a.free()
            b.free()
            return ms

        def pgram():
            spectra.periodogram_dev(d_x, fs, window='hann', scaling='spectrum', resident=True)[1].free()
        ms = {"ft": spread(lambda: spectra.mean_spectrum_dev(d_x, 0)), "hft": spread(lambda: spectra.mean_spectrum_dev(d_x, 1)),
              "periodogram": spread(pgram)}
        nbytes = {"ft": snum * tnum * 4, "hft": snum * tnum * 4, "periodogram": snum * tnum * 4 + (snum // 2 + 1) * tnum * 8}
        copies = {"ft": pcopy_ms(nbytes["ft"]), "periodogram": pcopy_ms(nbytes["periodogram"])}
        copies["hft"] = copies["ft"]
        d_x.free()
        cb = None
        if not args.no_cpu:
            cb = {"kind": "reference", "cores": 1, "sample": "the reference's expressions on the float32 array, whole"}
            a = time.perf_counter()
            np.mean(np.abs(np.fft.fft(x, axis=0)) ** 2.0, axis=1)
            cb["ft_seconds"] = time.perf_counter() - a
            a = time.perf_counter()
            np.mean(np.abs(np.fft.fft(x, axis=1)) ** 2.0, axis=0)
            cb["hft_seconds"] = time.perf_counter() - a
            a = time.perf_counter()
            for t in range(tnum):
                scipy.signal.periodogram(x[:, t], fs=fs, window='hann', scaling='spectrum')
            cb["periodogram_seconds"] = time.perf_counter() - a
        print(json.dumps({"path": "spectra %d x %d float32" % (snum, tnum),
                          "config": "ft: transpose to float64 + %d rows of %d (own power-of-two transform); hft: %d rows of %d (own "
                                    "mixed-radix transform); periodogram: hann, 'spectrum', the image stays resident" % (tnum, snum, snum, tnum),
                          "device_ms": {k: v["median"] for k, v in ms.items()}, "device_ms_spread": ms,
                          "compulsory_bytes": nbytes,
                          "hbm_frac": {k: nbytes[k] / ms[k]["median"] / 1e6 / 8000.0 for k in ms},
                          "copy_same_bytes_ms": copies,
                          "time_over_copy": {k: ms[k]["median"] / copies[k]["median"] for k in ms},
                          "first_call": spectra_first,
                          "roofline": {"bound": "memory", "note": "time per call (host clock around a device synchronise), with the "
                                       "download of the mean spectrum.  Compulsory bytes: the float32 radargram once, plus the float64 "
                                       "image for the periodogram; the column-wise cases move it twice more through the float64 "
                                       "transpose (write and read of 8 bytes per sample)"},
                          "cpu_baseline": cb}), flush=True)

    if 'display' not in args.skip:
        # what a plot reads from the resident radargram: the (10, 90) colour limits of all of it (4 histogram passes over the
        # float32 samples), the (1, 99) limits of a 100-trace window (plot_traces), and the flattened image (a gather, one store pass)
        import ctypes
        from impdar_amd import display
        snum, tnum = SPECTRA
        ctx, lib = _hip.context(), _hip.load()
        x = np.random.default_rng(13).standard_normal((snum, tnum)).astype(np.float32)
        d_x = _hip.DeviceArray.from_host(ctx, x)
        shift = np.round(200.0 * np.sin(np.arange(tnum) / 700.0)).astype(np.int32)
        t0 = 5000

        def spread(fn, reps=7):
            fn()
            ts = []
            for _ in range(reps):
                a = time.perf_counter()
                fn()
                lib.impdar_ctx_sync(ctx)
                ts.append((time.perf_counter() - a) * 1e3)
            return {"median": float(np.median(ts)), "min": min(ts), "max": max(ts), "reps": reps}

        def dcopy_ms(nbytes):
            half = (nbytes // 2 + 7) // 8 * 8                          # a copy reads and writes: half the bytes each way
            a = _hip.DeviceArray(ctx, (half // 8, 1), np.float64)
            b = _hip.DeviceArray(ctx, (half // 8, 1), np.float64)
            lib.impdar_dev_memset(ctx, a.ptr, 0, half)
            ms = spread(lambda: lib.impdar_cast_dev(ctx, a.ptr, _hip.F64, b.ptr, _hip.F64, ctypes.c_size_t(half // 8)))
            a.free()
            b.free()
            return ms

        def flat():
            display.flatten_dev(d_x, shift, resident=True).free()
        passes = 4                                                     # one per 8-bit digit of a float32 key
        ms = {"clims_10_90": spread(lambda: display.percentile_dev(d_x, (10, 90))),
              "traces_1_99": spread(lambda: display.percentile_dev(d_x, (1, 99), x_range=(t0, t0 + 100), skip_nan=False)),
              "flatten": spread(flat)}
        got = display.percentile_dev(d_x, (10, 90))
        nbytes = {"clims_10_90": snum * tnum * 4, "traces_1_99": snum * 100 * 4, "flatten": 2 * snum * tnum * 4}
        copies = {k: dcopy_ms(max(v, 4096)) for k, v in nbytes.items()}
        d_x.free()
        cb = None
        if not args.no_cpu:
            cb = {"kind": "reference", "cores": 1, "sample": "np.percentile as the reference calls it, on the float32 array"}
            a = time.perf_counter()
            want = np.percentile(x[~np.isnan(x)], (10, 90))
            cb["clims_10_90_seconds"] = time.perf_counter() - a
            cb["same_bits"] = bool(np.array_equal(want, got))
            a = time.perf_counter()
            np.percentile(x[:, t0:t0 + 100], (1, 99))
            cb["traces_1_99_seconds"] = time.perf_counter() - a
        print(json.dumps({"path": "display %d x %d float32" % (snum, tnum),
                          "config": "clims: (10, 90) of the whole radargram, NaNs skipped; traces: (1, 99) of traces %d-%d; flatten: every "
                                    "trace shifted by up to 200 rows, the image stays resident" % (t0, t0 + 100),
                          "device_ms": {k: v["median"] for k, v in ms.items()}, "device_ms_spread": ms,
                          "compulsory_bytes": nbytes, "histogram_passes": passes,
                          "hbm_frac": {k: nbytes[k] / ms[k]["median"] / 1e6 / 8000.0 for k in ms},
                          "copy_same_bytes_ms": copies,
                          "time_over_copy": {k: ms[k]["median"] / copies[k]["median"] for k in ms},
                          "roofline": {"bound": "memory", "note": "time per call (host clock around a device synchronise).  Compulsory "
                                       "bytes: the window once for the limits (the select streams it once per digit, %d times, with a "
                                       "download of the histograms and a host step between the passes); the radargram read and the image "
                                       "written once for the flatten" % passes},
                          "cpu_baseline": cb}), flush=True)

    if 'load' not in args.skip:
        # instrument file to resident float32 radargram: pulseEKKO-1.0-shaped records (128-byte trace header, int16 samples; the mean
        # of the first 100 samples taken off) and RAMAC-shaped ones (int16, kept as they are).  Per call with spreads: the host route
        # (decode_host, widen, to_device) against the device route (the file's bytes up as they are, decoded in HBM); the decode
        # kernels alone (the context's kernel timer, bytes already resident) against HBM on the compulsory bytes -- the records read
        # once, the result written once -- and against a device copy of the same bytes in this run
        import ctypes
        from impdar_amd import rawload
        snum, tnum = (int(v) for v in args.chain.split('x'))
        ctx, lib = _hip.context(), _hip.load()

        def lspread(fn, reps=5):
            fn()
            ts = []
            for _ in range(reps):
                a = time.perf_counter()
                fn()
                lib.impdar_ctx_sync(ctx)
                ts.append((time.perf_counter() - a) * 1e3)
            return {"median": float(np.median(ts)), "min": min(ts), "max": max(ts), "reps": reps}

        def lcopy_ms(nbytes):
            half = (nbytes // 2 + 7) // 8 * 8                          # a copy reads and writes: half the bytes each way
            a = _hip.DeviceArray(ctx, (half // 8, 1), np.float64)
            b = _hip.DeviceArray(ctx, (half // 8, 1), np.float64)
            lib.impdar_dev_memset(ctx, a.ptr, 0, half)
            ms = lspread(lambda: lib.impdar_cast_dev(ctx, a.ptr, _hip.F64, b.ptr, _hip.F64, ctypes.c_size_t(half // 8)), reps=7)
            a.free()
            b.free()
            return ms

        def load_line(label, layout, out_dtype):
            raw = np.random.default_rng(12).integers(0, 256, layout.stride * layout.tnum, dtype=np.uint8)
            out_dtype = np.dtype(out_dtype) if out_dtype is not None else rawload.native_dtype(layout)

            def host_route():
                d = _hip.DeviceArray.from_host(ctx, rawload.decode_host(raw, layout).astype(out_dtype, copy=False))
                d.free()

            def device_route():
                rawload.decode_dev(raw, layout, out_dtype, ctx=ctx).free()

            host_ms, dev_ms = lspread(host_route, reps=3), lspread(device_route)
            d_raw = _hip.DeviceArray.from_host(ctx, raw)
            kernel = []
            for _ in range(8):
                d = rawload.decode_dev(d_raw, layout, out_dtype)
                ms = ctypes.c_float()
                _hip.check(lib.impdar_ctx_last_kernel_ms(ctx, ctypes.byref(ms)), 'impdar_ctx_last_kernel_ms')
                kernel.append(ms.value)
                d.free()
            d_raw.free()
            kernel = sorted(kernel[1:])
            kernel_ms = {"min": kernel[0], "median": kernel[len(kernel) // 2], "max": kernel[-1]}
            el = rawload.IN_DTYPES[layout.in_kind].itemsize
            nbytes = layout.snum * layout.tnum * (el + out_dtype.itemsize)
            copy = lcopy_ms(nbytes)
            print(json.dumps({"path": "load %d x %d int16 records%s" % (snum, tnum, label),
                              "config": "%d MB of file to %d MB of resident %s, record of %d bytes with %d of header" %
                                        (raw.nbytes >> 20, (layout.snum * layout.tnum * out_dtype.itemsize) >> 20, out_dtype.name,
                                         layout.stride, layout.head),
                              "host_decode_widen_upload_ms": host_ms, "raw_upload_device_decode_ms": dev_ms,
                              "device_ms": kernel_ms["median"], "device_ms_spread": kernel_ms,
                              "compulsory_bytes": nbytes, "copy_same_bytes_ms": copy,
                              "kernel_events_over_copy_host_clock": kernel_ms["median"] / copy["median"],
                              "roofline": {"bound": "hbm", "achieved": nbytes / kernel_ms["median"] / 1e6, "peak": 8000.0, "unit": "GB/s",
                                           "frac": nbytes / kernel_ms["median"] / 1e6 / 8000.0,
                                           "note": "the decode kernels alone (for pulseEKKO the trace means, then the transposing pass) "
                                                   "from events on the stream, the file's bytes already resident; the copy of equal bytes "
                                                   "and the two routes per call on the host clock around a device synchronise, the file's "
                                                   "bytes in pageable host memory"}}), flush=True)

        load_line("", rawload.pe_layout(snum, tnum, True), np.float32)
        load_line(", kept int16 (RAMAC-shaped)", rawload.ramac_layout(snum, tnum), None)

    if 'gps' not in args.skip:
        # the time-offset search of kinematic GPS control: 10000 traces at 1 s inside a record of 100000 fixes, the reference's five
        # passes from offset 0 (5001 candidates over +-0.1 days, then 4 x 1001 around the running offset).  Per pass: the whole call
        # on the host clock (upload of the track and the traces, kernel, download of cc) and the kernel alone from events; the same
        # arithmetic in SciPy / NumPy (tests/gps_ref.py, the reference's lines) on one core for a sample of candidates, scaled
        import ctypes
        import os
        from impdar_amd import gpstrack
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tests'))
        import gps_ref
        tnum, ngps = 10000, 100000
        ctx, lib = _hip.context(), _hip.load()
        rng = np.random.default_rng(17)
        s_trace = np.arange(tnum, dtype=np.float64)
        s_gps = np.sort(rng.uniform(-0.12 * gps_ref.DAY, 0.12 * gps_ref.DAY + tnum, ngps))
        t, gps_t = gps_ref.DECIDED_T0 + s_trace / gps_ref.DAY, gps_ref.DECIDED_T0 + s_gps / gps_ref.DAY
        rlat = gps_ref.track_lat(s_trace - 2.5) + 2e-6 * rng.standard_normal(tnum)
        rlon = gps_ref.track_lon(s_trace - 2.5) + 2e-6 * rng.standard_normal(tnum)
        glat, glon = gps_ref.track_lat(s_gps), gps_ref.track_lon(s_gps)

        def one_pass(offset):
            sv = np.linspace(-0.1 * abs(offset), 0.1 * abs(offset), 1001) if offset != 0.0 else np.linspace(-0.1, 0.1, 5001)
            a = time.perf_counter()
            cc, nout = gpstrack.cc_search(gps_t, glat, glon, t, rlat, rlon, offset, sv, False)
            wall = (time.perf_counter() - a) * 1e3
            ms = ctypes.c_float()
            _hip.check(lib.impdar_ctx_last_kernel_ms(ctx, ctypes.byref(ms)), 'impdar_ctx_last_kernel_ms')
            return sv, cc, nout, wall, ms.value

        def five_passes():
            offset, walls, kernels = 0.0, [], []
            for _ in range(5):
                sv, cc, nout, wall, k = one_pass(offset)
                if np.any(nout):
                    raise ValueError('the GPS record does not span the search window')
                offset += sv[np.argmax(cc)]
                walls.append(wall)
                kernels.append(k)
            return offset, walls, kernels

        five_passes()
        runs = [five_passes() for _ in range(max(args.reps, 5))]
        walls, kernels = np.array([r[1] for r in runs]), np.array([r[2] for r in runs])

        def stat(v):
            return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "reps": int(len(v))}

        upload = []
        in_bytes = 8 * (3 * ngps + 3 * tnum + 5001)
        d = _hip.DeviceArray(ctx, (in_bytes // 8, 1), np.float64)
        h = np.zeros(in_bytes // 8)
        for _ in range(6):
            a = time.perf_counter()
            _hip.check(lib.impdar_dev_upload(ctx, d.ptr, h.ctypes.data_as(ctypes.c_void_p), in_bytes), 'impdar_dev_upload')
            upload.append((time.perf_counter() - a) * 1e3)
        d.free()
        upload_ms = float(np.median(upload[1:]))
        out = {"path": "gps offset search 10000 traces x 100000 fixes, 5001 + 4 x 1001 offsets",
               "config": "float64, np.interp form (no extrapolation), one workgroup of 256 threads per candidate, two passes over the "
                         "traces per candidate, one bisection of the fixes per trace and pass",
               "final_offset_s": runs[0][0] * gps_ref.DAY,
               "device_ms_per_pass": [stat(kernels[:, p]) for p in range(5)], "device_ms_five_passes": stat(kernels.sum(axis=1)),
               "call_ms_per_pass": [stat(walls[:, p]) for p in range(5)], "call_ms_five_passes": stat(walls.sum(axis=1)),
               "upload_ms_one_call": upload_ms, "upload_bytes_one_call": in_bytes,
               "upload_share_of_five_calls": 5 * upload_ms / float(np.median(walls.sum(axis=1))),
               "note": "device_ms: the search kernel alone from events on the stream; call_ms: cc_search on the host clock, every "
                       "call uploading the track and the traces again and waiting for cc; upload_ms_one_call: a synchronous copy of a "
                       "call's input bytes from pageable memory, timed by itself"}
        if not args.no_cpu:
            sample = np.linspace(-0.1, 0.1, 5001)[::500]
            a = time.perf_counter()
            gps_ref.cc_f64(gps_t, glat, glon, t, rlat, rlon, 0.0, sample, False)
            per = (time.perf_counter() - a) / len(sample)
            out["cpu_baseline"] = {"what": "the reference's interp1d + np.corrcoef lines (tests/gps_ref.cc_f64), one core, timed on %d "
                                           "candidates and scaled to 5001 + 4 x 1001" % len(sample),
                                   "ms_per_candidate": per * 1e3, "five_passes_s": per * (5001 + 4 * 1001),
                                   "speedup_over_device_calls": per * (5001 + 4 * 1001) * 1e3 / float(np.median(walls.sum(axis=1)))}
        print(json.dumps(out), flush=True)

    if 'atten' not in args.skip:
        # the window search of attenuation method 3: the pick of the decided fixtures (tests/analysis_ref.recipe) at 10000
        # traces, 30 rates, win_init = win_step = 100.  The kernel alone from events for the default target, for Nh_target 0 and
        # for Nh_target -1 (every window of every trace is visited: the worst case), the public call on the host clock, and the reference's loop
        # restated in NumPy (tests/analysis_ref.search) on one core at a reduced trace count, scaled
        import ctypes
        import os
        from impdar_amd import attsearch
        from impdar_amd.lib.analysis import attenuation
        # the one-core yardstick is the tests' restatement of the reference's loop (tests/analysis_ref.py), as for the GPS line:
        # one text of it in the repository, held to the reference's fixtures by tests/test_analysis_cpu.py
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tests'))
        import analysis_ref
        tnum, ns = 10000, np.arange(30.)
        ctx, lib = _hip.context(), _hip.load()
        z_m, power = analysis_ref.recipe(tnum, 21)
        z, pc = analysis_ref.prepared(z_m, power)

        def kernel(nh_target):
            out = attsearch.search_dev(attsearch.INDEX, z, pc, ns, 0.1, nh_target, 100, 100, first=50, ncent=tnum - 100)
            ms = ctypes.c_float()
            _hip.check(lib.impdar_ctx_last_kernel_ms(ctx, ctypes.byref(ms)), 'impdar_ctx_last_kernel_ms')
            return out, ms.value

        def stat(v):
            return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "reps": int(len(v))}

        class Bag(object):
            pass

        dat, dat.picks = Bag(), Bag()
        dat.tnum, dat.picks.z, dat.picks.corrected_power = tnum, z_m[None, :], power[None, :]
        kernel(1.)
        reps = max(args.reps, 5)
        default, zero, worst, walls = [kernel(1.) for _ in range(reps)], [kernel(0.) for _ in range(reps)], [kernel(-1.) for _ in range(reps)], []
        for _ in range(reps):
            a = time.perf_counter()
            rates, widths = attenuation.attenuation_method3(dat, 0)
            walls.append((time.perf_counter() - a) * 1e3)
        windows = lambda win: float(np.sum((win - 100.) / 100.))            # (the width after the last increment counts them)
        visits = lambda win: float(np.sum(50. * ((win - 100.) / 100.) * ((win - 100.) / 100. + 1.)))
        out = {"path": "attenuation window search 10000 traces, 30 rates",
               "config": "method 3, float64, win_init = win_step = 100, Cw 0.1; one workgroup of 256 threads per trace, a thread per "
                         "rate and eighth of the window, the window staged through LDS in tiles of 1024 pairs, the reference's passes",
               "device_ms": stat([k for _, k in default]), "device_ms_target_0": stat([k for _, k in zero]),
               "device_ms_every_window": stat([k for _, k in worst]),
               "call_ms": stat(walls),
               "windows_visited": windows(default[0][0][1]), "windows_visited_target_0": windows(zero[0][0][1]),
               "windows_visited_every_window": windows(worst[0][0][1]),
               "element_visits": visits(default[0][0][1]), "element_visits_target_0": visits(zero[0][0][1]),
               "element_visits_every_window": visits(worst[0][0][1]),
               "stopped_before_the_edge": float(np.mean((widths[50:tnum - 50] // 2 <= np.arange(50, tnum - 50)) &
                                                        (widths[50:tnum - 50] // 2 <= tnum - np.arange(50, tnum - 50)))),
               "note": "device_ms: the search kernel alone from events on the stream, Nh_target 1 (default), 0 (a walk still ends "
                       "where a single rate lies below Cw) and -1 (every window of every trace: the worst case); call_ms: attenuation_method3 on the host clock (dB, NaN removal, upload, kernel, download, the "
                       "loop over the outcomes); element_visits: window elements summed over the windows visited, each of them "
                       "read once per rate"}
        if not args.no_cpu:
            small = 1000
            zs, ps = analysis_ref.prepared(*analysis_ref.recipe(small, 21))
            a = time.perf_counter()
            analysis_ref.search(analysis_ref.INDEX, zs, ps, ns, 0.1, 1., 100, 100, range(50, small - 50), count=small)
            sec = time.perf_counter() - a
            ws = np.array([analysis_ref.walk(analysis_ref.INDEX, zs, ps, ns, 0.1, 1., 100, 100, tr)['win'] for tr in range(50, small - 50, 30)])
            per_visit = sec / (visits(ws) * (small - 100) / len(ws))
            out["cpu_baseline"] = {"what": "the reference's loop restated in NumPy (tests/analysis_ref.search: Python's sum over the "
                                           "window, three passes per rate), one core, timed at %d traces; extrapolated to 10000 traces by "
                                           "the element visits of the device run" % small,
                                   "s_at_%d_traces" % small: sec,
                                   "s_extrapolated": per_visit * out["element_visits"],
                                   "s_extrapolated_target_0": per_visit * out["element_visits_target_0"],
                                   "s_extrapolated_every_window": per_visit * out["element_visits_every_window"],
                                   "speedup_over_call_extrapolated": per_visit * out["element_visits"] * 1e3 / float(np.median(walls))}
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
