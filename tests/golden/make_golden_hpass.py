#!/usr/bin/env python3
"""Generate the ``W*`` golden vectors (horizontal frequency filters) by running the REFERENCE's
``horizontal_band_pass``, ``highpass`` and ``lowpass`` (``src/impdar/lib/RadarData/_RadarDataFiltering.py:138-350``,
imported -- never copied) on small synthetic radargrams: dipping and flat reflectors plus noise, so that every
wavelength band has something to pass.  Also records the reference's exception type and message for every
failure branch, and what it does with constant spacing -> save -> load -> ``horizontal_band_pass`` through a
``.mat`` file.  Only runs where the reference is installed; the committed ``*.npz`` files are what travels.

Usage:  python tests/golden/make_golden_hpass.py
"""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference/src')

from impdar.lib.NoInitRadarData import NoInitRadarData          # noqa: E402
from impdar.lib.RadarData import RadarData                      # noqa: E402

VERS = dict(numpy_version=np.__version__, scipy_version=scipy.__version__)


def radargram(snum, tnum, dtype, seed, amp=1.0):
    rng = np.random.default_rng(seed)
    t = np.arange(snum)[:, None]
    x = np.arange(tnum)[None, :]
    data = 0.3 * rng.standard_normal((snum, tnum))
    data += 2.0 * np.cos(2 * np.pi * x / 37.0 + 0.3 * t)                      # short horizontal wavelength
    data += 1.5 * np.sin(2 * np.pi * x / 400.0 + 0.1 * t)                     # long horizontal wavelength
    data += 3.0 * np.exp(-0.5 * ((t - (2 + 0.01 * x)) / 1.5) ** 2)            # gently dipping reflector
    data += 1.0                                                               # flat offset
    data *= amp
    if np.issubdtype(dtype, np.integer):
        return np.round(data).astype(dtype)
    return data.astype(dtype)


def make_dat(data, spacing=1.0, dt=1e-8):
    d = NoInitRadarData(big=True)
    d.data = data.copy()
    d.snum, d.tnum = data.shape
    d.dt = dt
    d.travel_time = np.arange(d.snum) * dt * 1e6
    d.flags.interp = np.array([1.0, spacing])
    return d


def save(name, **arrs):
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **arrs, **VERS)
    print('wrote', path, os.path.getsize(path), 'bytes')


def case(name, method, args, dtype, snum, tnum, seed, spacing=1.0, dt=1e-8, amp=1.0):
    from scipy.signal import butter
    d = make_dat(radargram(snum, tnum, dtype, seed, amp), spacing, dt)
    data = d.data.copy()
    out_buf = io.StringIO()
    with contextlib.redirect_stdout(out_buf):
        getattr(d, method)(*args)
    # the design the method used, restated from its printed resolution (checked against the output below)
    if method == 'horizontal_band_pass':
        nh, nl = int(args[0] / spacing), int(args[1] / spacing)
        b, a = butter(5, [(100. / nl) / 50., (100. / nh) / 50.], 'bandpass')
    else:
        nsamp = int(int(args[0]) / spacing)
        c = (100. / float(nsamp)) * 1.0e6 / ((1. / dt) / 2.0)
        b, a = butter(5, c, 'high') if method == 'highpass' else butter(3, c, 'low')
    from scipy.signal import filtfilt
    assert np.array_equal(filtfilt(b, a, data, axis=1), d.data, equal_nan=True), name
    save(name, method=method, args=np.array(args, dtype=np.float64), data=data, dt=dt,
         interp=np.asarray(d.flags.interp, dtype=np.float64), b=b, a=a, out=d.data,
         flags_hfilt=np.asarray(d.flags.hfilt, dtype=np.float64), stdout=out_buf.getvalue())


def errors():
    """(label, method, args, tnum, spacing, dt, flags tweak) -> the reference's exception type and message."""
    rows = [
        ('interp_none', 'horizontal_band_pass', (5., 100.), 200, 1.0, 1e-8, 'interp_none'),
        ('interp_zero', 'lowpass', (10.,), 200, 1.0, 1e-8, 'interp_zero'),
        ('elev', 'highpass', (10.,), 200, 1.0, 1e-8, 'elev'),
        ('hbp_low_ge_high', 'horizontal_band_pass', (100., 100.), 200, 1.0, 1e-8, ''),
        ('hbp_low_le_0', 'horizontal_band_pass', (0., 100.), 200, 1.0, 1e-8, ''),
        ('hbp_nsamp_high_lt_1', 'horizontal_band_pass', (0.5, 100.), 200, 1.0, 1e-8, ''),
        ('hbp_nsamp_low_gt_tnum', 'horizontal_band_pass', (5., 300.), 200, 1.0, 1e-8, ''),
        ('hbp_padlen', 'horizontal_band_pass', (3., 30.), 33, 1.0, 1e-8, ''),
        ('hbp_butter_corner', 'horizontal_band_pass', (2., 30.), 200, 1.0, 1e-8, ''),
        ('lp_nsamp_lt_1', 'lowpass', (0.9,), 200, 1.0, 1e-8, ''),
        ('lp_nsamp_gt_tnum', 'lowpass', (300.,), 200, 1.0, 1e-8, ''),
        ('lp_padlen', 'lowpass', (10.,), 12, 1.0, 1e-8, ''),
        ('lp_butter_corner', 'lowpass', (2.,), 200, 1.0, 1e-8, ''),
        ('hp_nsamp_lt_1', 'highpass', (3.,), 200, 4.0, 1e-8, ''),
        ('hp_nsamp_gt_tnum', 'highpass', (300.,), 200, 1.0, 1e-8, ''),
        ('hp_padlen', 'highpass', (10.,), 18, 1.0, 1e-8, ''),
        ('hp_butter_corner', 'highpass', (1.,), 200, 1.0, 1e-8, ''),
    ]
    labels, methods, args, tnums, spacings, dts, tweaks, types, messages = [], [], [], [], [], [], [], [], []
    for label, method, a, tnum, spacing, dt, tweak in rows:
        d = make_dat(radargram(4, tnum, np.float64, 99), spacing, dt)
        if tweak == 'interp_none':
            d.flags.interp = None
        elif tweak == 'interp_zero':
            d.flags.interp = np.zeros((2,))
        elif tweak == 'elev':
            d.flags.elev = 1
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                getattr(d, method)(*a)
        except Exception as e:                                       # noqa: BLE001 -- recording what it raises
            types.append(type(e).__name__)
            messages.append(str(e))
        else:
            raise AssertionError('the reference accepted ' + label)
        labels.append(label)
        methods.append(method)
        args.append(list(a) + [np.nan] * (2 - len(a)))
        tnums.append(tnum)
        spacings.append(spacing)
        dts.append(dt)
        tweaks.append(tweak)
    save('WE_errors', label=np.array(labels), method=np.array(methods), args=np.array(args), tnum=np.array(tnums),
         spacing=np.array(spacings), dt=np.array(dts), tweak=np.array(tweaks), exc_type=np.array(types),
         message=np.array(messages))


def mat_round_trip():
    """constant_space -> save -> load -> horizontal_band_pass through a .mat file, in the reference."""
    rng = np.random.default_rng(7)
    snum, tnum = 6, 300
    d = NoInitRadarData(big=True)
    d.data = rng.standard_normal((snum, tnum))
    d.snum, d.tnum = snum, tnum
    d.travel_time = np.arange(snum) * 0.01
    d.dt = 1e-8
    d.dist = np.hstack(([0.], np.cumsum(0.8 + 0.4 * rng.random(tnum - 1)))) / 1000.
    for attr in ('lat', 'long', 'x_coord', 'y_coord', 'decday', 'pressure', 'elev', 'trace_num', 'trig'):
        setattr(d, attr, np.arange(tnum, dtype=float))
    d.trace_int = np.ones(tnum)
    d.elevation = np.zeros(tnum)
    with contextlib.redirect_stdout(io.StringIO()):
        d.constant_space(1.0)
    spaced = d.data.copy()
    with tempfile.TemporaryDirectory() as tmp:
        fn = os.path.join(tmp, 'line_raw.mat')
        d.save(fn)
        e = RadarData(fn)
        loaded_interp = np.asarray(e.flags.interp, dtype=np.float64)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                e.horizontal_band_pass(5., 100.)
            result = dict(ok=True, exc_type='', message='', out=e.data)
        except Exception as exc:                                     # noqa: BLE001
            result = dict(ok=False, exc_type=type(exc).__name__, message=str(exc), out=np.zeros((0, 0)))
    save('WM_mat_round_trip', spaced=spaced, interp=np.asarray(d.flags.interp, dtype=np.float64),
         loaded_interp=loaded_interp, low=5., high=100., **result)


def main():
    case('W1_hbp_f64', 'horizontal_band_pass', (5., 100.), np.float64, 16, 600, 1)
    case('W2_hbp_f32', 'horizontal_band_pass', (5., 100.), np.float32, 16, 600, 2)
    case('W3_hbp_int16', 'horizontal_band_pass', (5., 100.), np.int16, 16, 600, 3, amp=30.0)
    case('W4_hbp_narrow', 'horizontal_band_pass', (20., 25.), np.float64, 12, 700, 4)     # [0.08, 0.1]
    case('W5_hbp_low_corner', 'horizontal_band_pass', (5., 1000.), np.float64, 8, 1200, 5)  # [0.002, 0.4]
    case('W6_hp_low_corner', 'highpass', (500.,), np.float64, 8, 1200, 6)                  # 0.004
    case('W7_lp_dt1', 'lowpass', (20.,), np.float64, 16, 500, 7)
    case('W8_lp_dt2', 'lowpass', (20.,), np.float32, 16, 500, 8, dt=4e-9)
    case('W9_hp_dt1', 'highpass', (20.,), np.float64, 16, 500, 9)
    case('WA_hp_dt2', 'highpass', (20.,), np.float32, 16, 500, 10, dt=4e-9)
    case('WB_hbp_spacing', 'horizontal_band_pass', (12., 240.), np.float64, 12, 600, 11, spacing=2.5)
    case('WC_hbp_tnum_padlen_plus_1', 'horizontal_band_pass', (3., 30.), np.float64, 9, 34, 12)
    case('WD_lp_tnum_padlen_plus_1', 'lowpass', (10.,), np.float64, 7, 13, 13)
    errors()
    mat_round_trip()


if __name__ == '__main__':
    main()
