#!/usr/bin/env python3
"""Generate the ``G*`` (gains), ``R*`` (reverse / hcrop / restack) and ``AW*`` (winavg_hfilt) golden vectors by
running the REFERENCE's ``rangegain``, ``agc``, ``reverse``, ``hcrop``, ``restack``
(``src/impdar/lib/RadarData/_RadarDataProcessing.py:20-47, 340-496``) and ``winavg_hfilt``
(``_RadarDataFiltering.py:353-440``), imported -- never copied -- on small synthetic radargrams.  Every file
stores the input state, the arguments, the reference's output and every attribute and flag a step may change; the
error cases store the reference's exception type and message.  Only runs where the reference is installed; the
committed ``*.npz`` files are what travels.

The windows of the float32 restack and winavg cases (3, 5, 7, 25 traces; 5, 7, 9, 11, 49 traces) are ones at which
the reference's own float32 accumulation stays below 2e-7 of max|expected| from an fp64 restatement on
``make_golden_hfilt.radargram(200, 1000, float32)`` (measured: at most 1.9e-7; 15, 21 and 31 give 2.2e-7 to 2.5e-7
and are not used), so the tests' 2e-6 bar keeps a tenfold margin over what the reference alone contributes.

Usage:  python tests/golden/make_golden_gain_taxis.py
"""
import contextlib
import io
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_hfilt import NoInitRadarData, VERS, radargram          # noqa: E402

SNUM, TNUM = 80, 48
VECTORS = ['dist', 'pressure', 'lat', 'long', 'x_coord', 'y_coord', 'elev', 'decday', 'trig', 'trace_num', 'trace_int']
FLAGS = ['rgain', 'agc', 'restack', 'reverse', 'hfilt']


def make_dat(data, trig=None, elev=True, dt_us=0.3):
    d = NoInitRadarData(big=True)
    d.data = data.copy()
    d.snum, d.tnum = data.shape
    n = d.tnum
    x = np.arange(n, dtype=np.float64)
    d.travel_time = np.arange(d.snum) * dt_us + 0.5
    d.dist = np.cumsum(0.004 + 0.001 * np.sin(x / 3.)) - 0.004
    d.pressure = 900. + 0.1 * x
    d.lat = -75. + 1e-4 * x
    d.long = 110. + 2e-4 * x ** 1.1
    d.x_coord = 1000. + 4.1 * x
    d.y_coord = 2000. - 3.3 * x + 0.01 * x ** 2
    d.elev = 1500. + 2. * np.sin(x / 5.) if elev else None
    d.decday = 100. + 1e-5 * x
    d.trig = np.zeros(n) if trig is None else trig
    d.trace_num = np.arange(n) + 1
    d.trace_int = np.full(n, 4.0)
    return d


def state(d, prefix):
    out = {prefix + 'data': np.array(d.data), prefix + 'tnum': d.tnum, prefix + 'snum': d.snum,
           prefix + 'travel_time': np.array(d.travel_time)}
    for k in VECTORS:
        if getattr(d, k) is not None:
            out[prefix + k] = np.array(getattr(d, k))
    for k in FLAGS:
        out[prefix + 'flags_' + k] = np.array(getattr(d.flags, k), dtype=np.float64)
    return out


def save(name, **arrs):
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **arrs, **VERS)
    print('wrote', path, os.path.getsize(path), 'bytes')


def case(name, kind, data, args, kwargs=None, ncalls=1, **dat_kw):
    """Run ``d.<kind>(*args, **kwargs)`` ``ncalls`` times on the reference and store the state around it."""
    kwargs = kwargs or {}
    d = make_dat(data, **dat_kw)
    arrs = dict(kind=kind, ncalls=ncalls, args=np.array(args, dtype=np.float64), **state(d, 'in_'))
    for k, v in kwargs.items():
        arrs['kw_' + k] = v
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), warnings.catch_warnings():
        warnings.simplefilter('ignore')                     # mean of an empty window, NaN in a maximum
        for _ in range(ncalls):
            getattr(d, kind)(*args, **kwargs)
    save(name, stdout=buf.getvalue(), **arrs, **state(d, 'out_'))


def rg(dtype, seed, snum=SNUM, tnum=TNUM, amp=1.0):
    return radargram(snum, tnum, dtype, seed, amp)


def errors():
    labels, types, messages = [], [], []

    def record(label, fn):
        try:
            with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
                warnings.simplefilter('ignore')
                fn()
        except Exception as e:                                       # noqa: BLE001 -- recording what it raises
            labels.append(label)
            types.append(type(e).__name__)
            messages.append(str(e))
        else:
            raise AssertionError('the reference accepted ' + label)
    f64, i16 = rg(np.float64, 90), rg(np.int16, 91, amp=300.)
    record('rangegain_int16_scalar_trig', lambda: make_dat(i16, trig=3).rangegain(0.1))
    record('rangegain_int16_vector_trig', lambda: make_dat(i16).rangegain(0.1))
    record('agc_window_1', lambda: make_dat(f64).agc(window=1))
    record('hcrop_left_or_right', lambda: make_dat(f64).hcrop(5, left_or_right='top'))
    record('hcrop_dimension', lambda: make_dat(f64).hcrop(5, dimension='snum'))
    record('hcrop_dist_too_large', lambda: make_dat(f64).hcrop(50., dimension='dist'))
    record('hcrop_dist_not_positive', lambda: make_dat(f64).hcrop(0., dimension='dist'))
    record('hcrop_tnum_0', lambda: make_dat(f64).hcrop(0))
    record('hcrop_tnum_1', lambda: make_dat(f64).hcrop(1))
    record('hcrop_tnum_too_large', lambda: make_dat(f64).hcrop(TNUM + 1))
    record('hcrop_tnum_minus_1', lambda: make_dat(f64).hcrop(-1))
    record('hcrop_tnum_too_negative', lambda: make_dat(f64).hcrop(-TNUM - 1))
    record('winavg_taper', lambda: make_dat(f64).winavg_hfilt(7, taper='cosine'))
    save('GZ_errors', label=np.array(labels), exc_type=np.array(types), message=np.array(messages), data=f64, data_int16=i16)


def main():
    rng = np.random.default_rng(70)
    # gains
    case('G1_rgain_f64_scalar_trig', 'rangegain', rg(np.float64, 1), (0.1,), trig=3)
    case('G2_rgain_f32_vector_trig', 'rangegain', rg(np.float32, 2), (0.02,),
         trig=np.hstack(([-1., -3., 0., 78., 79., 200.], rng.integers(0, 12, TNUM - 6))).astype(float))
    case('G3_rgain_f32_trig_minus1_odd_tnum', 'rangegain', rg(np.float32, 3, tnum=TNUM - 1), (0.5,), trig=-1)
    case('G4_rgain_f64_odd_tnum', 'rangegain', rg(np.float64, 4, tnum=TNUM - 1), (1.0e-2,),
         trig=rng.integers(0, 5, TNUM - 1).astype(float))
    x = rg(np.float64, 5)
    x[30:36] = 0.
    case('G5_agc_f64_even_window_zero_rows', 'agc', x, (), dict(window=4, scaling_factor=50))
    x = rg(np.float32, 6, tnum=TNUM - 1)
    x[40:52] = 0.
    x[10, 7] = np.nan
    case('G6_agc_f32_nan_window10_odd_tnum', 'agc', x, (), dict(window=10, scaling_factor=20))
    case('G7_agc_f32_odd_window', 'agc', rg(np.float32, 7), (), dict(window=7, scaling_factor=50))
    case('G8_agc_int16', 'agc', rg(np.int16, 8, amp=3.), (), dict(window=6, scaling_factor=50))
    case('G9_agc_f64_default_nan', 'agc', np.where(rng.random((SNUM, TNUM)) < 0.001, np.nan, rg(np.float64, 9)), ())
    # reverse / hcrop / restack
    case('R1_reverse_f64', 'reverse', rg(np.float64, 11), ())
    case('R2_reverse_f32_odd_tnum_no_elev', 'reverse', rg(np.float32, 12, tnum=TNUM - 1), (), elev=False)
    case('R3_reverse_int16_twice', 'reverse', rg(np.int16, 13, tnum=TNUM - 2, amp=300.), (), ncalls=2)
    case('R4_hcrop_left_tnum_f64', 'hcrop', rg(np.float64, 14), (9,), dict(left_or_right='left', dimension='tnum'))
    case('R5_hcrop_right_tnum_f32', 'hcrop', rg(np.float32, 15), (31,), dict(left_or_right='right', dimension='tnum'), trig=2.0)
    case('R6_hcrop_left_dist_int16', 'hcrop', rg(np.int16, 16, amp=300.), (0.05,), dict(left_or_right='left', dimension='dist'))
    case('R7_hcrop_right_dist_f64_odd_tnum', 'hcrop', rg(np.float64, 17, tnum=TNUM - 1), (0.1,),
         dict(left_or_right='right', dimension='dist'), elev=False)
    case('R8_hcrop_left_negative_f32_odd_tnum', 'hcrop', rg(np.float32, 18, tnum=TNUM - 1), (-10,),
         dict(left_or_right='left', dimension='tnum'))
    case('R9_hcrop_right_negative_f64', 'hcrop', rg(np.float64, 19), (-10,), dict(left_or_right='right', dimension='tnum'))
    case('RA_restack_f64_3', 'restack', rg(np.float64, 21), (3,))
    case('RB_restack_f32_even_request_remainder', 'restack', rg(np.float32, 22), (4,))
    case('RC_restack_int16_7_odd_tnum', 'restack', rg(np.int16, 23, tnum=TNUM - 1, amp=300.), (7,), elev=False)
    case('RD_restack_f32_25_odd_tnum', 'restack', rg(np.float32, 24, tnum=TNUM + 3), (25,))
    # winavg_hfilt
    case('AW1_winavg_f64_full_7', 'winavg_hfilt', rg(np.float64, 31), (7,))
    case('AW2_winavg_f32_pexp_even', 'winavg_hfilt', rg(np.float32, 32), (10,), dict(taper='pexp', filtdepth=40))
    case('AW3_winavg_int16_full', 'winavg_hfilt', rg(np.int16, 33, amp=300.), (5,))
    case('AW4_winavg_f64_past_tnum', 'winavg_hfilt', rg(np.float64, 34), (130,))
    case('AW5_winavg_f64_window1_nan', 'winavg_hfilt', rg(np.float64, 35), (1,))
    case('AW6_winavg_f32_odd_tnum_pexp_default', 'winavg_hfilt', rg(np.float32, 36, snum=130, tnum=TNUM - 1), (9,),
         dict(taper='pexp'))
    errors()


if __name__ == '__main__':
    main()
