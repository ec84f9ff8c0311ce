#!/usr/bin/env python3
"""Generate the ``H*`` golden vectors (horizontal filters) by running the REFERENCE's ``horizontalfilt`` and
``adaptivehfilt`` (``src/impdar/lib/RadarData/_RadarDataFiltering.py:19-135``, imported -- never copied) on
small synthetic radargrams: a strong flat band (direct wave / ringing), a dipping reflector and noise, with a
travel time long enough that the taper matters.  Only runs where the reference is installed; the committed
``*.npz`` files are what travels.

Usage:  python tests/golden/make_golden_hfilt.py
"""
import contextlib
import io
import os
import sys
import warnings

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference/src')

from impdar.lib.NoInitRadarData import NoInitRadarData          # noqa: E402

VERS = dict(numpy_version=np.__version__, scipy_version=scipy.__version__)


def radargram(snum, tnum, dtype, seed, amp=1.0):
    rng = np.random.default_rng(seed)
    t = np.arange(snum)[:, None]
    x = np.arange(tnum)[None, :]
    data = 0.3 * rng.standard_normal((snum, tnum))
    data += 5.0 * np.exp(-0.5 * ((t - 8) / 2.0) ** 2) * np.cos(0.9 * t)          # flat band near the top
    data += 2.0 * ((t - 20) % 37 == 0)                                         # antenna ringing, flat
    data += 1.5 * np.exp(-0.5 * ((t - (40 + 1.2 * x)) / 1.5) ** 2)             # dipping reflector
    data *= amp
    if np.issubdtype(dtype, np.integer):
        return np.round(data).astype(dtype)
    return data.astype(dtype)


def make_dat(data, dt_us=0.3):
    d = NoInitRadarData(big=True)
    d.data = data.copy()
    d.snum, d.tnum = data.shape
    d.travel_time = np.arange(d.snum) * dt_us + 0.5        # microseconds: exp(-0.05 tt) falls to ~0.05 at 60 us
    return d


def save(name, **arrs):
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **arrs, **VERS)
    print('wrote', path, os.path.getsize(path), 'bytes')


def hfilt_case(name, dtype, bounds, seed, snum=200, tnum=100, amp=1.0):
    d = make_dat(radargram(snum, tnum, dtype, seed, amp))
    data = d.data.copy()
    with contextlib.redirect_stdout(io.StringIO()):
        d.horizontalfilt(*bounds)
    assert d.data.dtype == data.dtype
    save(name, kind='hfilt', data=data, travel_time=d.travel_time, bounds=np.array(bounds), window=0, out=d.data,
         flags_hfilt=np.asarray(d.flags.hfilt, dtype=np.float64))


def ahfilt_case(name, dtype, window, seed, snum=200, tnum=100, amp=1.0):
    d = make_dat(radargram(snum, tnum, dtype, seed, amp))
    data = d.data.copy()
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter('ignore')                     # mean of an empty window
        d.adaptivehfilt(window)
    assert d.data.dtype == data.dtype
    save(name, kind='ahfilt', data=data, travel_time=d.travel_time, bounds=np.array([0, 0]), window=window,
         out=d.data, flags_hfilt=np.asarray(d.flags.hfilt, dtype=np.float64))


def main():
    hfilt_case('H1_hfilt_f64', np.float64, (20, 75), 1)
    hfilt_case('H2_hfilt_f32', np.float32, (0, 100), 2)
    hfilt_case('H3_hfilt_int16', np.int16, (10, 60), 3, amp=300.0)
    hfilt_case('H4_hfilt_clamp_negative', np.float64, (-5, 50), 4)
    hfilt_case('H5_hfilt_clamp_past_tnum', np.float32, (70, 500), 5)
    hfilt_case('H6_hfilt_end_minus1', np.float64, (0, -1), 6)
    ahfilt_case('H7_ahfilt_f64_even', np.float64, 20, 7)
    ahfilt_case('H8_ahfilt_f32_odd', np.float32, 11, 8)
    ahfilt_case('H9_ahfilt_int16', np.int16, 16, 9, amp=300.0)
    ahfilt_case('HA_ahfilt_window_past_tnum', np.float64, 130, 10)
    ahfilt_case('HB_ahfilt_window1_nan', np.float64, 1, 11)
    ahfilt_case('HC_ahfilt_snum13', np.float64, 6, 12, snum=13, tnum=40)


if __name__ == '__main__':
    main()
