#!/usr/bin/env python3
"""Generate the ``D*`` golden vectors (denoise) by running the REFERENCE's ``RadarData.denoise``
(``src/impdar/lib/RadarData/_RadarDataFiltering.py:552-587``, imported -- never copied) on small synthetic
radargrams: a strong flat band, antenna ringing, a dipping reflector and noise.  int16 cases run the reference on
``data.astype(float64)``: the reference squares int16 in int16, which wraps (difference 1).  Only
runs where the reference is installed; the committed ``*.npz`` files are what travels.

Usage:  python tests/golden/make_golden_denoise.py
"""
import os
import sys

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


def save(name, **arrs):
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **arrs, **VERS)
    print('wrote', path, os.path.getsize(path), 'bytes')


def case(name, ftype, dtype, win, seed, snum=120, tnum=80, amp=1.0, noise=None):
    data = radargram(snum, tnum, dtype, seed, amp)
    d = NoInitRadarData(big=True)
    widen = ftype == 'wiener' and np.issubdtype(dtype, np.integer)
    d.data = data.astype(np.float64) if widen else data.copy()
    d.snum, d.tnum = data.shape
    d.denoise(vert_win=win[0], hor_win=win[1], noise=noise, ftype=ftype)
    if ftype == 'median':
        assert d.data.dtype == data.dtype
    else:
        assert d.data.dtype == np.float64
    save(name, ftype=ftype, data=data, win=np.array(win), noise=np.nan if noise is None else float(noise),
         out=d.data)


def main():
    case('D1_wiener_f64_1x10', 'wiener', np.float64, (1, 10), 1)
    case('D2_wiener_f32_3x5', 'wiener', np.float32, (3, 5), 2)
    case('D3_wiener_f64_even_4x6', 'wiener', np.float64, (4, 6), 3)
    case('D4_wiener_f32_even_4x6', 'wiener', np.float32, (4, 6), 4)
    case('D5_wiener_past_array', 'wiener', np.float64, (41, 25), 5, snum=30, tnum=20)
    case('D6_wiener_noise_given', 'wiener', np.float64, (5, 5), 6, noise=0.05)
    case('D7_wiener_int16', 'wiener', np.int16, (1, 10), 7, amp=300.0)
    case('D8_median_f64_1x10', 'median', np.float64, (1, 10), 8)
    case('D9_median_f32_5x5', 'median', np.float32, (5, 5), 9)
    case('DA_median_int16_even_4x6', 'median', np.int16, (4, 6), 10, amp=300.0)
    case('DB_median_past_array', 'median', np.float64, (30, 21), 11, snum=12, tnum=9)
    case('DC_median_1x1', 'median', np.float32, (1, 1), 12)
    case('DD_median_f32_9x9', 'median', np.float32, (9, 9), 13)


if __name__ == '__main__':
    main()
