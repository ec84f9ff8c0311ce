#!/usr/bin/env python3
"""Generate the ``FD*`` golden vectors (what the reference's radargram, trace and power plots read and draw) by running the
REFERENCE's ``plot_radargram(return_plotinfo=True)``, ``plot_traces`` and ``plot_power`` (``src/impdar/lib/plot.py:102-283,
368-533``) -- loaded by file path, never copied -- on small synthetic radargrams with synthetic picks, under the Agg
backend.  Its loaders need packages this generator has no use for, so the ``load`` module it imports is replaced by an
empty stand-in.

Stored per case, all as the reference left them:

  ``data`` (float32 or float64), ``travel_time``, ``dist``, ``long``, ``lat``; ``samp1`` / ``samp2`` / ``samp3`` / ``power``
  / ``picknums`` where the case has picks
  ``x_range_in``, ``y_range_in``, ``flatten_layer`` (-1: none), ``xdat``, ``ydat``: what ``plot_radargram`` was called with
  ``clims``, ``image`` and ``image_mask`` (``im.get_array()``: the values and where imshow masked them, the NaNs),
  ``extent``, ``x_range_out``: what it returned
  ``tr`` and ``trace_xlim``: the traces ``plot_traces`` drew and the x-limits it set
  ``power_layer``, ``power_c``, ``power_clims``: the pick ``plot_power`` drew, its colours in dB and its colour limits

The cases: both dtypes, with and without NaNs, a sub-window, NaN travel times at the top, and ``flatten_layer`` with
picks that miss traces and offsets of 0, positive, negative and of ``snum`` rows or more.

Only runs where the reference is installed; the committed files are what travels.

Usage:  python tests/golden/make_golden_display.py REFERENCE_SRC            (the directory that holds impdar/)
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_reference(src):
    """The reference's plot module under a private package name, its loaders replaced by a stand-in."""
    import matplotlib
    matplotlib.use('Agg')
    pkg = types.ModuleType('ref_impdar_lib')
    pkg.__path__ = [os.path.join(src, 'impdar', 'lib')]
    sys.modules['ref_impdar_lib'] = pkg
    stand_in = types.ModuleType('ref_impdar_lib.load')
    stand_in.load = None
    sys.modules['ref_impdar_lib.load'] = stand_in
    return importlib.import_module('ref_impdar_lib.plot')


def synthetic(rng, snum, tnum, dtype, nan_frac, nan_top):
    data = (rng.standard_normal((snum, tnum)) * 100.0 + 20.0 * np.sin(0.4 * np.arange(snum))[:, None]).astype(dtype)
    if nan_frac:
        bad = rng.random((snum, tnum)) < nan_frac
        bad[:, :4] = False                  # (plot_traces draws these traces: a NaN there would make its limits NaN)
        data[bad] = np.nan
    tt = 0.01 * np.arange(snum) + 0.01
    tt[:nan_top] = np.nan
    return dict(data=data, travel_time=tt, dist=0.003 * np.arange(tnum) ** 1.1, long=-110.0 + 0.001 * np.arange(tnum),
                lat=-80.0 + 0.0005 * np.arange(tnum))


def synthetic_picks(rng, snum, tnum, wild):
    """Two picks; number 7 wanders about the middle rows, misses some traces, and with ``wild`` holds rows far outside
    the radargram, so that its offsets reach snum rows and more."""
    mid = np.round(snum / 2 + 0.3 * snum * np.sin(0.5 * np.arange(tnum))).astype(np.float64)
    mid[1::6] = np.nan
    mid[3] = int(np.nanmean(mid))           # an offset of exactly 0
    if wild:
        mid[5], mid[8] = float(int(np.nanmean(mid)) + snum), float(int(np.nanmean(mid)) - snum - 3)
        mid[10], mid[12] = float(int(np.nanmean(mid)) + snum - 1), float(int(np.nanmean(mid)) - snum + 1)
    flat = np.full((tnum,), 4.0)
    samp2 = np.vstack((flat, mid))
    power = np.abs(rng.standard_normal((2, tnum))) * 1.0e-3 + 1.0e-6
    power[1, 2] = np.nan
    return dict(samp1=samp2 - 2.0, samp2=samp2, samp3=samp2 + 2.0, power=power, picknums=np.array([3, 7]))


def ref_dat(arrs):
    snum, tnum = arrs['data'].shape
    picks = None
    if 'samp2' in arrs:
        picks = types.SimpleNamespace(samp1=arrs['samp1'], samp2=arrs['samp2'], samp3=arrs['samp3'], power=arrs['power'],
                                      picknums=[int(p) for p in arrs['picknums']])
    return types.SimpleNamespace(data=arrs['data'], snum=snum, tnum=tnum, travel_time=arrs['travel_time'], dist=arrs['dist'],
                                 nmo_depth=None, long=arrs['long'], lat=arrs['lat'], x_coord=None, y_coord=None, fn=None,
                                 picks=picks, flags=types.SimpleNamespace(elev=False))


# name, shape, dtype, NaN fraction, NaN travel times at the top, picks (None | 'plain' | 'wild'), x_range, y_range, flatten, xdat, ydat, tr
CASES = [
    ('FD01_40x23_f32_plain', (40, 23), np.float32, 0.0, 0, None, (0, -1), (0, -1), None, 'tnum', 'twtt', (0, 3)),
    ('FD02_40x23_f64_nan_window', (40, 23), np.float64, 0.3, 2, None, (3, 20), (1, 33), None, 'tnum', 'twtt', (1, 1)),
    ('FD03_37x19_f32_flatten', (37, 19), np.float32, 0.0, 0, 'plain', (0, -1), (0, -1), 7, 'tnum', 'twtt', (2, 4)),
    ('FD04_37x19_f64_flatten_wild', (37, 19), np.float64, 0.0, 0, 'wild', (0, -1), (0, -1), 7, 'tnum', 'depth', (0, 4)),
    ('FD05_64x257_f32_flatten_window_nan', (64, 257), np.float32, 0.1, 0, 'wild', (2, 15), (0, -1), 7, 'dist', 'twtt', (0, 2)),
    ('FD06_66x260_f64_dist_dual', (66, 260), np.float64, 0.0, 3, 'plain', (1, 259), (2, 65), None, 'dist', 'dual', (3, 4)),
    ('FD07_64x300_f32_flatten', (64, 300), np.float32, 0.05, 0, 'plain', (0, -1), (0, -1), 3, 'tnum', 'twtt', (0, 1)),
]


def main(src):
    import matplotlib.pyplot as plt
    plot = load_reference(src)
    rng = np.random.default_rng(20261021)
    for name, shape, dtype, nan_frac, nan_top, picks, x_range, y_range, flatten, xdat, ydat, tr in CASES:
        arrs = synthetic(rng, shape[0], shape[1], dtype, nan_frac, nan_top)
        if picks:
            arrs.update(synthetic_picks(rng, shape[0], shape[1], picks == 'wild'))
        dat = ref_dat(arrs)
        im, xd, yd, x_out, clims = plot.plot_radargram(dat, xdat=xdat, ydat=ydat, x_range=x_range, y_range=y_range,
                                                       flatten_layer=flatten, return_plotinfo=True)
        shown = im.get_array()
        arrs.update(x_range_in=np.array(x_range), y_range_in=np.array(y_range), flatten_layer=-1 if flatten is None else flatten,
                    xdat=xdat, ydat=ydat, clims=np.asarray(clims), image=np.ma.getdata(shown), image_mask=np.ma.getmaskarray(shown),
                    extent=np.asarray(im.get_extent(), dtype=np.float64), x_range_out=np.array(x_out))
        assert np.array_equal(np.isnan(arrs['image']), arrs['image_mask']) and arrs['image'].dtype == dtype
        _, ax = plot.plot_traces(dat, tr)
        arrs.update(tr=np.array(tr), trace_xlim=np.asarray(ax.get_xlim(), dtype=np.float64))
        if picks:
            _, ax = plot.plot_power(dat, 7)
            sc = ax.collections[0]
            arrs.update(power_layer=7, power_c=np.ma.getdata(sc.get_array()).astype(np.float64),
                        power_clims=np.asarray(sc.get_clim(), dtype=np.float64))
        plt.close('all')
        path = os.path.join(HERE, name + '.npz')
        np.savez_compressed(path, numpy_version=np.__version__, **arrs)
        nbytes = os.path.getsize(path)
        print('wrote %s %d bytes; clims %r, image %s, %d masked, trace limits %r' %
              (path, nbytes, arrs['clims'], arrs['image'].shape, int(arrs['image_mask'].sum()), arrs['trace_xlim']))
        assert nbytes < 1000 * 1024, nbytes


if __name__ == '__main__':
    main(sys.argv[1])
