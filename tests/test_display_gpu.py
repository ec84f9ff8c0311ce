"""The display unit on the MI355X (csrc/display.hip): order statistics and percentiles of a window, the flattened image,
the window copy, the plots drawn from them and ``impplot rg`` -- through the host-buffer and the resident entry points,
as float32 and as float64.

Everything here is exact.  The order statistics are the values np.partition puts at the ranks, the percentiles are
np.percentile's, the flattened image and the window are the arrays the reference handed to imshow (the FD* fixtures,
tests/golden/make_golden_display.py), bit for bit with NaNs in the same places; only the sign of a zero is left open
(np.partition does not order -0.0 and 0.0 either).
"""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import display_ref as dr
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

NAMES = dr.fixture_names(GOLDEN)
# shape, (y_range, x_range): the odd start of (37, 19) misaligns every row; 512 x 2051 merges many workgroups
SHAPES = [((1, 1), None), ((1, 3), None), ((5, 1), None), ((37, 19), ((3, 30), (1, 18))), ((64, 257), ((0, -1), (255, 257))),
          ((130, 1030), None), ((512, 2051), None)]
QS = ((10, 90), (1, 99), (0, 100), (50,))
KINDS = ('normal', 'negative', 'constant', 'three', 'narrow', 'special', 'nan30')


def same(a, b):
    """Equal bit for bit up to the sign of a zero, NaNs in the same places."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def make(kind, shape, dtype, rng):
    n = shape[0] * shape[1]
    if kind == 'normal':
        x = rng.standard_normal(n) * 100.0
    elif kind == 'negative':
        x = -np.abs(rng.standard_normal(n)) - 1.0e-3
    elif kind == 'constant':
        x = np.full(n, -2.5)
    elif kind == 'three':
        x = rng.choice([-1.5, 0.25, 7.0], n)
    elif kind == 'narrow':
        # every value in [1, 1 + 2^-12): float32 keys differ in the low 10 bits alone, float64 keys in the low 32
        x = 1.0 + rng.integers(0, 2 ** 10 if dtype == np.float32 else 2 ** 32, n) * (2.0 ** -23 if dtype == np.float32 else 2.0 ** -52)
    elif kind == 'special':
        tiny = float(np.finfo(dtype).smallest_subnormal)
        x = rng.standard_normal(n)
        x[rng.integers(0, n, max(n // 5, 1))] = rng.choice([np.inf, -np.inf, tiny, -tiny, 3 * tiny, 0.0, -0.0], max(n // 5, 1))
    elif kind == 'nan30':
        x = rng.standard_normal(n)
        x[rng.random(n) < 0.3] = np.nan
        if n > 1 and np.isnan(x).all():
            x[0] = 1.0
    x = x.astype(dtype).reshape(shape)
    if kind == 'narrow':
        assert x.min() >= 1.0 and x.max() < 1.0 + 2.0 ** -12
    return x


def windows(shape, win):
    yr, xr = win if win else ((0, -1), (0, -1))
    y1, x1 = (shape[0] if yr[1] == -1 else yr[1]), (shape[1] if xr[1] == -1 else xr[1])
    return yr, xr, (slice(yr[0], y1), slice(xr[0], x1))


def order_stats(hip, data, dev, yr, xr, q, skip_nan):
    """The C entry itself: (N, nan_count, vals) through the host-buffer form (dev None) or the resident one."""
    lib = hip.load()
    snum, tnum = data.shape
    y1, x1 = (snum if yr[1] == -1 else yr[1]), (tnum if xr[1] == -1 else xr[1])
    qa = np.ascontiguousarray(q, dtype=np.float64)
    counts, vals = (C.c_longlong * 2)(), np.zeros(2 * qa.size, dtype=data.dtype)
    if dev is None:
        rc = lib.impdar_order_stats(hip.context(), data.ctypes.data_as(C.c_void_p), hip.dtype_code(data.dtype), snum, tnum, yr[0], y1, xr[0],
                                    x1, hip.as_dp(qa)[1], qa.size, int(skip_nan), counts, vals.ctypes.data_as(C.c_void_p))
    else:
        rc = lib.impdar_order_stats_dev(dev.ctx, dev.ptr, hip.dtype_code(data.dtype), snum, tnum, yr[0], y1, xr[0], x1, hip.as_dp(qa)[1],
                                        qa.size, int(skip_nan), counts, vals.ctypes.data_as(C.c_void_p))
    hip.check(rc, 'impdar_order_stats')
    return counts[0], counts[1], vals


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('shape,win', SHAPES)
def test_order_statistics_and_percentiles_are_numpys(hip, shape, win, dtype):
    from impdar_amd import display
    rng = np.random.default_rng(shape[0] * 10007 + shape[1])
    yr, xr, sl = windows(shape, win)
    for kind in KINDS:
        data = make(kind, shape, dtype, rng)
        w = data[sl].reshape(-1)
        kept = w[~np.isnan(w)]
        dev = hip.DeviceArray.from_host(hip.context(), data)
        try:
            for q in QS:
                if kept.size == 0:
                    for d in (None, dev):
                        N, nan, vals = order_stats(hip, data, d, yr, xr, q, True)
                        assert (N, nan) == (w.size, w.size) and np.isnan(vals).all()
                    continue
                lo, hi, _ = dr.ranks(kept.size, np.asarray(q, dtype=np.float64))
                ranks = np.stack((lo, hi), axis=1).reshape(-1)
                want_vals = np.partition(kept, np.unique(ranks))[ranks]
                with np.errstate(invalid='ignore'):
                    want = np.percentile(kept, q)
                for d in (None, dev):
                    N, nan, vals = order_stats(hip, data, d, yr, xr, q, True)
                    assert (N, nan) == (w.size, w.size - kept.size), (kind, q)
                    assert same(vals, want_vals), (kind, q, d is None)
                    again = order_stats(hip, data, d, yr, xr, q, True)
                    assert again[2].tobytes() == vals.tobytes()                 # two calls, the same bits
                    got = display.percentile_host(data, q, yr, xr) if d is None else display.percentile_dev(d, q, yr, xr)
                    assert same(got, want), (kind, q, d is None)
            assert np.array_equal(dev.to_host(), data, equal_nan=True)            # the radargram stays as it was
        finally:
            dev.free()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('shape,win', SHAPES)
def test_nans_that_are_not_skipped_and_windows_without_values(hip, shape, win, dtype):
    from impdar_amd import display
    rng = np.random.default_rng(5)
    yr, xr, sl = windows(shape, win)
    data = make('normal', shape, dtype, rng)
    one = data.copy()
    one[sl][-1, -1] = np.nan                    # one NaN, in the window's last corner
    nothing = data.copy()
    nothing[sl] = np.nan                        # the window all NaN (the rest is not)
    for arr in (one, nothing):
        dev = hip.DeviceArray.from_host(hip.context(), arr)
        try:
            for form in ('host', 'dev'):
                def pct(q, skip_nan):
                    if form == 'host':
                        return display.percentile_host(arr, q, yr, xr, skip_nan)
                    return display.percentile_dev(dev, q, yr, xr, skip_nan)
                if arr is one and arr[sl].size == 1:
                    continue                                    # (that window is the all-NaN one)
                if arr is one:
                    for q in QS:
                        got = pct(q, False)
                        assert got.shape == (len(q),) and np.isnan(got).all() and np.isnan(np.percentile(arr[sl], q)).all()
                    N, nan, vals = order_stats(hip, arr, None if form == 'host' else dev, yr, xr, (10, 90), False)
                    assert (N, nan) == (arr[sl].size, 1) and np.isnan(vals).all()
                    if arr[sl].size > 1:
                        w = arr[sl].reshape(-1)
                        assert same(pct((10, 90), True), np.percentile(w[~np.isnan(w)], (10, 90)))
                else:
                    with pytest.raises(IndexError):
                        pct((10, 90), True)                     # nothing is left to rank: np.percentile of an empty array
                    assert np.isnan(pct((10, 90), False)).all() and np.isnan(np.percentile(arr[sl], (10, 90))).all()
        finally:
            dev.free()


def test_more_percentages_than_one_call_takes_and_a_scalar(hip):
    from impdar_amd import display
    data = make('normal', (130, 1030), np.float32, np.random.default_rng(11))
    q = np.linspace(0.0, 100.0, 19)
    assert same(display.percentile_host(data, q), np.percentile(data, q))
    got = display.percentile_host(data, 37.5)
    assert isinstance(got, np.float64) and got == np.percentile(data, [37.5])[0]
    ints = np.round(data).astype(np.int16)                                  # integers are widened by work_array
    assert same(display.percentile_host(ints, (10, 90)), np.percentile(ints.astype(np.float64), (10, 90)))


def test_c_entries_refuse_bad_arguments(hip):
    lib, ctx = hip.load(), hip.context()
    data = np.zeros((8, 4), dtype=np.float32)
    p = data.ctypes.data_as(C.c_void_p)
    counts, vals = (C.c_longlong * 2)(), np.zeros(16, dtype=np.float32)
    v = vals.ctypes.data_as(C.c_void_p)
    q = hip.as_dp(np.array([10.0, 90.0]))[1]
    bad_q = hip.as_dp(np.array([10.0, 100.5]))[1]
    nan_q = hip.as_dp(np.array([np.nan, 50.0]))[1]
    assert lib.impdar_order_stats(ctx, p, hip.F32, 8, 4, 0, 8, 0, 4, q, 2, 1, counts, v) == 0
    assert lib.impdar_order_stats(ctx, p, hip.F32, 8, 4, 0, 9, 0, 4, q, 2, 1, counts, v) == hip.ERR_ARG
    assert lib.impdar_order_stats(ctx, p, hip.F32, 8, 4, 3, 2, 0, 4, q, 2, 1, counts, v) == hip.ERR_ARG
    assert lib.impdar_order_stats(ctx, p, hip.F32, 8, 4, 0, 8, -1, 4, q, 2, 1, counts, v) == hip.ERR_ARG
    assert lib.impdar_order_stats(ctx, p, hip.F32, 8, 4, 0, 8, 0, 4, q, 9, 1, counts, v) == hip.ERR_ARG
    assert lib.impdar_order_stats(ctx, p, hip.F32, 8, 4, 0, 8, 0, 4, q, 0, 1, counts, v) == hip.ERR_ARG
    assert lib.impdar_order_stats(ctx, p, hip.F32, 8, 4, 0, 8, 0, 4, bad_q, 2, 1, counts, v) == hip.ERR_ARG
    assert lib.impdar_order_stats(ctx, p, hip.F32, 8, 4, 0, 8, 0, 4, nan_q, 2, 1, counts, v) == hip.ERR_ARG
    assert lib.impdar_order_stats(ctx, p, 5, 8, 4, 0, 8, 0, 4, q, 2, 1, counts, v) == hip.ERR_ARG
    assert lib.impdar_order_stats(ctx, None, hip.F32, 8, 4, 0, 8, 0, 4, q, 2, 1, counts, v) == hip.ERR_ARG
    # an empty window is reported through the counts
    assert lib.impdar_order_stats(ctx, p, hip.F32, 8, 4, 2, 2, 0, 4, q, 2, 1, counts, v) == 0 and list(counts) == [0, 0]
    assert np.isnan(vals[:4]).all()
    shift = np.zeros(4, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    out = np.zeros((8, 4), dtype=np.float32).ctypes.data_as(C.c_void_p)
    assert lib.impdar_flatten(ctx, p, hip.F32, 8, 4, 0, 4, shift, out) == 0
    assert lib.impdar_flatten(ctx, p, hip.F32, 8, 4, 2, 2, shift, out) == hip.ERR_ARG
    assert lib.impdar_flatten(ctx, p, hip.F32, 8, 4, 0, 5, shift, out) == hip.ERR_ARG
    assert lib.impdar_flatten(ctx, p, hip.F32, 8, 4, 0, 4, None, out) == hip.ERR_ARG
    assert lib.impdar_window_dev(ctx, None, hip.F32, 8, 4, 0, 8, 0, 4, out) == hip.ERR_ARG


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('shape', [(7, 5), (64, 257), (130, 1030)])
def test_flatten_and_window_at_every_kind_of_shift(hip, shape, dtype):
    from impdar_amd import display
    snum, tnum = shape
    rng = np.random.default_rng(snum)
    data = rng.standard_normal(shape).astype(dtype)
    data[rng.random(shape) < 0.05] = np.nan
    kinds = np.array([0, 1, -1, snum - 1, -(snum - 1), snum, -snum, dr.NO_SHIFT, 3, -2], dtype=np.int64)
    dev = hip.DeviceArray.from_host(hip.context(), data)
    try:
        for first in (0, 5):                    # (five traces hold half of the kinds at a time)
            shift = kinds[(np.arange(tnum) + first) % kinds.size].astype(np.int32)
            want = dr.flatten_gather(data, shift)
            for x0, x1 in ((0, tnum), (1, tnum - 1), (tnum - 2, tnum), (0, 4)):
                sub = np.ascontiguousarray(shift[x0:x1])
                assert same(display.flatten_host(data, sub, (x0, x1)), want[:, x0:x1]), (x0, x1)
                assert same(display.flatten_dev(dev, sub, (x0, x1)), want[:, x0:x1]), (x0, x1)
                for yr in ((0, -1), (1, snum - 1), (snum // 2, snum // 2 + 1)):
                    y1 = snum if yr[1] == -1 else yr[1]
                    assert same(display.window_dev(dev, yr, (x0, x1)), data[yr[0]:y1, x0:x1])
            d_img = display.flatten_dev(dev, shift, resident=True)
            assert same(d_img.to_host(), want)
            d_img.free()
        assert display.window_dev(dev, (2, 2), (0, -1)).shape == (0, tnum)
        assert np.array_equal(dev.to_host(), data, equal_nan=True)
    finally:
        dev.free()


def make_dat(g, dtype=None):
    from impdar_amd.lib.RadarData import RadarData
    return dr.fill_dat(RadarData(None), g, dtype)


def drawn_window(g):
    """The rows and traces of a fixture's image that is not flattened: y_range after the reference's NaN-aware bound."""
    snum, tnum = g['data'].shape
    y0, y1 = int(g['y_range_in'][0]), int(g['y_range_in'][1])
    first = int(np.min(np.where(~np.isnan(g['travel_time']))[0])) if str(g['ydat']) in ('twtt', 'dual') else 0
    return (max(y0, first), snum if y1 == -1 else y1), tuple(int(v) for v in g['x_range_out'])


@pytest.mark.parametrize('name', NAMES)
def test_radardata_methods_give_the_fixtures_images(hip, name):
    g = dr.load_fixture(GOLDEN, name)
    layer = int(g['flatten_layer'])
    for resident in (False, True):
        dat = make_dat(g)
        if resident:
            dat.to_device()
        x_range = tuple(int(v) for v in g['x_range_in'])
        y_range = tuple(int(v) for v in g['y_range_in'])
        assert same(dat.percentiles((10, 90), y_range, x_range), g['clims'])
        if layer >= 0:
            assert same(dat.flattened(layer, x_range), g['image'])
        else:
            yr, xr = drawn_window(g)
            assert same(dat.window(yr, xr), g['image'])
        assert (dat._dev is not None and dat.data is None) if resident else dat._dev is None
        if resident:
            dat.from_device()
            assert same(dat.data, g['data'])


@pytest.mark.parametrize('name', NAMES)
def test_plots_return_what_the_reference_returned(hip, name):
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    from impdar_amd.lib import plot
    g = dr.load_fixture(GOLDEN, name)
    layer = int(g['flatten_layer'])
    for resident in (False, True):
        dat = make_dat(g)
        if resident:
            dat.to_device()
        im, xd, yd, x_range, clims = plot.plot_radargram(dat, xdat=str(g['xdat']), ydat=str(g['ydat']), x_range=tuple(int(v) for v in g['x_range_in']),
                                                         y_range=tuple(int(v) for v in g['y_range_in']),
                                                         flatten_layer=None if layer < 0 else layer, return_plotinfo=True)
        shown = im.get_array()
        assert same(clims, g['clims']) and tuple(x_range) == tuple(g['x_range_out'])
        assert same(np.ma.getdata(shown), g['image']) and np.array_equal(np.ma.getmaskarray(shown), g['image_mask'])
        assert np.array_equal(np.asarray(im.get_extent(), dtype=np.float64), g['extent'])
        assert im.get_clim() == (g['clims'][0], g['clims'][1]) and im.get_cmap().name == 'gray'
        fig, ax = plot.plot_traces(dat, tuple(int(v) for v in g['tr']))
        assert np.array_equal(np.asarray(ax.get_xlim(), dtype=np.float64), g['trace_xlim'])
        t0, t1 = int(g['tr'][0]), int(g['tr'][1])
        assert len(ax.lines) == max(t1 - t0, 1) and np.array_equal(np.asarray(ax.lines[0].get_xdata()), g['data'][:, t0], equal_nan=True)
        assert (ax.get_xlabel(), ax.get_ylabel()) == ('Amplitude', 'Two way travel time (usec)')
        if 'power_c' in g:
            fig, ax = plot.plot_power(dat, int(g['power_layer']))
            sc = ax.collections[0]
            assert same(np.ma.getdata(sc.get_array()).astype(np.float64), g['power_c'])
            assert np.array_equal(np.asarray(sc.get_clim(), dtype=np.float64), g['power_clims'])
            assert (ax.get_xlabel(), ax.get_ylabel()) == ('Easting', 'Northing')
            if np.nanmin(g['samp1']) >= 0 and np.nanmax(g['samp3']) < g['data'].shape[0]:        # (picks with rows outside the radargram cannot be drawn)
                fig, ax = plot.plot_radargram(dat, pick_colors=True, flatten_layer=None if layer < 0 else layer)
                assert len(ax.lines) == 6 and ax.get_xlabel() == 'Trace number'       # top, middle and bottom of two picks
        assert dat._dev is not None if resident else dat.data is not None
        plt.close('all')


def test_plot_errors_are_the_references(hip):
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    from impdar_amd.lib import plot
    dat = make_dat(dr.load_fixture(GOLDEN, 'FD03_37x19_f32_flatten'))
    with pytest.raises(ValueError, match='x axis choices are tnum or dist'):
        plot.plot_radargram(dat, xdat='km')
    with pytest.raises(ValueError, match='Unrecognized ydat'):
        plot.plot_radargram(dat, ydat='fathoms')
    with pytest.raises(ValueError, match='Elevation plot requested but we have none'):
        plot.plot_radargram(dat, ydat='elev')
    with pytest.raises(ValueError, match='That layer is not in existence, cannot flatten'):
        plot.plot_radargram(dat, flatten_layer=99)
    with pytest.raises(ValueError, match='y axis choices are twtt or depth'):
        plot.plot_traces(dat, 3, ydat='elev')
    with pytest.raises(ValueError, match='tr must either be a 2-tuple'):
        plot.plot_traces(dat, (1, 2, 3))
    with pytest.raises(ValueError, match='Pick number 99 not found in your file'):
        plot.plot_power(dat, 99)
    dat.dist = None
    with pytest.raises(ValueError, match='xdat cannot be dist when the data has no dist'):
        plot.plot_radargram(dat, xdat='dist')
    # another attribute's colour limits come from NumPy on the host attribute
    dat.other = dat.data * 2.0
    clims = plot.plot_radargram(dat, data_name='other', return_plotinfo=True)[4]
    assert same(clims, np.percentile(dat.other, (10, 90)))
    plt.close('all')


def test_impplot_rg_saves_a_file_in_a_fresh_process(hip, tmp_path):
    fn = str(tmp_path / 'line.mat')
    shutil.copy(os.path.join(GOLDEN, 'PK_ref_saved_picked.mat'), fn)
    env = dict(os.environ, MPLBACKEND='Agg')
    for args, ext in ((['rg', '-s', '-picks', '-flatten_layer', '2', fn], 'png'), (['traces', '-s', '--o_fmt', 'pdf', fn, '3', '9'], 'pdf')):
        out = subprocess.run([sys.executable, '-m', 'impdar_amd.bin.impplot'] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:]
        assert os.path.getsize(str(tmp_path / ('line.' + ext))) > 1000
