"""Layer slopes on the GPU (csrc/slope.hip), held to the yardstick of tests/slope_ref.py: 8 x the distance of ``ref`` (np.gradient,
scipy.ndimage.gaussian_filter and NumPy in float64) from ``hi`` (the contract in longdouble), per array, with the weights of
slope_ref's docstring.  The shapes (slope_ref.CASES, built from the route header's constants) are the smallest that reach every
path: the degenerate ones, a radius that passes the radargram on both axes, one trace count below, at and past each trace-block
width, one sample count below, at and past the column pass' segment, trace counts no vector width divides.

Largest ratios seen on an MI355X: see DESIGN.md 4.22.
"""
import ctypes as C
import functools
import os
import sys
from unittest.mock import patch

import numpy as np
import pytest

import slope_ref as R
from stolt_route_cases import last_metrics

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
DTYPE_IDS = ['f32', 'f64']
ROW_PASS = 'slope_row_kernel + slope_col_kernel'


def make(data, dt=1.0e-9):
    from impdar_amd import synth
    from impdar_amd.lib.RadarData import RadarData
    snum, tnum = data.shape
    geo = synth.geometry(max(snum, 2), max(tnum, 2), dt=dt, dx=1.0)
    d = RadarData(None)
    d.data, d.snum, d.tnum = data.copy(), snum, tnum
    d.travel_time, d.dist, d.trace_int, d.dt = geo['travel_time'][:snum], geo['dist'][:tnum], geo['trace_int'][:tnum], dt
    d.fn = ''
    return d


@functools.lru_cache(maxsize=None)
def yardstick(snum, tnum, dtype, sigma):
    """(x, Yard) of a shape and a sigma pair: computed once and never written to."""
    x = R.fixture(snum, tnum, dtype)
    return x, R.Yard(x, sigma)


def field_host(x, kind, sigma, max_slope=R.MAX_SLOPE):
    from impdar_amd import slope as S
    return S.slope_host(x, S.check_slope(x.shape, kind, sigma, max_slope, x.dtype))


def field_dev(x, kind, sigma, max_slope=R.MAX_SLOPE):
    from impdar_amd import _hip, slope as S
    d_x = _hip.DeviceArray.from_host(_hip.context(), x)
    d_o = _hip.DeviceArray(_hip.context(), x.shape, np.float64)
    try:
        y = S.slope_dev(d_x, S.check_slope(x.shape, kind, sigma, max_slope), d_o).to_host()
        assert np.array_equal(d_x.to_host(), x, equal_nan=True)
        return y
    finally:
        d_x.free()
        d_o.free()


def smooth_host(x, half, slope=None, sigma=(2.0, 8.0)):
    from impdar_amd import slope as S
    return S.dipsmooth_host(x, S.check_dipsmooth(x.shape, half, sigma, R.MAX_SLOPE, slope, x.dtype), slope)


def smooth_dev(x, half, slope=None, sigma=(2.0, 8.0), in_place=True):
    from impdar_amd import _hip, slope as S
    args = S.check_dipsmooth(x.shape, half, sigma, R.MAX_SLOPE, slope)
    ctx = _hip.context()
    d_x = _hip.DeviceArray.from_host(ctx, x)
    d_o = d_x if in_place else _hip.DeviceArray(ctx, x.shape, x.dtype)
    d_s = _hip.DeviceArray.from_host(ctx, slope) if slope is not None else None
    try:
        y = S.dipsmooth_dev(d_x, args, d_s, out=None if in_place else d_o).to_host()
        if not in_place:
            assert np.array_equal(d_x.to_host(), x, equal_nan=True)
        if d_s is not None:
            assert np.array_equal(d_s.to_host(), slope, equal_nan=True)
        return y
    finally:
        d_x.free()
        d_o.free()
        if d_s is not None:
            d_s.free()


def check_fields(x, Y, sigma, what):
    """Every kind: the bar, the host and the resident form and a second call the same bits, the metrics line."""
    out = {}
    for kind in R.KINDS:
        y = field_host(x, kind, sigma)
        m = last_metrics()
        assert m['entry'] == 'impdar_slope' and m['kernel'] == ROW_PASS and m['device_ms'] > 0
        assert y.dtype == np.float64 and y.shape == x.shape
        R.held('%s %s' % (kind, what), Y, y, R.slope_ref(x, kind, sigma), kind)
        assert np.array_equal(field_dev(x, kind, sigma), y) and np.array_equal(field_host(x, kind, sigma), y)
        out[kind] = y
    return out


def check_dipsmooth(x, Y, sigma, half, own, what):
    """dipsmooth with hi's slope: the bar; with its own: the bits of dipsmooth(slope=slope_host(kind 0)).  The host form, the
    resident form in place and out of place and a second call give the same bits."""
    given = Y.given_slope()
    y = smooth_host(x, half, given)
    m = last_metrics()
    assert m['entry'] == 'impdar_dipsmooth' and m['kernel'] == 'slope_gather_kernel' and m['device_ms'] > 0
    assert y.dtype == x.dtype and y.shape == x.shape
    R.held_dipsmooth('dipsmooth half %d %s' % (half, what), x, half, given, y)
    assert np.array_equal(smooth_dev(x, half, given), y) and np.array_equal(smooth_dev(x, half, given, in_place=False), y)
    assert np.array_equal(smooth_host(x, half, given), y)
    y_own = smooth_host(x, half, None, sigma)
    m = last_metrics()
    assert m['entry'] == 'impdar_dipsmooth' and m['kernel'] == ROW_PASS + ' + slope_gather_kernel'
    assert np.array_equal(y_own, smooth_host(x, half, own, sigma))
    assert np.array_equal(smooth_dev(x, half, None, sigma), y_own) and np.array_equal(smooth_dev(x, half, None, sigma, in_place=False), y_own)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_parity_host_and_resident(hip, case, dtype):
    snum, tnum = case
    for sigma in R.SIGMAS:
        x, Y = yardstick(snum, tnum, dtype, sigma)
        what = '%s %s %s' % (R.case_id(case), sigma, np.dtype(dtype).name)
        f = check_fields(x, Y, sigma, what)
        for half in R.HALVES:
            check_dipsmooth(x, Y, sigma, half, f['slope'], what)
        if sigma == (0.0, 0.0):         # no smoothing: the planes are the products themselves, one orientation per sample
            assert np.all((np.abs(f['coherence'] - 1) < 1e-12) | (f['jzz'] + f['jxx'] == 0))


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_radius_past_the_radargram_on_both_axes(hip, dtype):
    (snum, tnum), sigma = R.WIDE
    x, Y = yardstick(snum, tnum, dtype, sigma)
    f = check_fields(x, Y, sigma, 'wide %s' % np.dtype(dtype).name)
    check_dipsmooth(x, Y, sigma, R.MAX_HALF, f['slope'], 'wide %s' % np.dtype(dtype).name)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('sigma', [(1.0, 1.0), (2.0, 4.0), (0.0, 3.0)], ids=str)
def test_window_independence(hip, sigma, dtype):
    """The field of a crop offset by (3, 5) has the full radargram's bits wherever the unclamped window (the Gaussian's reach and
    the gradient's one sample more) lies inside the crop."""
    x = yardstick(130, 257, dtype, sigma)[0]
    crop = np.ascontiguousarray(x[3:3 + 70, 5:5 + 80])
    rz, rx = R.radius(sigma[0]) + 1, R.radius(sigma[1]) + 1
    for kind in R.KINDS:
        full, part = field_host(x, kind, sigma), field_host(crop, kind, sigma)
        inner = part[rz:70 - rz, rx:80 - rx]
        assert inner.size > 0 and np.array_equal(inner, full[3 + rz:3 + 70 - rz, 5 + rx:5 + 80 - rx]), kind


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_non_finite_data(hip, dtype):
    """One NaN sample gives NaN exactly where hi has it, in every kind and in dipsmooth; an Inf in its place gives the same
    result; everything else stays within the bar."""
    sigma = (2.0, 4.0)
    clean = yardstick(60, 31, dtype, sigma)[0]
    x, xi = clean.copy(), clean.copy()
    x[17, 9] = np.nan
    xi[17, 9] = -np.inf
    Y = R.Yard(x, sigma)
    for kind in R.KINDS:
        y = field_host(x, kind, sigma)
        assert np.array_equal(np.isnan(y), np.isnan(Y.hi(kind))) and 0 < np.isnan(y).sum() < y.size, kind
        assert np.array_equal(field_host(xi, kind, sigma), y, equal_nan=True), kind
        R.held('%s with a NaN %s' % (kind, np.dtype(dtype).name), Y, y, R.slope_ref(x, kind, sigma), kind)
    given = Y.given_slope()
    assert np.isnan(given).any()
    for half in R.HALVES:
        y = smooth_host(x, half, given)
        R.held_dipsmooth('dipsmooth with a NaN half %d' % half, x, half, given, y)
        assert np.array_equal(smooth_host(xi, half, given), y, equal_nan=True)
        assert np.array_equal(smooth_dev(x, half, given), y, equal_nan=True)
        own = smooth_host(x, half, None, sigma)
        assert np.array_equal(own, smooth_host(x, half, field_host(x, 'slope', sigma), sigma), equal_nan=True)
        assert np.isnan(own[np.isnan(given)]).all()


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_exact_cases(hip, dtype):
    """An all-zero radargram gives zeros; a constant one slope 0 and coherence 0; an all-zero given slope the plain clipped row
    mean."""
    zeros = np.zeros((40, 37), dtype=dtype)
    const = np.full((40, 37), 2.5, dtype=dtype)
    for kind in R.KINDS:
        assert np.all(field_host(zeros, kind, (2.0, 4.0)) == 0), kind
    assert np.all(field_host(const, 'slope', (2.0, 4.0)) == 0) and np.all(field_host(const, 'coherence', (2.0, 4.0)) == 0)
    assert np.all(smooth_host(zeros, 4) == 0) and np.all(smooth_host(const, 4) == 2.5)
    x = yardstick(60, 31, dtype, (2.0, 4.0))[0]
    flat = np.zeros(x.shape)
    for half in R.HALVES:
        y = smooth_host(x, half, flat)
        R.held_dipsmooth('row mean half %d' % half, x, half, flat, y)
        # every trace in reach, summed in float64 with i rising, divided by their number, rounded once
        n = np.zeros(x.shape)
        s = np.zeros(x.shape)
        for i in range(-half, half + 1):
            lo, hi = max(0, -i), min(31, 31 - i)
            if hi <= lo:                # (half 32 passes the 31 traces)
                continue
            s[:, lo:hi] = s[:, lo:hi] + x[:, lo + i:hi + i].astype(np.float64)
            n[:, lo:hi] += 1
        assert np.array_equal(y, (s / n).astype(dtype))
    steep = np.full(x.shape, 1.0e6)             # a given slope past the trace: the ends of the neighbours, no read outside
    assert np.array_equal(smooth_host(x, 2, steep), R.dipsmooth_ref(x, 2, steep))


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_max_slope_clamps_the_slope_alone(hip, dtype):
    sigma = (1.0, 1.0)
    x, Y = yardstick(33, 70, dtype, sigma)
    p, dip = field_host(x, 'slope', sigma, 1.0e9), field_host(x, 'dip', sigma)
    tight = field_host(x, 'slope', sigma, 0.25)
    assert np.array_equal(tight, np.clip(p, -0.25, 0.25)) and np.abs(p).max() > 0.25
    assert np.array_equal(field_host(x, 'dip', sigma, 0.25), dip)
    Y25 = R.Yard(x, sigma, 0.25)
    R.held('slope clamped at 0.25 %s' % np.dtype(dtype).name, Y25, tight, R.slope_ref(x, 'slope', sigma, 0.25), 'slope')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_methods_host_and_resident(hip, dtype):
    sigma = (2.0, 4.0)
    x = yardstick(60, 31, dtype, sigma)[0]
    want = {k: field_host(x, k, sigma) for k in ('slope', 'dip', 'coherence')}
    smoothed = smooth_host(x, 4, None, sigma)
    edited = np.ascontiguousarray(want['slope'] * 0.5)
    smoothed_given = smooth_host(x, 4, edited)
    for resident in (False, True):
        d = make(x)
        flags_before = {k: np.array(v, copy=True) for k, v in vars(d.flags).items()}
        if resident:
            d.to_device()
        for k, v in want.items():
            got = d.layer_slope(sigma=sigma, kind=k)
            assert got.dtype == np.float64 and np.array_equal(got, v), k
        assert np.array_equal(d._dev.to_host() if resident else d.data, x)                     # the data untouched
        for kw, res in ((dict(sigma=sigma), smoothed), (dict(slope=edited), smoothed_given)):
            e = make(x)
            if resident:
                e.to_device()
            e.dip_smooth(4, **kw)
            assert (getattr(e, '_dev', None) is not None) == resident
            e.from_device()
            assert np.array_equal(e.data, res) and e.data.dtype == dtype
        for k, v in flags_before.items():
            assert np.array_equal(np.asarray(getattr(d.flags, k)), v), k
        with pytest.raises(ValueError):
            d.dip_smooth(4, slope=edited[:, :-1])
        with pytest.raises(ValueError):
            d.layer_slope(kind='power')
    i = make(np.round(x * 100).astype(np.int16))
    i.dip_smooth(2, sigma=sigma)
    assert i.data.dtype == np.float64 and np.array_equal(i.data, smooth_host(np.round(x * 100).astype(np.float64), 2, None, sigma))


def _line_file(tmp_path, snum, tnum):
    from impdar_amd import synth
    from impdar_amd.lib.NoInitRadarData import NoInitRadarData
    geo = synth.geometry(snum, tnum, dt=1.0e-9, dx=1.0)
    d = NoInitRadarData(big=True)
    d.data = np.array(R.fixture(snum, tnum, np.float64))
    d.snum, d.tnum = snum, tnum
    for k in ('lat', 'long', 'trace_num', 'decday', 'trig', 'pressure'):
        setattr(d, k, np.zeros(tnum))
    d.travel_time, d.dist, d.trace_int, d.dt = geo['travel_time'], geo['dist'], geo['trace_int'], geo['dt']
    fn = str(tmp_path / 'line_raw.mat')
    d.save(fn)
    return d, fn


def test_impproc_end_to_end(hip, tmp_path):
    from impdar_amd.bin import impproc
    from impdar_amd.lib.RadarData import RadarData
    d, fn = _line_file(tmp_path, 96, 40)
    with patch.object(sys, 'argv', ['impproc', 'dipsmooth', '3', '--sigma', '1', '2', '--max_slope', '2', fn]):
        impproc.main()
    r = RadarData(str(tmp_path / 'line_dipsm.mat'))
    from impdar_amd import slope as S
    assert np.array_equal(r.data, S.dipsmooth_host(d.data, S.check_dipsmooth(d.data.shape, 3, (1.0, 2.0), 2.0)))
    assert not np.array_equal(r.data, d.data)
    for kind, suffix in (('slope', 'slope'), ('dip', 'dip'), ('coherence', 'coh')):
        with patch.object(sys, 'argv', ['impproc', 'slope', '--kind', kind, fn]):
            impproc.main()
        out_fn = str(tmp_path / ('line_%s.mat' % suffix))
        assert os.path.exists(out_fn), suffix
        r = RadarData(out_fn)
        assert r.data.shape == d.data.shape and np.array_equal(r.data, field_host(d.data, kind, (2.0, 8.0)))


def test_refusals_from_the_c_abi(hip):
    """IMPDAR_ERR_ARG from the four C entries with the route header's reason; the output is not touched."""
    lib, ctx = hip.load(), hip.context()
    x = np.array(R.fixture(100, 8, np.float32))
    out32, out64, given = np.full_like(x, 7), np.full(x.shape, 7.0), np.zeros(x.shape)
    p, q32, q64 = x.ctypes.data_as(C.c_void_p), out32.ctypes.data_as(C.c_void_p), out64.ctypes.data_as(C.POINTER(C.c_double))
    gp = given.ctypes.data_as(C.POINTER(C.c_double))
    ok = dict(dtype=0, snum=100, tnum=8, kind=0, sz=2.0, sx=8.0, ms=4.0)
    nan, inf = float('nan'), float('inf')
    reasons = [(dict(kind=6), 'kind must be 0 (slope), 1 (dip), 2 (coherence), 3 (jzz), 4 (jzx) or 5 (jxx)'), (dict(kind=-1), 'kind must be 0'),
               (dict(sz=-1.0), 'sigma must be finite and lie in 0 .. 16'), (dict(sx=16.5), 'sigma must be finite'), (dict(sz=nan), 'sigma must be finite'),
               (dict(sx=inf), 'sigma must be finite'), (dict(ms=0.0), 'max_slope must be finite and positive'), (dict(ms=nan), 'max_slope must be'),
               (dict(ms=inf), 'max_slope must be'), (dict(snum=0), 'empty radargram'), (dict(tnum=0), 'empty radargram'),
               (dict(dtype=2), 'dtype must be float32 or float64')]
    for change, reason in reasons:
        k = dict(ok, **change)
        for fn in (lib.impdar_slope, lib.impdar_slope_dev):
            rc = fn(ctx, p, k['dtype'], k['snum'], k['tnum'], k['kind'], k['sz'], k['sx'], k['ms'], C.cast(q64, C.c_void_p) if fn is lib.impdar_slope_dev else q64)
            assert rc == hip.ERR_ARG and reason in hip.last_error(), (change, hip.last_error())
    ok = dict(dtype=0, snum=100, tnum=8, half=4, sz=2.0, sx=8.0, ms=4.0)
    reasons = [(dict(half=0), 'half must lie in 1 .. 32'), (dict(half=33), 'half must lie'), (dict(half=-4), 'half must lie')] + reasons[2:]
    for change, reason in reasons:
        k = dict(ok, **change)
        for fn in (lib.impdar_dipsmooth, lib.impdar_dipsmooth_dev):
            rc = fn(ctx, p, k['dtype'], k['snum'], k['tnum'], k['half'], None, k['sz'], k['sx'], k['ms'], q32)
            assert rc == hip.ERR_ARG and reason in hip.last_error(), (change, hip.last_error())
    for change, reason in reasons[:3] + reasons[-3:]:       # with a slope given the sigmas are not read; the rest is
        k = dict(ok, **change)
        assert lib.impdar_dipsmooth(ctx, p, k['dtype'], k['snum'], k['tnum'], k['half'], gp, nan, nan, nan, q32) == hip.ERR_ARG
        assert reason in hip.last_error(), (change, hip.last_error())
    assert np.all(out32 == 7) and np.all(out64 == 7)
    probe = np.zeros(11, dtype=np.int32)
    pp = probe.ctypes.data_as(C.POINTER(C.c_int))
    assert lib.impdar_slope_route_probe(4096, 10000, 2.0, 8.0, 4, pp) == 0
    assert probe.tolist()[:3] == [8, 32, R.ROW_TX] and probe[3] == 4096 * 40 and probe[6] == 64 * 313 and probe[4] <= 160 * 1024 >= probe[7]
    assert lib.impdar_slope_route_probe(4096, 10000, 2.0, 17.0, 4, pp) == hip.ERR_ARG
    assert lib.impdar_slope_route_probe(4096, 10000, 2.0, 8.0, 0, pp) == hip.ERR_ARG
