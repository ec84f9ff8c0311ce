"""Predictive deconvolution and the autocorrelogram on the GPU (csrc/decon.hip), held to the yardstick of tests/decon_ref.py:
max|dev - hi| <= 8 max|ref - hi| per array, with ``hi`` the contract in longdouble and ``ref`` NumPy / SciPy in float64 -- the house
margin for a different order of the same sums.  The shapes (decon_ref.CASES) are the smallest that reach every path: every access
width and its fall-back, an odd rest of traces, several trace groups, sample counts around the kernels' block C = 64, both lag
runs, a prediction that reaches across a block, and the three kinds of window.

Largest ratio max|dev - hi| / max|ref - hi| seen on an MI355X: see DESIGN.md 4.20.
"""
import ctypes as C
import functools
import os
import sys
from unittest.mock import patch

import numpy as np
import pytest

import decon_ref as R
from stolt_route_cases import last_metrics

pytestmark = pytest.mark.gpu

DT = 1.0e-9
DTYPES = [np.float32, np.float64]
DTYPE_IDS = ['f32', 'f64']


def make(data):
    from impdar_amd import synth
    from impdar_amd.lib.RadarData import RadarData
    snum, tnum = data.shape
    geo = synth.geometry(snum, max(tnum, 2), dt=DT, dx=1.0)
    d = RadarData(None)
    d.data, d.snum, d.tnum = data.copy(), snum, tnum
    d.travel_time, d.dist, d.trace_int, d.dt = geo['travel_time'], geo['dist'][:tnum], geo['trace_int'][:tnum], geo['dt']
    d.fn = ''
    return d


@functools.lru_cache(maxsize=None)
def yardstick(case, dtype, design='each'):
    """(x, hi, ref) of a case, hi and ref being (y, operators); computed once and never written to."""
    snum, tnum, oplen, gap, window = case
    x = R.ringing(snum, tnum, dtype, seed=snum + tnum) + R.noise(snum, tnum, dtype, seed=oplen + gap) * dtype(0.05)
    x = x.astype(dtype)
    hi = R.decon(x, oplen, gap, 0.1, window, design, 'hi')
    ref = R.decon(x, oplen, gap, 0.1, window, design, 'ref')
    for a in (x,) + hi + ref:
        a.setflags(write=False)
    return x, hi, ref


def held(what, got, hi, ref):
    e_dev, e_ref = R.err(got, hi), R.err(ref, hi)
    print('%s: dev %.3e ref %.3e ratio %.2f' % (what, e_dev, e_ref, e_dev / e_ref if e_ref else float(e_dev > 0)))
    assert e_dev <= 8 * e_ref, what


def run_host(x, oplen, gap, window=None, design='each', prewhiten=0.1):
    from impdar_amd import decon
    return decon.decon_host(x, decon.check_decon(x.shape, oplen, gap, prewhiten, window, design), operators=True)


def run_dev(x, oplen, gap, window=None, design='each', prewhiten=0.1, in_place=True):
    from impdar_amd import _hip, decon
    args = decon.check_decon(x.shape, oplen, gap, prewhiten, window, design)
    d_x = _hip.DeviceArray.from_host(_hip.context(), x)
    d_o = d_x if in_place else _hip.DeviceArray(_hip.context(), x.shape, x.dtype)
    try:
        res, ops = decon.decon_dev(d_x, args, out=None if in_place else d_o, operators=True)
        y = res.to_host()
        if not in_place:
            assert np.array_equal(d_x.to_host(), x, equal_nan=True)
        return y, ops
    finally:
        d_x.free()
        d_o.free()


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_parity_host_and_resident(hip, case, dtype):
    """y and the operators of the host form and of the resident form in place, each against the yardstick; the two forms, the
    out-of-place call and a second call give the same bits."""
    snum, tnum, oplen, gap, window = case
    x, (y_hi, a_hi), (y_ref, a_ref) = yardstick(case, dtype)
    y_h, a_h = run_host(x, oplen, gap, window)
    m = last_metrics()
    assert m['entry'] == 'impdar_decon' and 'decon_apply_kernel' in m['kernel']
    assert m['device_ms'] > 0 and all(m[k] >= 0 for k in ('acorr_ms', 'solve_ms', 'apply_ms'))
    assert y_h.dtype == dtype and y_h.shape == (snum, tnum) and a_h.shape == (oplen, tnum)
    held('y %s %s host' % (R.case_id(case), np.dtype(dtype).name), y_h, y_hi, y_ref)
    held('operators %s %s host' % (R.case_id(case), np.dtype(dtype).name), a_h, a_hi, a_ref)
    y_d, a_d = run_dev(x, oplen, gap, window)
    assert np.array_equal(y_d, y_h) and np.array_equal(a_d, a_h)
    y_o, a_o = run_dev(x, oplen, gap, window, in_place=False)
    assert np.array_equal(y_o, y_h) and np.array_equal(a_o, a_h)
    y_2, a_2 = run_host(x, oplen, gap, window)
    assert np.array_equal(y_2, y_h) and np.array_equal(a_2, a_h)


class View(object):
    """A (snum, tnum) array that starts one element into a device allocation: no access wider than an element is aligned."""

    def __init__(self, hip, x):
        flat = np.concatenate([np.zeros(1, dtype=x.dtype), x.ravel(), np.zeros(3, dtype=x.dtype)])
        self.base = hip.DeviceArray.from_host(hip.context(), flat)
        self.ctx, self.shape, self.dtype = self.base.ctx, x.shape, x.dtype
        self.ptr = C.c_void_p(self.base.ptr.value + x.dtype.itemsize)

    def to_host(self):
        return self.base.to_host()[1:1 + self.shape[0] * self.shape[1]].reshape(self.shape)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_misaligned_resident_view(hip, dtype):
    """tnum = 64 takes 16-byte accesses when the array allows them; a view one element in falls back, with the same bits."""
    from impdar_amd import decon
    case = (97, 64, 31, 1, None)
    x, (y_hi, a_hi), (y_ref, a_ref) = yardstick(case, dtype)
    want = run_host(x, 31, 1)
    v = View(hip, x)
    try:
        res, ops = decon.decon_dev(v, decon.check_decon(x.shape, 31, 1), operators=True)
        assert np.array_equal(res.to_host(), want[0]) and np.array_equal(ops, want[1])
        A = decon.acorr_dev(View(hip, x), decon.check_acorr(x.shape, 40))
        assert np.array_equal(A, decon.acorr_host(x, decon.check_acorr(x.shape, 40)))
    finally:
        v.base.free()


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('case', [(97, 64, 31, 1, None), (2 * R.C + 3, 65, 31, R.C + 1, None), (97, 3, 31, 36, (5, 90)), (16, 1, 1, 1, None),
                                  (R.C + 1, 130, 2, 2, (1, R.C + 1))], ids=R.case_id)
def test_autocorrelogram_parity(hip, case, dtype):
    from impdar_amd import decon
    snum, tnum, oplen, gap, window = case
    x = yardstick(case, dtype)[0]
    s0, s1 = R.window_of(snum, window)
    for maxlag in sorted({0, min(oplen + gap, s1 - s0 - 1), s1 - s0 - 1}):
        for normalize in (True, False):
            args = decon.check_acorr(x.shape, maxlag, window)
            A = decon.acorr_host(x, args, normalize)
            assert A.shape == (maxlag + 1, tnum) and A.dtype == np.float64
            held('acorr %s %s maxlag %d norm %d' % (R.case_id(case), np.dtype(dtype).name, maxlag, normalize), A,
                 R.acorr(x, maxlag, window, normalize, 'hi'), R.acorr(x, maxlag, window, normalize, 'ref'))
            d = make(x)
            d.to_device()
            lag_s, A_d = d.autocorrelation(maxlag, window=window, normalize=normalize)
            assert np.array_equal(A_d, A) and np.allclose(lag_s, np.arange(maxlag + 1) * DT)
    m = last_metrics()
    assert m['entry'] == 'impdar_acorr' and m['kernel'] == 'decon_acorr_kernel' and m['acorr_ms'] >= 0


def test_oplen_256_against_the_float64_reference(hip):
    """600 x 5, oplen 256: a longdouble recursion of that length in Python is too slow for the suite, so the bar is the distance
    between the float64 reference and the same reference with its sums taken from the other end, times 8."""
    snum, tnum, oplen, gap, window = R.BIG
    x = (R.ringing(snum, tnum, np.float64, seed=9) + 0.05 * R.noise(snum, tnum, np.float64, seed=10))
    y_ref, a_ref = R.decon(x, oplen, gap, 0.1, window, 'each', 'ref')
    y_rev, a_rev = R.decon(x, oplen, gap, 0.1, window, 'each', 'ref_reversed')
    y, a = run_host(x, oplen, gap)
    for what, got, ref, rev in (('y', y, y_ref, y_rev), ('operators', a, a_ref, a_rev)):
        e_dev, e_ref = R.err(got, ref), R.err(rev, ref)
        print('oplen 256 %s: dev %.3e reversed reference %.3e ratio %.2f' % (what, e_dev, e_ref, e_dev / e_ref))
        assert e_dev <= 8 * e_ref, what
    y_d, a_d = run_dev(x, oplen, gap)
    assert np.array_equal(y_d, y) and np.array_equal(a_d, a)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('tnum', [65, 130])
def test_a_trace_does_not_depend_on_its_neighbours(hip, tnum, dtype):
    """Trace j of a (snum, tnum) call equals the same trace run as (snum, 1), bit for bit: first, a middle and the last group."""
    from impdar_amd import decon
    snum, oplen, gap = 2 * R.C + 3, 31, 5
    x = R.ringing(snum, tnum, dtype, seed=tnum)
    y, a = run_host(x, oplen, gap, window=(3, snum - 2))
    A = decon.acorr_host(x, decon.check_acorr(x.shape, 50))
    for j in (0, 31, 32, tnum // 2, tnum - 2, tnum - 1):
        col = np.ascontiguousarray(x[:, j:j + 1])
        y1, a1 = run_host(col, oplen, gap, window=(3, snum - 2))
        assert np.array_equal(y1[:, 0], y[:, j]) and np.array_equal(a1[:, 0], a[:, j]), j
        assert np.array_equal(decon.acorr_host(col, decon.check_acorr(col.shape, 50))[:, 0], A[:, j]), j


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_dead_and_non_finite_traces(hip, dtype):
    """An all-zero trace, one with a NaN and one with an Inf inside the window, among live neighbours: they pass unchanged with
    zero operators and NaN autocorrelogram columns, and the neighbours do not notice.  A NaN outside the window spreads to the
    samples the reference spreads it to."""
    from impdar_amd import decon
    snum, tnum, oplen, gap, window = 97, 9, 8, 3, (10, 80)
    clean = R.ringing(snum, tnum, dtype, seed=21)
    x = clean.copy()
    x[:, 2] = 0
    x[40, 4] = np.nan
    x[55, 6] = np.inf
    x[3, 7] = np.nan                    # above the window: a live trace
    x[90, 8] = -np.inf                  # below it
    y, a = run_host(x, oplen, gap, window)
    y0, a0 = run_host(clean, oplen, gap, window)
    for j in (2, 4, 6):
        assert np.array_equal(y[:, j], x[:, j], equal_nan=True) and np.all(a[:, j] == 0), j
    for j in (0, 1, 3, 5):
        assert np.array_equal(y[:, j], y0[:, j]) and np.array_equal(a[:, j], a0[:, j]), j
    y_ref, a_ref = R.decon(x, oplen, gap, 0.1, window, 'each', 'ref')
    for j in (7, 8):
        assert np.array_equal(a[:, j], a0[:, j]) and np.any(a[:, j] != 0)
        assert np.array_equal(np.isnan(y[:, j]), np.isnan(y_ref[:, j])) and np.array_equal(np.isinf(y[:, j]), np.isinf(y_ref[:, j])), j
    assert np.isnan(y[3, 7]) and np.all(np.isnan(y[3 + gap:3 + gap + oplen, 7])) and np.sum(np.isnan(y[:, 7])) == 1 + oplen
    A = decon.acorr_host(x, decon.check_acorr(x.shape, 12, window))
    A0 = decon.acorr_host(clean, decon.check_acorr(x.shape, 12, window))
    assert np.all(np.isnan(A[:, [2, 4, 6]])) and np.array_equal(A[:, [0, 1, 3, 5, 7, 8]], A0[:, [0, 1, 3, 5, 7, 8]])
    y_d, a_d = run_dev(x, oplen, gap, window)
    assert np.array_equal(y_d, y, equal_nan=True) and np.array_equal(a_d, a)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('case', [(97, 64, 31, 2, None), (2 * R.C + 3, 65, 8, R.C + 1, (2, 2 * R.C)), (R.C, 3, 2, 7, None)], ids=R.case_id)
def test_design_mean(hip, case, dtype):
    """One operator from the summed lags: held to the yardstick, the same for every trace, unchanged by dead traces appended
    (300 of them: another block of the sum), and with every trace dead the data passes."""
    snum, tnum, oplen, gap, window = case
    x, (y_hi, a_hi), (y_ref, a_ref) = yardstick(case, dtype, 'mean')
    y, a = run_host(x, oplen, gap, window, 'mean')
    assert 'decon_mean_kernel' in last_metrics()['kernel']
    held('mean operators %s %s' % (R.case_id(case), np.dtype(dtype).name), a, a_hi, a_ref)
    held('mean y %s %s' % (R.case_id(case), np.dtype(dtype).name), y, y_hi, y_ref)
    assert np.all(a == a[:, :1]) and np.any(a != 0)
    y_d, a_d = run_dev(x, oplen, gap, window, 'mean')
    assert np.array_equal(y_d, y) and np.array_equal(a_d, a)
    dead = np.zeros((snum, 300), dtype=dtype)
    dead[snum // 2, 1::2] = np.nan
    xx = np.concatenate([x, dead], axis=1)
    yy, aa = run_host(xx, oplen, gap, window, 'mean')
    assert np.array_equal(aa[:, :tnum], a) and np.array_equal(yy[:, :tnum], y)
    assert np.all(aa[:, tnum:] == 0) and np.array_equal(yy[:, tnum:], dead, equal_nan=True)
    yz, az = run_host(dead, oplen, gap, window, 'mean')
    assert np.array_equal(yz, dead, equal_nan=True) and np.all(az == 0)


def band_energy(x, oplen, gap):
    """sum over the traces of sum_{l = gap}^{gap + oplen - 1} (r[l] / r[0])^2, in longdouble."""
    A = R.acorr(x, gap + oplen - 1, kind='hi')
    return float(np.sum(A[gap:] ** 2))


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_effect_on_the_ringing_fixture(hip, dtype):
    """The filter does its job: on the ringing fixture at 256 x 64 the normalised autocorrelation inside the lags gap .. gap +
    oplen - 1 drops by at least half the factor the longdouble restatement achieves."""
    oplen, gap = 24, 2
    x = R.ringing(256, 64, dtype)
    before = band_energy(x, oplen, gap)
    factor_hi = before / band_energy(R.decon(x, oplen, gap, kind='hi')[0], oplen, gap)
    y = run_host(x, oplen, gap)[0]
    factor = before / band_energy(y, oplen, gap)
    print('effect %s: band energy falls by %.1f (longdouble restatement: %.1f)' % (np.dtype(dtype).name, factor, factor_hi))
    assert factor_hi > 4 and factor >= factor_hi / 2


def test_method_on_a_resident_radargram(hip):
    x = R.ringing(97, 64, np.float32, seed=4)
    want, ops = run_host(x, 16, 3, (5, 90))
    d = make(x)
    flags_before = {k: np.array(v, copy=True) for k, v in vars(d.flags).items()}
    d.to_device()
    got_ops = d.decon_operators(16, gap=3, window=(5, 90))
    assert np.array_equal(got_ops, ops) and np.array_equal(d._dev.to_host(), x)          # the data untouched
    d.predictive_decon(16, gap=3, window=(5, 90))
    assert getattr(d, '_dev', None) is not None and np.array_equal(d._dev.to_host(), want)
    d.from_device()
    assert np.array_equal(d.data, want)
    for k, v in flags_before.items():
        assert np.array_equal(np.asarray(getattr(d.flags, k)), v), k
    h = make(x)
    h.predictive_decon(16, gap=3, window=(5, 90))
    assert np.array_equal(h.data, want) and np.array_equal(h.decon_operators(16, gap=3, window=(5, 90)).shape, (16, 64))
    i = make(np.round(x * 100).astype(np.int16))
    i.predictive_decon(4)
    assert i.data.dtype == np.float64


def _line_file(tmp_path, snum, tnum):
    from impdar_amd import synth
    from impdar_amd.lib.NoInitRadarData import NoInitRadarData
    geo = synth.geometry(snum, tnum, dt=DT, dx=1.0)
    d = NoInitRadarData(big=True)
    d.data = R.ringing(snum, tnum, np.float64, seed=8)
    d.snum, d.tnum = snum, tnum
    for k in ('lat', 'long', 'trace_num', 'decday', 'trig', 'pressure'):
        setattr(d, k, np.zeros(tnum))
    d.travel_time, d.dist, d.trace_int, d.dt = geo['travel_time'], geo['dist'], geo['trace_int'], geo['dt']
    fn = str(tmp_path / 'line_raw.mat')
    d.save(fn)
    return d, fn


def test_impproc_decon_end_to_end(hip, tmp_path):
    from impdar_amd.bin import impproc
    from impdar_amd.lib.RadarData import RadarData
    d, fn = _line_file(tmp_path, 96, 20)
    argv = ['impproc', 'decon', '--oplen', '12', '--gap', '3', '--prewhiten', '0.5', '--window', '4', '90', '--design', 'mean', fn]
    with patch.object(sys, 'argv', argv):
        impproc.main()
    out_fn = str(tmp_path / 'line_decon.mat')
    assert os.path.exists(out_fn)
    r = RadarData(out_fn)
    want = make(d.data)
    want.predictive_decon(12, gap=3, prewhiten=0.5, window=(4, 90), design='mean')
    assert np.array_equal(r.data, want.data) and not np.array_equal(r.data, d.data)


def test_impplot_acorr_without_a_display(hip, tmp_path):
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    from impdar_amd.bin import impplot
    from impdar_amd.lib import plot
    d, fn = _line_file(tmp_path, 32, 16)
    try:
        figs = impplot.plot_acorr([fn], maxlag=10, s=True)
        assert len(figs) == 1 and os.path.exists(str(tmp_path / 'line_raw.png'))
        fig, ax = figs[0]
        img = np.asarray(ax.get_images()[0].get_array())
        lag_s, A = make(d.data).autocorrelation(10)
        assert np.array_equal(img, A) and ax.get_xlabel() and ax.get_ylabel()
        fig2, ax2 = plt.subplots()
        assert plot.plot_acorr(make(d.data), fig=fig2, ax=ax2) == (fig2, ax2)
        with patch.object(sys, 'argv', ['impplot', 'acorr', '--maxlag', '5', '-s', fn]):
            impplot.main()
    finally:
        plt.close('all')


def test_refusals_from_python_and_from_the_c_abi(hip):
    """ValueError from Python before any device call; IMPDAR_ERR_ARG from the C ABI with the route header's reason; the output
    is not touched."""
    d = make(R.noise(100, 8, np.float32))
    for kw in (dict(oplen=0), dict(oplen=257), dict(oplen=8, gap=0), dict(oplen=8, window=(0, 101)), dict(oplen=8, gap=3, window=(10, 20)),
               dict(oplen=8, prewhiten=-1.0), dict(oplen=8, design='all')):
        with pytest.raises(ValueError):
            d.predictive_decon(**kw)
    with pytest.raises(ValueError):
        d.autocorrelation(100)
    lib, ctx = hip.load(), hip.context()
    x = R.noise(100, 8, np.float32)
    out = np.full_like(x, 7)
    p, q = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    ok = dict(dtype=0, snum=100, tnum=8, s0=0, s1=100, oplen=8, gap=2, prewhiten=0.1, design=0)
    reasons = [(dict(oplen=0), 'oplen must lie in 1 .. 256'), (dict(oplen=257), 'oplen must lie in 1 .. 256'), (dict(gap=0), 'gap must be at least 1'),
               (dict(s0=-1), 'the window must satisfy'), (dict(s1=101), 'the window must satisfy'), (dict(s0=50, s1=50), 'the window must satisfy'),
               (dict(s0=10, s1=20, gap=3), "gap + oplen must not exceed the window's length"), (dict(prewhiten=-0.5), 'prewhiten must be finite'),
               (dict(prewhiten=float('nan')), 'prewhiten must be finite'), (dict(design=2), 'design must be 0 (each) or 1 (mean)'),
               (dict(dtype=2), 'dtype must be float32 or float64')]
    for change, reason in reasons:
        k = dict(ok, **change)
        for fn in (lib.impdar_decon, lib.impdar_decon_dev):
            rc = fn(ctx, p, k['dtype'], k['snum'], k['tnum'], k['s0'], k['s1'], k['oplen'], k['gap'], k['prewhiten'], k['design'], q, None)
            assert rc == hip.ERR_ARG and reason in hip.last_error(), (change, hip.last_error())
    A = np.full((101, 8), 7.0)
    for fn in (lib.impdar_acorr, lib.impdar_acorr_dev):
        for s0, s1, maxlag, reason in ((0, 100, 100, "maxlag must be below the window's length"), (10, 30, 20, 'maxlag must be below'),
                                       (0, 100, -1, 'maxlag must not be negative'), (0, 101, 5, 'the window must satisfy')):
            rc = fn(ctx, p, 0, 100, 8, s0, s1, maxlag, 1, A.ctypes.data_as(C.POINTER(C.c_double)))
            assert rc == hip.ERR_ARG and reason in hip.last_error(), (s0, s1, maxlag, hip.last_error())
        assert fn(ctx, p, 3, 100, 8, 0, 100, 5, 1, A.ctypes.data_as(C.POINTER(C.c_double))) == hip.ERR_ARG
    assert np.all(out == 7) and np.all(A == 7)
