"""Complex-trace attributes on the GPU (csrc/attr.hip), held to the yardstick of tests/attr_ref.py: 8 x the distance of
``ref`` (scipy.signal.hilbert and NumPy on the data's own dtype) from ``hi`` (the contract in longdouble), per array, with the
phase and frequency bars weighted by the envelope (attr_ref's docstring).  The shapes (attr_ref.CASES) are the smallest that
reach every path: the degenerate lengths, every reason for the rocFFT route, the smallest own transform of either kind, every
workgroup size of the row kernel, the LDS limit and the length just past it, and more traces than workgroups.

Largest ratios seen on an MI355X: see DESIGN.md 4.21.
"""
import ctypes as C
import functools
import os
import sys
from unittest.mock import patch

import numpy as np
import pytest

import attr_ref as R
from stolt_route_cases import last_metrics

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
DTYPE_IDS = ['f32', 'f64']
ALL_CASES = R.CASES + [(32, 2101, R.OWN_POW2, 64)]          # (32 x 2100 divides evenly: this one has the short last block)


def make(data, dt=R.DT):
    from impdar_amd import synth
    from impdar_amd.lib.RadarData import RadarData
    snum, tnum = data.shape
    geo = synth.geometry(snum, max(tnum, 2), dt=dt, dx=1.0)
    d = RadarData(None)
    d.data, d.snum, d.tnum = data.copy(), snum, tnum
    d.travel_time, d.dist, d.trace_int, d.dt = geo['travel_time'][:snum], geo['dist'][:tnum], geo['trace_int'][:tnum], dt
    d.fn = ''
    return d


@functools.lru_cache(maxsize=None)
def yardstick(n, tnum, dtype, name='rickers'):
    """(x, Yard) of a shape: computed once and never written to."""
    x = R.fixture(n, tnum, dtype, name)
    return x, R.Yard(x)


def run_host(x, kind, smooth=1, dt=R.DT):
    from impdar_amd import attributes as A
    return A.attr_host(x, A.check_attr(x.shape, kind, smooth, dt))


def run_dev(x, kind, smooth=1, dt=R.DT, in_place=True):
    from impdar_amd import _hip, attributes as A
    args = A.check_attr(x.shape, kind, smooth, dt)
    d_x = _hip.DeviceArray.from_host(_hip.context(), x)
    d_o = d_x if in_place else _hip.DeviceArray(_hip.context(), x.shape, x.dtype)
    try:
        y = A.attr_dev(d_x, args, out=None if in_place else d_o).to_host()
        if not in_place:
            assert np.array_equal(d_x.to_host(), x, equal_nan=True)
        return y
    finally:
        d_x.free()
        d_o.free()


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('case', ALL_CASES, ids=R.case_id)
def test_parity_host_and_resident(hip, case, dtype):
    """Every kind through the host form against the yardstick; the resident form in place and out of place and a second call
    give the same bits; the route is the one the case is there for."""
    n, tnum, route, threads = case
    x, Y = yardstick(n, tnum, dtype)
    for kind in R.KINDS:
        y = run_host(x, kind)
        m = last_metrics()
        assert m['entry'] == 'impdar_attr' and m['device_ms'] > 0
        assert ('attr_rows_kernel' in m['kernel']) == (route != R.ROCFFT) and ('mixed' in m['kernel']) == (route == R.OWN_MIXED)
        assert y.dtype == dtype and y.shape == (n, tnum)
        R.held('%s %s %s host' % (kind, R.case_id(case), np.dtype(dtype).name), Y, y, R.attr_ref(x, kind), kind)
        assert np.array_equal(run_dev(x, kind), y)
        assert np.array_equal(run_dev(x, kind, in_place=False), y)
        assert np.array_equal(run_host(x, kind), y)
    if n <= 2:
        assert np.all(run_host(x, 'quadrature') == 0)
    if n == 1:
        assert np.all(run_host(x, 'frequency') == 0)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('case', [(60, 31), (300, 5), (2048, 3)], ids=lambda c: '%dx%d' % c)
def test_chirp(hip, case, dtype):
    """The second fixture, and what the attributes are for: away from the ends the envelope of a unit sweep is 1 and its
    instantaneous frequency follows the sweep."""
    n, tnum = case
    x, Y = yardstick(n, tnum, dtype, 'chirp')
    for kind in R.KINDS:
        R.held('%s chirp %dx%d %s' % (kind, n, tnum, np.dtype(dtype).name), Y, run_host(x, kind), R.attr_ref(x, kind), kind)
    if n >= 2048:
        e, f = run_host(x, 'envelope'), run_host(x, 'frequency') * R.DT
        mid = slice(n // 8, n - n // 8)
        assert np.max(np.abs(e[mid] - 1)) < 0.05
        assert np.all(np.diff(f[mid][::64], axis=0) > 0) and 0.02 < f[mid].min() < 0.05 and 0.12 < f[mid].max() < 0.16


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('smooth', R.SMOOTHS)
@pytest.mark.parametrize('shape', R.SMOOTH_CASES, ids=lambda s: '%dx%d' % s)
def test_smoothed_frequency(hip, shape, smooth, dtype):
    """A window shorter than the trace and one longer than it (255 on 60 samples), on the own-transform route (60, 300) and, with
    the same yardstick, on the rocFFT route (the same traces cut to 59 and 299 samples are another radargram: its own bars)."""
    n, tnum = shape
    for nn in (n, n - 1):
        x, Y = yardstick(nn, tnum, dtype)
        y = run_host(x, 'frequency', smooth)
        assert ('attr_rows_kernel' in last_metrics()['kernel']) == (nn == n)
        R.held('frequency W %d %dx%d %s' % (smooth, nn, tnum, np.dtype(dtype).name), Y, y, R.attr_ref(x, 'frequency', smooth), 'frequency', smooth)
        assert np.array_equal(run_dev(x, 'frequency', smooth), y) and np.array_equal(run_dev(x, 'frequency', smooth, in_place=False), y)
        assert np.array_equal(run_host(x, 'frequency', smooth), y)
        if smooth == 1:
            assert np.array_equal(y, run_host(x, 'frequency'))


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('n', [60, 59], ids=['own', 'rocfft'])
def test_non_finite_and_zero_traces(hip, n, dtype):
    """A NaN and an Inf in two traces of 60 x 31 and an all-zero trace, among live neighbours: NaN and zero columns, exactly,
    in every kind and with a window, and the neighbours do not notice."""
    clean = yardstick(n, 31, dtype)[0]
    x = clean.copy()
    x[17, 3] = np.nan
    x[n - 1, 29] = -np.inf
    x[:, 11] = 0
    live = [j for j in range(31) if j not in (3, 29, 11)]
    for kind, smooth in [(k, 1) for k in R.KINDS] + [('frequency', 9)]:
        y, y0 = run_host(x, kind, smooth), run_host(clean, kind, smooth)
        assert np.all(np.isnan(y[:, [3, 29]])) and np.all(y[:, 11] == 0), (kind, smooth)
        assert np.array_equal(y[:, live], y0[:, live]), (kind, smooth)
        assert np.array_equal(run_dev(x, kind, smooth), y, equal_nan=True)
        assert np.array_equal(np.isnan(y), np.isnan(R.attr_hi(x, kind, smooth)))
    zeros = np.zeros((n, 4), dtype=dtype)
    for kind in R.KINDS:
        assert np.array_equal(run_host(zeros, kind), zeros)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('case', [c for c in R.CASES if c[2] != R.ROCFFT and c[1] <= 65], ids=R.case_id)
def test_a_trace_does_not_depend_on_its_neighbours(hip, case, dtype):
    """On the own-transform routes a trace run alone (tnum = 1) gives the bits it has inside the radargram."""
    n, tnum = case[:2]
    x = yardstick(n, tnum, dtype)[0]
    for kind, smooth in (('envelope', 1), ('phase', 1), ('frequency', 1), ('frequency', 9)):
        y = run_host(x, kind, smooth)
        for j in sorted({0, tnum // 2, tnum - 1}):
            col = np.ascontiguousarray(x[:, j:j + 1])
            assert np.array_equal(run_host(col, kind, smooth)[:, 0], y[:, j]), (kind, smooth, j)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_methods_and_analytic_signal(hip, dtype):
    x = yardstick(126, 65, dtype)[0]
    want = {k: run_host(x, k) for k in R.KINDS}
    want9 = run_host(x, 'frequency', 9)
    for resident in (False, True):
        d = make(x)
        flags_before = {k: np.array(v, copy=True) for k, v in vars(d.flags).items()}
        if resident:
            d.to_device()
        z = d.analytic_signal()
        assert z.dtype == (np.complex64 if dtype == np.float32 else np.complex128)
        assert np.array_equal(z.real, x) and np.array_equal(z.imag, want['quadrature'])        # the real part is the data bit for bit
        for k in R.KINDS:
            assert np.array_equal(d.complex_attribute(k), want[k])
        assert np.array_equal(d.complex_attribute('frequency', smooth=9), want9)
        assert np.array_equal(d._dev.to_host() if resident else d.data, x)                     # the data untouched
        for method, kw, res in (('envelope', {}, want['envelope']), ('instantaneous_phase', {}, want['phase']),
                                ('instantaneous_frequency', {}, want['frequency']), ('instantaneous_frequency', dict(smooth=9), want9)):
            e = make(x)
            if resident:
                e.to_device()
            getattr(e, method)(**kw)
            assert (getattr(e, '_dev', None) is not None) == resident
            e.from_device()
            assert np.array_equal(e.data, res) and e.data.dtype == dtype, method
        for k, v in flags_before.items():
            assert np.array_equal(np.asarray(getattr(d.flags, k)), v), k
    i = make(np.round(x * 100).astype(np.int16))
    i.envelope()
    assert i.data.dtype == np.float64 and np.array_equal(i.data, run_host(np.round(x * 100).astype(np.float64), 'envelope'))
    c = make(x)
    c.data = c.data.astype(np.complex64)
    with pytest.raises(TypeError):
        c.envelope()


def test_resident_envelope_between_band_pass_and_stolt(hip, monkeypatch):
    """vertical_band_pass -> envelope -> migrate('stolt') on a resident radargram equals the same three steps through host arrays,
    and the radargram stays in HBM from the first to the last (the host array is absent throughout; the metrics line after
    the envelope is impdar_attr's own, after the migration Stolt's: nothing ran in between)."""
    monkeypatch.setenv('IMPDAR_STOLT_FFT', 'own')           # one transform implementation for both runs
    x = yardstick(126, 65, np.float32)[0]
    h = make(x, dt=1.0e-8)
    h.vertical_band_pass(2., 12.)
    h.envelope()
    h.migrate(mtype='stolt')
    d = make(x, dt=1.0e-8)
    d.to_device()
    d.vertical_band_pass(2., 12.)
    assert d.data is None and d._dev is not None
    d.envelope()
    assert d.data is None and d._dev is not None and last_metrics()['entry'] == 'impdar_attr'
    d.migrate(mtype='stolt')
    assert d.data is None and d._dev is not None and 'stolt' in last_metrics()['entry']
    d.from_device()
    assert d.data.shape == h.data.shape and np.array_equal(d.data, np.asarray(h.data, dtype=d.data.dtype))


def _line_file(tmp_path, snum, tnum):
    from impdar_amd import synth
    from impdar_amd.lib.NoInitRadarData import NoInitRadarData
    geo = synth.geometry(snum, tnum, dt=R.DT, dx=1.0)
    d = NoInitRadarData(big=True)
    d.data = np.array(R.fixture(snum, tnum, np.float64))
    d.snum, d.tnum = snum, tnum
    for k in ('lat', 'long', 'trace_num', 'decday', 'trig', 'pressure'):
        setattr(d, k, np.zeros(tnum))
    d.travel_time, d.dist, d.trace_int, d.dt = geo['travel_time'], geo['dist'], geo['trace_int'], geo['dt']
    fn = str(tmp_path / 'line_raw.mat')
    d.save(fn)
    return d, fn


def test_impproc_attr_end_to_end(hip, tmp_path):
    from impdar_amd.bin import impproc
    from impdar_amd.lib.RadarData import RadarData
    d, fn = _line_file(tmp_path, 96, 20)
    for argv, suffix, kind, smooth in ((['--kind', 'envelope'], 'env', 'envelope', 1), (['--kind', 'phase'], 'phase', 'phase', 1),
                                       (['--kind', 'frequency', '--smooth', '9'], 'ifreq', 'frequency', 9)):
        with patch.object(sys, 'argv', ['impproc', 'attr'] + argv + [fn]):
            impproc.main()
        out_fn = str(tmp_path / ('line_%s.mat' % suffix))
        assert os.path.exists(out_fn), suffix
        r = RadarData(out_fn)
        assert np.array_equal(r.data, run_host(d.data, kind, smooth, dt=float(r.dt))) and not np.array_equal(r.data, d.data)


def test_refusals_from_python_and_from_the_c_abi(hip):
    """ValueError from Python before any device call; IMPDAR_ERR_ARG from both C entries with the route header's reason; the
    output is not touched."""
    d = make(np.array(R.fixture(100, 8, np.float32)))
    for call in (lambda: d.instantaneous_frequency(smooth=2), lambda: d.instantaneous_frequency(smooth=257),
                 lambda: d.complex_attribute('envelope', smooth=3), lambda: d.complex_attribute('power')):
        with pytest.raises(ValueError):
            call()
    lib, ctx = hip.load(), hip.context()
    x = np.array(R.fixture(100, 8, np.float32))
    out = np.full_like(x, 7)
    p, q = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    ok = dict(dtype=0, snum=100, tnum=8, kind=3, smooth=1, dt=1.0e-9)
    reasons = [(dict(kind=4), 'kind must be 0 (quadrature), 1 (envelope), 2 (phase) or 3 (frequency)'), (dict(kind=-1), 'kind must be 0'),
               (dict(smooth=2), 'smooth must be odd and lie in 1 .. 255'), (dict(smooth=0), 'smooth must be odd'), (dict(smooth=257), 'smooth must be odd'),
               (dict(kind=1, smooth=3), 'smooth above 1 goes with kind 3 (frequency) alone'), (dict(dt=0.0), 'dt must be finite and positive'),
               (dict(dt=float('nan')), 'dt must be finite and positive'), (dict(dt=float('inf')), 'dt must be finite and positive'),
               (dict(snum=0), 'empty radargram'), (dict(tnum=0), 'empty radargram'), (dict(dtype=2), 'dtype must be float32 or float64')]
    for change, reason in reasons:
        k = dict(ok, **change)
        for fn in (lib.impdar_attr, lib.impdar_attr_dev):
            rc = fn(ctx, p, k['dtype'], k['snum'], k['tnum'], k['kind'], k['smooth'], k['dt'], q)
            assert rc == hip.ERR_ARG and reason in hip.last_error(), (change, hip.last_error())
    assert np.all(out == 7)
