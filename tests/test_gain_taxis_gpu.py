"""The gains, the trace-axis steps and winavg_hfilt on the MI355X: every ``G*`` / ``R*`` / ``AW*`` fixture of the
reference through the host-buffer path and, for float input, the resident path (equal bit for bit, NaNs included);
rangegain, agc, reverse and hcrop equal to the fixture bit for bit (each is a copy, a maximum or one rounding),
restack and winavg_hfilt within 1e-12 (float64) and 2e-6 (float32 and int16 input) of max|expected|, the bars
``hfilt`` and ``nmo`` are held to; the chain's size, 4096 x {10000, 10001, 10002}, resident, against NumPy
restatements written here at the same bars; and ``impproc hcrop`` -> ``restack`` -> ``vbp`` -> ``agc`` -> ``migrate``
on a .mat file against the same steps on a resident radargram."""
import contextlib
import io
import sys
from unittest.mock import patch

import numpy as np
import pytest

from conftest import golden, rel_max
from test_gain_taxis_cpu import CASES, bar, run_fixture

pytestmark = pytest.mark.gpu

SNUM = 4096
SIZES = [(np.float32, 10000), (np.float64, 10000), (np.float32, 10001), (np.float64, 10001), (np.float32, 10002),
         (np.float64, 10002)]


@pytest.fixture(autouse=True)
def _one_transform_implementation(monkeypatch):
    monkeypatch.setenv('IMPDAR_STOLT_FFT', 'own')


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


@pytest.mark.parametrize('name', CASES)
def test_fixture_host_and_resident(hip, name):
    g = golden(name)
    _, host = run_fixture(g)
    if g['in_data'].dtype in (np.float32, np.float64):
        r, res = run_fixture(g, resident=True)
        r.from_device()
        assert host.dtype == res.dtype and host.shape == res.shape
        np.testing.assert_array_equal(bits(host), bits(res))
        np.testing.assert_array_equal(bits(r.data), bits(res))


# ------------------------------------------------------------------------------------------------ chain size
@pytest.fixture(scope='module')
def big_x():
    return np.random.default_rng(21).standard_normal((SNUM, 10002)).astype(np.float32)


def big_dat(x, dt=1e-8):
    from impdar_amd.lib.RadarData import RadarData
    d = RadarData(None)
    d.data = x
    d.snum, d.tnum = x.shape
    d.dt = dt
    d.travel_time = np.arange(d.snum) * dt * 1e6 + 0.01
    tnum = d.tnum
    for k in ('lat', 'long', 'decday', 'pressure', 'x_coord', 'y_coord', 'elev'):
        setattr(d, k, np.arange(tnum, dtype=float))
    d.dist = np.arange(tnum) * 1e-3
    d.trig = np.zeros(tnum)
    d.trace_num = np.arange(tnum) + 1
    d.trace_int = np.ones(tnum)
    return d


def resident_result(x, step):
    """``step(dat)`` on a resident copy of ``x``; the RadarData after ``from_device``."""
    d = big_dat(x.copy())
    d.to_device()
    quiet(step, d)
    assert d.data is None
    d.from_device()
    return d


def cut(big_x, dtype, tnum):
    return np.ascontiguousarray(big_x[:, :tnum]).astype(dtype)


def within_bar(got, want, dtype, what):
    assert got.dtype == want.dtype and got.shape == want.shape
    err = float(np.max(np.abs(got.astype(np.float64) - want))) / float(np.max(np.abs(want)))
    print('%s: max|diff| / max|expected| = %.3e' % (what, err))
    assert err <= bar(np.dtype(dtype)), err


@pytest.mark.parametrize('dtype,tnum', SIZES)
def test_rangegain_at_chain_size(hip, big_x, dtype, tnum):
    x = cut(big_x, dtype, tnum)
    trig = np.random.default_rng(22).integers(-3, 40, tnum).astype(float)
    d = big_dat(x.copy())
    d.trig = trig
    d.to_device()
    d.rangegain(0.07)
    d.from_device()
    start = np.array([slice(int(t) + 1, None).indices(SNUM)[0] for t in trig])
    g = d.travel_time * 0.07
    want = x.copy()
    for a in range(0, SNUM, 512):                                   # in row blocks: the temporaries stay small
        s = slice(a, a + 512)
        rows = np.arange(a, min(a + 512, SNUM))[:, None] >= start[None, :]
        want[s] = np.where(rows, (x[s].astype(np.float64) * g[s, None]).astype(dtype), x[s])
    assert d.data.dtype == dtype and d.flags.rgain
    np.testing.assert_array_equal(bits(d.data), bits(want))


@pytest.mark.parametrize('window', [50, 1001])
@pytest.mark.parametrize('dtype,tnum', SIZES)
def test_agc_at_chain_size(hip, big_x, dtype, tnum, window):
    x = cut(big_x, dtype, tnum)
    x[2000:2070] = 0.                                               # longer than the short window: maxamp 0 -> 1e-6
    x[100, 77] = np.nan
    x[3000, tnum - 1] = np.nan
    d = resident_result(x, lambda d: d.agc(window=window, scaling_factor=30))
    half = window // 2
    with np.errstate(invalid='ignore'):
        rowmax = np.max(np.abs(x), axis=1).astype(np.float64)
        maxamp = np.array([np.max(rowmax[max(0, i - half):min(i + half, SNUM)]) for i in range(SNUM)])
    assert np.isnan(maxamp).sum() >= 2 * half and (maxamp == 0).any() == (window == 50)
    maxamp[maxamp == 0] = 1.0e-6
    want = x * (30 / maxamp).astype(dtype)[:, None]
    assert d.data.dtype == dtype and d.flags.agc
    np.testing.assert_array_equal(np.isnan(d.data), np.isnan(want))
    np.testing.assert_array_equal(bits(d.data), bits(want))


@pytest.mark.parametrize('dtype,tnum', SIZES)
def test_reverse_and_hcrop_at_chain_size(hip, big_x, dtype, tnum):
    x = cut(big_x, dtype, tnum)
    d = resident_result(x, lambda d: d.reverse())
    assert d.data.dtype == dtype and d.flags.reverse and d.lat[0] == tnum - 1 and d.dist[0] == 0.
    np.testing.assert_array_equal(bits(d.data), bits(x[:, ::-1]))
    d = resident_result(x, lambda d: d.hcrop(1236, 'left', 'tnum'))
    assert d.data.dtype == dtype and d.tnum == tnum - 1235 and d.trace_num[0] == 2 and d.lat[0] == 1235.
    np.testing.assert_array_equal(bits(d.data), bits(x[:, 1235:]))
    d = resident_result(x, lambda d: d.hcrop(8.7645, 'right', 'dist'))
    assert d.data.dtype == dtype and d.tnum == 8765 and d.lat[-1] == 8764.
    np.testing.assert_array_equal(bits(d.data), bits(x[:, :8765]))


@pytest.mark.parametrize('traces', [5, 101])
@pytest.mark.parametrize('dtype,tnum', SIZES)
def test_restack_at_chain_size(hip, big_x, dtype, tnum, traces):
    x = cut(big_x, dtype, tnum)
    d = resident_result(x, lambda d: d.restack(traces))
    n = tnum // traces
    want = x[:, :n * traces].reshape(SNUM, n, traces).mean(axis=2, dtype=np.float64)
    assert d.tnum == n and d.flags.restack and d.lat[0] == (traces - 1) / 2. and len(d.trace_int) == n
    within_bar(d.data, want, dtype, 'restack %d, %s x %d' % (traces, np.dtype(dtype).name, tnum))


@pytest.mark.parametrize('avg_win', [51, 1001])
@pytest.mark.parametrize('dtype,tnum', SIZES)
def test_winavg_at_chain_size(hip, big_x, dtype, tnum, avg_win):
    x = cut(big_x, dtype, tnum)
    d = resident_result(x, lambda d: d.winavg_hfilt(avg_win))
    h = (avg_win - 1) // 2
    i = np.arange(tnum)
    lo, hi = np.maximum(i - h, 0), np.minimum(i + h, tnum)
    p = np.zeros((SNUM, tnum + 1))
    np.cumsum(x, axis=1, dtype=np.float64, out=p[:, 1:])
    m = (p[:, hi] - p[:, lo]) / (hi - lo)
    del p
    m = m.astype(dtype).astype(np.float64)                           # the reference's mean is in the data's dtype
    tt = d.travel_time
    scale = np.exp(-tt * 0.05) / np.exp(-tt[0] * 0.05)
    want = (x.astype(np.float64) - m * scale[:, None])
    del m
    assert d.data.dtype == dtype and list(d.flags.hfilt) == [0, 2]
    within_bar(d.data, want.astype(dtype), dtype, 'winavg %d, %s x %d' % (avg_win, np.dtype(dtype).name, tnum))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('tnum', [66, 67, 68, 1])
def test_every_access_width_of_every_kernel(hip, dtype, tnum):
    """Trace counts with tnum % 4 of 2, 3 and 0, and a single trace, on float32 and float64 input, and a stack
    longer than the restack tile: every instantiation of every kernel, host path against resident path and NumPy."""
    from test_gain_taxis_cpu import np_agc, np_rangegain, np_restack, np_winavg
    from impdar_amd import gain, hfilt as hf
    x = np.random.default_rng(tnum).standard_normal((150, tnum)).astype(dtype)
    ref = big_dat(x)
    g, start = gain.rangegain_tables(ref.travel_time, np.arange(tnum) % 7 - 2., 0.3, 150, tnum)
    lo, hi = hf.winavg_windows(tnum, quiet(hf.winavg_window, 9, tnum))
    steps = [(lambda d: d.reverse(), x[:, ::-1], True),
             (lambda d: d.agc(window=9, scaling_factor=7), np_agc(x, 4, 7), True),
             (lambda d: d.winavg_hfilt(9), np_winavg(x, lo, hi, hf.taper(ref.travel_time)), False)]
    if tnum > 1:
        steps.append((lambda d: d.restack(3), np_restack(x, 3), False))
        steps.append((lambda d: d.hcrop(4), x[:, 3:], True))
    for step, want, exact in steps:
        h = big_dat(x.copy())
        quiet(step, h)
        r = resident_result(x, step)
        np.testing.assert_array_equal(bits(h.data), bits(r.data))
        if exact:
            np.testing.assert_array_equal(bits(r.data), bits(want))
        elif want.size and not np.isnan(want).all():
            within_bar(r.data, want, dtype, 'tnum %d' % tnum)
    h = big_dat(x.copy())
    h.trig = np.arange(tnum) % 7 - 2.
    h.rangegain(0.3)
    np.testing.assert_array_equal(bits(h.data), bits(np_rangegain(x, g, start)))


def test_restack_longer_than_the_tile(hip):
    x = np.random.default_rng(5).standard_normal((7, 3 * 9001 + 5)).astype(np.float32)
    from test_gain_taxis_cpu import np_restack
    for arr in (x, x.astype(np.float64)):
        h = big_dat(arr.copy())
        h.restack(9001)
        r = resident_result(arr, lambda d: d.restack(9001))
        assert h.data.shape == (7, 3)
        np.testing.assert_array_equal(bits(h.data), bits(r.data))
        within_bar(r.data, np_restack(arr, 9001), arr.dtype, 'restack 9001')


def _line_file(tmp_path, snum=160, tnum=93, seed=4):
    from impdar_amd import synth
    from impdar_amd.lib.NoInitRadarData import NoInitRadarData
    geo = synth.geometry(snum, tnum)
    rng = np.random.default_rng(seed)
    d = NoInitRadarData(big=True)
    d.data = synth.noise_radargram(snum, tnum, seed=seed)
    d.snum, d.tnum = snum, tnum
    for k in ('lat', 'long', 'decday', 'pressure', 'x_coord', 'y_coord', 'elev'):
        setattr(d, k, np.cumsum(rng.random(tnum)))
    d.trig = np.zeros(tnum)
    d.trace_num = np.arange(tnum) + 1.
    d.travel_time, d.dt, d.dist, d.trace_int = geo['travel_time'], geo['dt'], geo['dist'], geo['trace_int']
    fn = str(tmp_path / 'line_raw.mat')
    d.save(fn)
    return fn


def test_impproc_chain_on_mat_file_equals_the_resident_chain(hip, tmp_path):
    """`impproc hcrop left tnum 12`, `restack 3`, `vbp 2 12`, `agc -window 20`, `migrate --mtype stolt` on files (every
    step through host buffers) = the same five methods on one resident radargram: bit for bit up to the migration,
    within 1e-12 after it (the bar a resident Stolt chain is held to)."""
    from impdar_amd.bin import impproc
    from impdar_amd.lib.RadarData import RadarData
    fn = _line_file(tmp_path)
    names = ['line_hcropped', 'line_hcropped_restacked', 'line_hcropped_restacked_bandpassed',
             'line_hcropped_restacked_bandpassed_agc', 'line_hcropped_restacked_bandpassed_agc_migrated']
    argvs = [['hcrop', 'left', 'tnum', '12'], ['restack', '3'], ['vbp', '2', '12'], ['agc', '-window', '20'],
             ['migrate', '--mtype', 'stolt']]
    src = fn
    for argv, name in zip(argvs, names):
        with patch.object(sys, 'argv', ['impproc'] + argv + [src]):
            quiet(impproc.main)
        src = str(tmp_path / (name + '.mat'))
    before = RadarData(str(tmp_path / (names[3] + '.mat')))
    r = RadarData(src)
    m = RadarData(fn)
    m.to_device()
    quiet(m.hcrop, 12.0, left_or_right='left', dimension='tnum')
    quiet(m.restack, 3)
    quiet(m.vertical_band_pass, 2., 12.)
    quiet(m.agc, window=20, scaling_factor=50)
    assert m.data is None
    np.testing.assert_array_equal(bits(m._dev.to_host()), bits(before.data))
    quiet(m.migrate, 'stolt', vel=1.69e8, vtaper=1000, htaper=100, tmig=0, verbose=1, vel_fn=None, nxpad=100, nearfield=False)
    m.from_device()
    assert r.data.shape == m.data.shape and r.tnum == m.tnum == (93 - 11) // 3
    assert rel_max(r.data, m.data) < 1e-12
    for k in ('dist', 'lat', 'long', 'elev', 'trig', 'trace_num', 'trace_int', 'decday'):
        np.testing.assert_array_equal(np.asarray(getattr(r, k), dtype=float), np.asarray(getattr(m, k), dtype=float), err_msg=k)
    assert r.flags.restack and r.flags.agc and r.flags.mig == 'stolt' and list(r.flags.bpass) == [1., 2., 12.]
