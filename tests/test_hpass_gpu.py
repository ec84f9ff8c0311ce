"""Horizontal frequency filters on the MI355X: every ``W*`` fixture of the reference through the host-buffer and
the resident paths within 1e-12 of max|expected| (the bar that rules out chunked or second-order-section
shortcuts on the narrow and low-corner designs), the chain's size against ``scipy.signal.filtfilt`` on sampled
rows, NaN confinement, row counts that are not a multiple of the rows per wavefront, the resident chain
vbp -> constant_space -> hbp -> stolt against the host chain bit for bit, and ``impproc hbp / lp`` on .mat files."""
import contextlib
import io
import sys
from unittest.mock import patch

import numpy as np
import pytest

from conftest import golden, rel_max
from test_hpass_cpu import CASES, dat_of

pytestmark = pytest.mark.gpu


def run(d, g):
    with contextlib.redirect_stdout(io.StringIO()):
        getattr(d, g['method'].item())(*[float(v) for v in g['args']])


@pytest.mark.parametrize('name', CASES)
def test_fixture_host_and_resident(hip, name):
    g = golden(name)
    d = dat_of(g)
    run(d, g)
    assert d.data.dtype == np.float64
    assert rel_max(d.data, g['out']) <= 1e-12, (name, rel_max(d.data, g['out']))
    np.testing.assert_array_equal(d.flags.hfilt, [1., 3.])
    r = dat_of(g)
    if r.data.dtype not in (np.float32, np.float64):
        r.data = r.data.astype(np.float64)     # residency holds float32 / float64
    r.to_device()
    run(r, g)
    r.from_device()
    assert r.data.dtype == np.float64
    np.testing.assert_array_equal(r.data.view(np.uint64), d.data.view(np.uint64))


def _filtfilt_rows(x, spec, rows):
    from scipy.signal import filtfilt
    b, a, _ = spec
    return filtfilt(b, a, x[rows], axis=1)


def test_chain_size_sampled_rows_and_nan_confinement(hip):
    from impdar_amd import hpass as hp
    snum, tnum = 4096, 10000
    x = np.random.default_rng(21).standard_normal((snum, tnum))
    x += np.sin(2 * np.pi * np.arange(tnum) / 60.0)[None, :]
    with contextlib.redirect_stdout(io.StringIO()):
        spec = hp.band_pass_design(5., 100., 1.0, tnum)
    got = hp.filtfilt_host(x, spec)
    assert got.dtype == np.float64
    rows = np.sort(np.random.default_rng(22).choice(snum, 64, replace=False))
    want = _filtfilt_rows(x, spec, rows)
    assert rel_max(got[rows], want) <= 1e-12
    y = x.copy()
    y[1234, 5000] = np.nan
    got_nan = hp.filtfilt_host(y, spec)
    assert np.isnan(got_nan[1234]).all()                 # as SciPy: the whole row
    others = np.ones(snum, dtype=bool)
    others[1234] = False
    np.testing.assert_array_equal(got_nan[others].view(np.uint64), got[others].view(np.uint64))
    # resident float32 becomes resident float64, and equals the host result of the same float32 input
    from impdar_amd import _hip
    xf = x[:1000].astype(np.float32)
    d_x = _hip.DeviceArray.from_host(_hip.context(), xf)
    d_y = hp.filtfilt_dev(d_x, spec)
    assert d_y is not d_x and d_y.dtype == np.float64
    d_x.free()
    r = d_y.to_host()
    d_y.free()
    np.testing.assert_array_equal(r.view(np.uint64), hp.filtfilt_host(xf, spec).view(np.uint64))


@pytest.mark.parametrize('snum', [1, 17, 4099])
def test_row_counts(hip, snum):
    from impdar_amd import hpass as hp
    tnum = 257
    x = np.random.default_rng(snum).standard_normal((snum, tnum)).astype(np.float32)
    with contextlib.redirect_stdout(io.StringIO()):
        specs = [hp.band_pass_design(5., 100., 1.0, tnum), hp.pass_design('low', 20., 1.0, tnum, 1e-8),
                 hp.pass_design('high', 20., 1.0, tnum, 1e-8)]
    for spec in specs:
        got = hp.filtfilt_host(x, spec)
        rows = np.arange(snum) if snum < 64 else np.r_[0:8, snum - 8:snum]
        assert rel_max(got[rows], _filtfilt_rows(x, spec, rows)) <= 1e-12


def _chain_dat(x, dist):
    from impdar_amd.lib.NoInitRadarData import NoInitRadarDataFiltering
    snum, tnum = x.shape
    d = NoInitRadarDataFiltering()
    d.data, (d.snum, d.tnum) = x.copy(), x.shape
    d.dt, d.dist = 1e-8, dist.copy()
    d.travel_time = np.arange(snum) * 1e-2
    for a in ['lat', 'long', 'x_coord', 'y_coord', 'decday', 'pressure', 'elev']:
        setattr(d, a, np.arange(tnum, dtype=float))
    d.trig = np.zeros(tnum)
    return d


def test_resident_chain_equals_host_chain(hip, monkeypatch):
    monkeypatch.setenv('IMPDAR_STOLT_FFT', 'own')           # one transform implementation for both runs
    rng = np.random.default_rng(31)
    snum, tnum = 512, 900
    x = rng.standard_normal((snum, tnum)).astype(np.float32)
    dist = np.hstack(([0.], np.cumsum(0.6 + 0.8 * rng.random(tnum - 1)))) / 1000.
    outs = []
    for resident in (False, True):
        d = _chain_dat(x, dist)
        with contextlib.redirect_stdout(io.StringIO()):
            if resident:
                d.to_device()
            d.vertical_band_pass(2., 10.)
            d.constant_space(1.0)
            d.horizontal_band_pass(5., 100.)
            if resident:
                assert d.data is None and d._dev.dtype == np.float64
            d.migrate('stolt', htaper=100, vtaper=1000)
            if resident:
                d.from_device()
        np.testing.assert_array_equal(d.flags.hfilt, [1., 3.])
        outs.append(d.data)
    np.testing.assert_array_equal(outs[1].view(np.uint64), outs[0].view(np.uint64))


def _spaced_line_file(tmp_path):
    from impdar_amd.lib.NoInitRadarData import NoInitRadarDataFiltering
    rng = np.random.default_rng(8)
    snum, tnum = 60, 400
    d = NoInitRadarDataFiltering()
    d.data = rng.standard_normal((snum, tnum))
    d.snum, d.tnum = snum, tnum
    d.dt = 1e-8
    d.travel_time = np.arange(snum) * 1e-2
    d.flags.interp = np.array([1.0, 1.0])
    fn = str(tmp_path / 'line_raw.mat')
    d.save(fn)
    return fn


def test_impproc_hbp_and_lp_on_mat_file(hip, tmp_path):
    from impdar_amd.lib.RadarData import RadarData
    from impdar_amd.bin import impproc
    fn = _spaced_line_file(tmp_path)
    for argv, out, call in ((['hbp', '5', '100', fn], 'line_hbp.mat', ('horizontal_band_pass', (5., 100.))),
                            (['lp', '20', fn], 'line_lp.mat', ('lowpass', (20.,)))):
        with patch.object(sys, 'argv', ['impproc'] + argv), contextlib.redirect_stdout(io.StringIO()):
            impproc.main()
        r = RadarData(str(tmp_path / out))
        want = RadarData(fn)
        with contextlib.redirect_stdout(io.StringIO()):
            getattr(want, call[0])(*call[1])
        np.testing.assert_array_equal(r.data, want.data)
        np.testing.assert_array_equal(np.ravel(r.flags.hfilt), [1., 3.])


def test_reference_mat_round_trip(hip, tmp_path):
    """What the reference does with constant spacing -> save -> load -> horizontal_band_pass, here."""
    from impdar_amd.lib.NoInitRadarData import NoInitRadarDataFiltering
    from impdar_amd.lib.RadarData import RadarData
    m = golden('WM_mat_round_trip')
    d = NoInitRadarDataFiltering()
    d.data = np.array(m['spaced'], copy=True)
    d.snum, d.tnum = d.data.shape
    d.dt = 1e-8
    d.travel_time = np.arange(d.snum) * 0.01
    d.flags.interp = np.array(m['interp'], copy=True)
    for attr in ('trace_num', 'trace_int', 'long', 'lat', 'x_coord', 'y_coord', 'decday', 'elev', 'trig', 'pressure'):
        setattr(d, attr, getattr(d, attr)[:d.tnum])
    fn = str(tmp_path / 'spaced.mat')
    d.save(fn)
    e = RadarData(fn)
    np.testing.assert_array_equal(np.asarray(e.flags.interp, dtype=np.float64), m['loaded_interp'])
    assert bool(m['ok'])
    with contextlib.redirect_stdout(io.StringIO()):
        e.horizontal_band_pass(float(m['low']), float(m['high']))
    assert rel_max(e.data, m['out']) <= 1e-12
