"""Spectra without a GPU: the restated periodogram of tests/spectra_ref.py (what the FS* fixtures' expected values were
formed with, in longdouble) against scipy.signal.periodogram on every fixture, the argument errors of
impdar_amd/spectra.py -- raised before any device call -- and the C declarations."""
import os
import re

import numpy as np
import pytest
import scipy.signal

import spectra_ref as sr
from conftest import GOLDEN, ROOT

NAMES = sr.fixture_names(GOLDEN)


def test_all_fixtures_are_present():
    assert len(NAMES) == 27
    kinds = [n.rsplit('_', 1)[1] for n in NAMES]
    assert kinds.count('flat') == 13 and kinds.count('peaked') == 13 and kinds.count('nan') == 1
    for n in NAMES:
        g = sr.load_fixture(GOLDEN, n)
        snum, tnum = g['data'].shape
        assert g['data'].dtype == np.float32
        assert g['ft_hi'].shape == (snum,) and g['hft_hi'].shape == (tnum,)
        for i in range(3):
            assert g['pg%d_hi' % i].shape == (snum // 2 + 1, tnum) and g['Y_pg%d' % i].shape == (tnum,)
    for path in os.listdir(GOLDEN):
        if path.startswith('FS'):
            assert os.path.getsize(os.path.join(GOLDEN, path)) < 1000 * 1024, path


@pytest.mark.parametrize('name', NAMES)
def test_restated_periodogram_is_scipys(name):
    """In float64 the restatement and SciPy's own routine, trace by trace as the reference calls it, agree within a
    quarter of the yardstick (they are the same operations; SciPy detrends and windows through other functions)."""
    g = sr.load_fixture(GOLDEN, name)
    data = g['data'].astype(np.float64)
    for i, (win, scaling) in enumerate(sr.PARAMS):
        with np.errstate(all='ignore'):
            mine = sr.periodogram(data, 1.0 / sr.DT, win, scaling)
            theirs = scipy.signal.periodogram(data, fs=1.0 / sr.DT, window=win, scaling=scaling, axis=0)[1]
            first = scipy.signal.periodogram(data[:, 0], fs=1.0 / sr.DT, window=win, scaling=scaling)[1]
            assert np.array_equal(theirs[:, 0], first, equal_nan=True)       # (the reference calls it trace by trace)
            freq = scipy.signal.periodogram(data[:, 0], fs=1.0 / sr.DT, window=win, scaling=scaling)[0]
        assert np.array_equal(np.isnan(mine), np.isnan(theirs))
        Y = sr.yardstick_periodogram(data, 1.0 / sr.DT, win, scaling)
        ok = np.isfinite(theirs)
        assert np.all((np.abs(mine - theirs) <= 0.25 * Y)[ok]), (name, i)
        assert np.array_equal(freq, np.fft.rfftfreq(data.shape[0], 1.0 / (1.0 / sr.DT)))
        # ... and the stored expected value is that quantity: inside the reference's own recorded distance
        assert np.all((np.abs(theirs - g['pg%d_hi' % i]) <= g['rho64_pg%d' % i] * (1 + 1e-12) + 1e-300)[ok])


@pytest.mark.parametrize('name', NAMES)
def test_bar_resolves_single_bins(name):
    """On the flat cases at least 99 % of the expected bins lie above 4 C Y: a wrong bin, a missed doubling or a
    mis-reversed index cannot hide under the bar (the periodogram's bin 0 is zero by construction: the detrend)."""
    g = sr.load_fixture(GOLDEN, name)
    if str(g['kind']) != 'flat':
        return
    for q in ('ft', 'hft', 'pg0', 'pg1', 'pg2'):
        bins = g[q + '_hi'][1:] if q.startswith('pg') else g[q + '_hi']
        if bins.size:
            assert np.mean(bins > 4 * sr.C * g['Y_' + q]) >= 0.99, (name, q)


def test_yardsticks_match_the_fixtures():
    g = sr.load_fixture(GOLDEN, 'FS03_36x7_flat')
    data = g['data'].astype(np.float64)
    assert np.isclose(sr.yardstick_mean(data, 0), g['Y_ft'], rtol=1e-13) and np.isclose(sr.yardstick_mean(data, 1), g['Y_hft'], rtol=1e-13)
    assert np.allclose(sr.yardstick_periodogram(data, 1.0 / sr.DT, 'hamming', 'density'), g['Y_pg1'], rtol=1e-13)
    # the constant is 8 x the reference's largest own distance, and no fixture's is larger
    worst = max(float(np.max(sr.load_fixture(GOLDEN, n)['rho64_' + q] / np.min(sr.load_fixture(GOLDEN, n)['Y_' + q])))
                for n in NAMES if not n.endswith('nan') for q in ('ft', 'hft'))
    assert 8 * worst <= sr.C <= 8 * worst * 1.25 + 0.5


def test_argument_errors_come_before_any_device_call(monkeypatch):
    from impdar_amd import _hip, spectra

    def no_device(*a, **k):
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_hip, 'load', no_device)
    monkeypatch.setattr(_hip, 'context', no_device)
    data = np.zeros((12, 3), dtype=np.float32)
    with pytest.raises(ValueError, match="Unknown scaling: 'power'"):
        spectra.periodogram_host(data, 1.0e8, scaling='power')
    with pytest.raises(ValueError, match='window has length 11'):
        spectra.periodogram_host(data, 1.0e8, window=np.ones(11))
    with pytest.raises(ValueError, match='Unknown window type'):
        spectra.periodogram_host(data, 1.0e8, window='no_such_window')
    with pytest.raises(ValueError, match='axis'):
        spectra.mean_spectrum_host(data, 2)
    with pytest.raises(TypeError, match='complex'):
        spectra.mean_spectrum_host(data.astype(np.complex64), 0)
    with pytest.raises(TypeError, match='complex'):
        spectra.periodogram_host(data.astype(np.complex128), 1.0e8)
    with pytest.raises(ValueError, match='must be positive'):
        spectra.periodogram_host(data, 0.0)


def test_window_and_scale_are_scipys():
    from impdar_amd import spectra
    for win, scaling in sr.PARAMS + (('hann', 'density'), (('kaiser', 4.0), 'spectrum')):
        w, scale = spectra.window_and_scale(36, 1.0e8, win, scaling)
        ref = scipy.signal.get_window(win or 'boxcar', 36)
        assert (w is None and win is None) or np.array_equal(w, ref)
        assert scale == sr.scale_of(ref, 1.0e8, scaling)
    w, scale = spectra.window_and_scale(5, 2.0, np.arange(1.0, 6.0), 'density')
    assert np.array_equal(w, np.arange(1.0, 6.0)) and scale == 1.0 / (2.0 * 55.0)


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, 'include', 'impdar_hip.h')).read()
    for name in ('impdar_mean_spectrum', 'impdar_mean_spectrum_dev', 'impdar_periodogram', 'impdar_periodogram_dev',
                 'impdar_spec_route_probe'):
        assert re.search(r'\bint %s\(' % name, text), name
    from impdar_amd import _hip
    assert 'impdar_periodogram_dev' in _hip.SIGNATURES and 'impdar_spec_route_probe' in _hip.SIGNATURES


def test_radardata_has_the_methods_and_import_stays_light():
    import subprocess
    import sys
    code = ('import sys, impdar_amd, impdar_amd.lib.plot, impdar_amd.lib.RadarData as R; '
            'assert all(hasattr(R.RadarData, m) for m in ("vertical_spectrum", "horizontal_spectrum", "spectrogram")); '
            'assert "matplotlib" not in sys.modules')
    subprocess.check_call([sys.executable, '-c', code], cwd=ROOT)
