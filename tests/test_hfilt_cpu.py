"""Horizontal filters without a GPU: the adaptive filter's window table against Python's own slicing, the
closed form the kernels implement (windowed means, then the 7-tap stencil [1,2,3,4,3,2,1]/16 on the odd
extension) against every ``H*`` fixture of the reference, and the plumbing of ``RadarData.hfilt``,
``process(ahfilt=...)``, ``impdar proc -ahfilt`` and ``impproc hfilt / ahfilt`` with the device calls mocked."""
import sys
import warnings
from unittest.mock import MagicMock, patch

import numpy as np
import pytest

from conftest import golden, golden_names
from impdar_amd import hfilt as hf
from impdar_amd.bin import impdarexec, impproc
from impdar_amd.lib import process
from impdar_amd.lib.RadarData import RadarData


def closed_form(data, travel_time, kind, bounds, window):
    """fp64 restatement of what the kernels compute, cast as the reference casts."""
    x = np.asarray(data)
    snum, tnum = x.shape
    scale = hf.taper(travel_time)
    if kind == 'hfilt':
        a, b = hf.hfilt_bounds(bounds[0], bounds[1], tnum)
        m = x[:, a:b].astype(np.float64).mean(axis=1)
        if x.dtype == np.float32:
            m = m.astype(np.float32).astype(np.float64)
        if np.issubdtype(x.dtype, np.integer):
            return (x.astype(np.float64) - (m * scale)[:, None]).astype(x.dtype)
        return x - (m * scale).astype(x.dtype)[:, None]
    lo, hi = hf.ahfilt_windows(tnum, window)
    x0 = x[:, :1].astype(np.float64)                 # pivot: a strong flat band cancels before the long sums
    p = np.concatenate([np.zeros((snum, 1)), np.cumsum(x.astype(np.float64) - x0, axis=1)], axis=1)
    n = (hi - lo).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        m = np.where(n > 0, x0 + (p[:, hi] - p[:, lo]) / n, np.nan)
    del p
    if x.dtype == np.float32:
        m = m.astype(np.float32)
    ext = np.concatenate([2 * m[:1] - m[3:0:-1], m, 2 * m[-1:] - m[-2:-5:-1]], axis=0).astype(np.float64)
    w = np.array([1, 2, 3, 4, 3, 2, 1], dtype=np.float64) / 16.
    s = sum(w[k] * ext[k:k + snum] for k in range(7))
    out = x.astype(np.float64) - s * scale[:, None]
    with np.errstate(invalid='ignore'):
        return out.astype(x.dtype)


def assert_matches(got, g):
    want = g['out']
    np.testing.assert_array_equal(np.isnan(np.asarray(got, dtype=np.float64)), np.isnan(want.astype(np.float64)))
    ok = ~np.isnan(want.astype(np.float64))
    if not ok.any():
        return
    d = np.abs(np.asarray(got, dtype=np.float64)[ok] - want[ok].astype(np.float64))
    if np.issubdtype(want.dtype, np.integer):
        assert d.max() <= 1, d.max()
        return
    norm = np.max(np.abs(g['data'].astype(np.float64)))
    bar = 1e-12 if want.dtype == np.float64 else 2e-6
    assert d.max() / norm <= bar, d.max() / norm


# ------------------------------------------------------------------------------------------------ tables
def test_ahfilt_windows_match_python_slicing():
    for tnum in range(1, 41):
        for w in range(0, 91):
            lo, hi = hf.ahfilt_windows(tnum, w)
            h = w // 2
            for i in range(tnum):
                if i <= h:
                    s = slice(0, h + i)
                elif i >= tnum - h:
                    s = slice(tnum - w, tnum)
                else:
                    s = slice(i - h + 1, i + h)
                a, b, _ = s.indices(tnum)
                assert hi[i] - lo[i] == len(range(tnum)[s]), (tnum, w, i)
                if b > a:
                    assert (lo[i], hi[i]) == (a, b), (tnum, w, i)


def test_hfilt_bounds_clamp_as_the_reference():
    assert hf.hfilt_bounds(-5, 50, 100) == (0, 50)
    assert hf.hfilt_bounds(70, 500, 100) == (70, 100)
    assert hf.hfilt_bounds(0, -1, 100) == (0, 1)
    assert hf.hfilt_bounds(200, 300, 100) == (99, 100)


def test_fixtures_cover_the_cases():
    names = golden_names('H')
    assert len(names) >= 12
    kinds = {golden(n)['kind'].item() for n in names}
    assert kinds == {'hfilt', 'ahfilt'}
    assert np.isnan(golden('HB_ahfilt_window1_nan')['out']).all()
    assert golden('HC_ahfilt_snum13')['data'].shape[0] == 13


@pytest.mark.parametrize('name', golden_names('H'))
def test_closed_form_matches_the_reference(name):
    g = golden(name)
    got = closed_form(g['data'], g['travel_time'], g['kind'].item(), g['bounds'], int(g['window']))
    assert got.dtype == g['out'].dtype
    assert_matches(got, g)


# ------------------------------------------------------------------------------------------------ plumbing
def run_impproc(argv, loaded):
    with patch.object(sys, 'argv', ['impproc'] + argv), patch('impdar_amd.bin.impproc.load', return_value=loaded):
        impproc.main()


def test_impproc_hfilt_forwards_bounds_and_names_output():
    dat = MagicMock()
    run_impproc(['hfilt', '5', '-3', 'line_raw.mat'], [dat])
    dat.hfilt.assert_called_with(ftype='hfilt', bounds=(5, -3))
    dat.save.assert_called_with('line_hfilted.mat')
    with pytest.raises(SystemExit):
        run_impproc(['hfilt', '1.5', '3', 'x.mat'], [MagicMock()])


def test_impproc_ahfilt_always_uses_window_1000_like_the_reference():
    dat = MagicMock()
    run_impproc(['ahfilt', '25', 'x.mat'], [dat])
    dat.hfilt.assert_called_with(ftype='adaptive', window_size=1000)
    dat.save.assert_called_with('x_ahfilt.mat')
    with pytest.raises(SystemExit):
        run_impproc(['ahfilt', 'wide', 'x.mat'], [MagicMock()])


def mock_dat():
    d = MagicMock()
    d.data = np.zeros((16, 8), dtype=np.float32)
    return d


def test_process_ahfilt_order_and_residency():
    d = mock_dat()
    assert process.process([d], vbp=(1., 20.), ahfilt=[25], interp=(2.5, None), migrate='x') is True
    names = [c[0] for c in d.method_calls]
    assert names == ['to_device', 'vertical_band_pass', 'hfilt', 'constant_space', 'migrate', 'from_device']
    d.hfilt.assert_called_with(ftype='adaptive', window_size=25)
    d = mock_dat()
    assert process.process([d], ahfilt=7) is True                # one step: no residency
    assert [c[0] for c in d.method_calls] == ['hfilt']
    d.hfilt.assert_called_with(ftype='adaptive', window_size=7)
    d = mock_dat()
    assert process.process([d], ahfilt=0) is False               # the reference's `if ahfilt:`
    with pytest.raises(ValueError):
        process.process([mock_dat()], ahfilt=[1, 2])


def test_process_hfilt_is_still_rejected():
    with pytest.raises(NotImplementedError):
        process.process([mock_dat()], hfilt=(1, 2))


def test_impdar_proc_ahfilt_reaches_process():
    parser = impdarexec._get_args()
    kw = vars(parser.parse_args(['proc', '-vbp', '2', '12', '-ahfilt', '25', '-migrate', 'stolt', 'a.mat']))
    assert kw['ahfilt'] == [25] and kw['vbp'] == [2., 12.]
    with pytest.raises(SystemExit):
        parser.parse_args(['proc', '-ahfilt', '2.5', 'a.mat'])


def test_hfilt_unknown_type_raises():
    d = RadarData(None)
    with pytest.raises(ValueError, match='Unrecognized filter type'):
        d.hfilt(ftype='x')


def test_hfilt_dispatch():
    d = MagicMock()
    RadarData.hfilt(d, ftype='hfilt', bounds=(3, 9))
    d.horizontalfilt.assert_called_with(3, 9)
    RadarData.hfilt(d, ftype='adaptive', window_size=12)
    d.adaptivehfilt.assert_called_with(window_size=12)


def test_ahfilt_short_radargram_raises_scipys_error():
    d = RadarData(None)
    d.data = np.ones((12, 30), dtype=np.float32)
    d.snum, d.tnum = d.data.shape
    d.travel_time = np.arange(12) * 0.1
    with pytest.raises(ValueError, match='must be greater than padlen, which is 12'):
        d.adaptivehfilt(10)
    with pytest.raises(ValueError, match='must be greater than padlen, which is 12'):
        hf.ahfilt_host(np.ones((5, 30), dtype=np.int16), *hf.ahfilt_windows(30, 4), hf.taper(np.arange(5.)))


def test_reference_padlen_message_is_scipys():
    from scipy.signal import filtfilt
    with warnings.catch_warnings(), pytest.raises(ValueError) as e:
        filtfilt([.25] * 4, 1, np.ones(12))
    assert str(e.value) == hf.PADLEN_MESSAGE
