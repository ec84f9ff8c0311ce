"""Denoise without a GPU: a NumPy closed form of both filters (direct fp64 window sums for Wiener, an
``np.sort`` rank for the median) against every ``D*`` fixture of the reference -- this pins the window
alignment, the zero padding, the reflection and the rank -- and the plumbing of ``RadarData.denoise``,
``process(denoise=...)``, ``impdar proc -denoise`` and ``impproc denoise`` with the device calls mocked."""
import sys
from unittest.mock import MagicMock, patch

import numpy as np
import pytest

from conftest import golden, golden_names
from impdar_amd import denoise as dn
from impdar_amd.bin import impdarexec, impproc
from impdar_amd.lib import process
from impdar_amd.lib.RadarData import RadarData


def _box(a, m, n):
    """Zero-padded (m, n) box sums of a 2-D float64 array; output i covers i - w//2 .. i + (w-1)//2."""
    p = np.pad(a, ((m // 2, (m - 1) // 2), (n // 2, (n - 1) // 2)))
    v = np.lib.stride_tricks.sliding_window_view(p, m, axis=0).sum(axis=-1)
    return np.lib.stride_tricks.sliding_window_view(v, n, axis=1).sum(axis=-1)


def wiener_closed(data, m, n, noise=None):
    """fp64 restatement of scipy.signal.wiener; integers widened first, float32 squares rounded to float32.
    An output whose window holds a non-finite value is NaN."""
    x = np.asarray(data)
    if x.dtype not in (np.float32, np.float64):
        x = x.astype(np.float64)
    bad = ~np.isfinite(x)
    xz = np.where(bad, 0, x)
    sq = (xz * xz).astype(np.float64)                   # float32 * float32 rounds to float32, as the reference
    N = m * n
    cnt = _box(bad.astype(np.float64), m, n)
    mean = _box(xz.astype(np.float64), m, n) / N
    var = _box(sq, m, n) / N - mean ** 2
    mean[cnt > 0] = np.nan
    var[cnt > 0] = np.nan
    if noise is None:
        noise = np.mean(var)
    with np.errstate(divide='ignore', invalid='ignore'):
        out = np.where(var < noise, mean, (x.astype(np.float64) - mean) * (1 - noise / var) + mean)
    return out, noise


def reflect(j, L):
    j = np.mod(j, 2 * L)
    return np.where(j < L, j, 2 * L - 1 - j)


def median_closed(data, m, n):
    """scipy.ndimage.median_filter(size=(m, n)), mode 'reflect', rank N // 2, in the data's dtype."""
    x = np.asarray(data)
    snum, tnum = x.shape
    rows = reflect(np.arange(-(m // 2), snum + (m - 1) // 2), snum)
    cols = reflect(np.arange(-(n // 2), tnum + (n - 1) // 2), tnum)
    p = x[np.ix_(rows, cols)]
    w = np.lib.stride_tricks.sliding_window_view(p, (m, n)).reshape(snum, tnum, m * n)
    return np.sort(w, axis=-1)[:, :, (m * n) // 2]


# The reference transforms float32 data in single precision (scipy's fftconvolve keeps the input's precision),
# so its own float32 results are only that good: a float32 fixture is held to 2e-6 of max|x|, and the exact
# float32 semantics (float32-rounded squares, fp64 sums) to 1e-10 against the closed form.
def bar_for(data):
    return 2e-6 if np.asarray(data).dtype == np.float32 else 1e-10


def assert_wiener_close(got, want, data, bar=1e-10):
    got = np.asarray(got)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    norm = float(np.max(np.abs(np.asarray(data, dtype=np.float64))))
    err = float(np.max(np.abs(got[ok] - want[ok]))) / norm
    assert err <= bar, err


# ------------------------------------------------------------------------------------------------ closed form
def test_fixtures_cover_the_cases():
    names = golden_names('D')
    assert len(names) >= 12
    gs = [golden(nm) for nm in names]
    kinds = {(g['ftype'].item(), g['data'].dtype.name) for g in gs}
    assert {('wiener', 'float64'), ('wiener', 'float32'), ('wiener', 'int16'), ('median', 'float64'),
            ('median', 'float32'), ('median', 'int16')} <= kinds
    assert any(g['win'][0] > g['data'].shape[0] and g['win'][1] > g['data'].shape[1] for g in gs)
    assert any(np.isfinite(g['noise']) for g in gs)
    assert any(tuple(g['win']) == (1, 1) for g in gs)
    i16 = golden('D7_wiener_int16')['data']
    assert np.abs(i16).max() > 181                         # its square wraps in int16


@pytest.mark.parametrize('name', golden_names('D'))
def test_closed_form_matches_the_reference(name):
    g = golden(name)
    m, n = (int(w) for w in g['win'])
    if g['ftype'].item() == 'wiener':
        noise = None if np.isnan(g['noise']) else float(g['noise'])
        got, _ = wiener_closed(g['data'], m, n, noise)
        assert_wiener_close(got, g['out'], g['data'], bar_for(g['data']))
    else:
        got = median_closed(g['data'], m, n)
        assert got.dtype == g['out'].dtype
        np.testing.assert_array_equal(got, g['out'])


# ------------------------------------------------------------------------------------------------ plumbing
def mock_dat():
    d = MagicMock()
    d.data = np.zeros((16, 8), dtype=np.float32)
    return d


def test_process_denoise_order_and_residency():
    d = mock_dat()
    assert process.process([d], vbp=(1., 20.), ahfilt=[25], denoise=[1, 10], interp=(2.5, None), migrate='x')
    names = [c[0] for c in d.method_calls]
    assert names == ['to_device', 'vertical_band_pass', 'hfilt', 'denoise', 'constant_space', 'migrate',
                     'from_device']
    d.denoise.assert_called_with(1, 10)
    d = mock_dat()
    assert process.process([d], denoise=(3, 5)) is True          # one step: no residency
    assert [c[0] for c in d.method_calls] == ['denoise']
    d.denoise.assert_called_with(3, 5)


@pytest.mark.parametrize('bad', [(1.0, 10), (1, '10'), (1,), 5, (np.int64(1), 10), (True, 3)])
def test_process_denoise_validation(bad):
    with pytest.raises(ValueError, match='Denoise must be two integers giving vertical and horizontal window sizes'):
        process.process([mock_dat()], denoise=bad)


def test_process_other_steps_still_rejected():
    for name in ('nmo', 'hfilt', 'restack'):
        with pytest.raises(NotImplementedError):
            process.process([mock_dat()], **{name: (1, 2)})


def test_impdar_proc_denoise_reaches_process():
    parser = impdarexec._get_args()
    kw = vars(parser.parse_args(['proc', '-denoise', '1', '10', 'a.mat']))
    assert kw['denoise'] == [1, 10]
    with patch('impdar_amd.lib.process.load', return_value=[mock_dat()]) as ld, \
            patch('impdar_amd.lib.process.process', return_value=False) as pr:
        with patch.object(sys, 'argv', ['impdar', 'proc', '-denoise', '1', '10', 'a.mat']):
            impdarexec.main()
    ld.assert_called_once()
    assert pr.call_args[1]['denoise'] == [1, 10]
    with pytest.raises(SystemExit):
        parser.parse_args(['proc', '-denoise', '1.5', '3', 'a.mat'])


def run_impproc(argv, loaded):
    with patch.object(sys, 'argv', ['impproc'] + argv), patch('impdar_amd.bin.impproc.load', return_value=loaded):
        impproc.main()


def test_impproc_denoise_forwards_maps_weiner_and_names_output():
    dat = MagicMock()
    run_impproc(['denoise', '3', '7', 'line_raw.mat'], [dat])
    dat.denoise.assert_called_with(vert_win=3, hor_win=7, noise=None, ftype='wiener')
    dat.save.assert_called_with('line_denoise.mat')
    dat = MagicMock()
    run_impproc(['denoise', '1', '10', '--filt', 'median', 'x.mat'], [dat])
    dat.denoise.assert_called_with(vert_win=1, hor_win=10, noise=None, ftype='median')
    dat = MagicMock()
    run_impproc(['denoise', '1', '10', '--filt', 'wiener', 'x.mat'], [dat])
    dat.denoise.assert_called_with(vert_win=1, hor_win=10, noise=None, ftype='wiener')
    with pytest.raises(SystemExit):
        run_impproc(['denoise', '1', '10', '--filt', 'gauss', 'x.mat'], [MagicMock()])


def test_denoise_unknown_ftype_raises():
    d = RadarData(None)
    d.data = np.ones((8, 8))
    with pytest.raises(ValueError, match='Only the wiener filter has been implemented for denoising.'):
        d.denoise(1, 3, ftype='weiner')
    with pytest.raises(ValueError, match='Only the wiener filter has been implemented for denoising.'):
        d.denoise(1, 3, ftype='gauss')


@pytest.mark.parametrize('win', [(0, 10), (1, 0), (-3, 5), (1.5, 3)])
def test_denoise_window_below_one_raises(win):
    with pytest.raises(ValueError):
        dn.check_windows(*win)
    d = RadarData(None)
    d.data = np.ones((8, 8))
    for ftype in ('wiener', 'median'):
        with pytest.raises(ValueError):
            d.denoise(win[0], win[1], ftype=ftype)
