"""Denoise on the MI355X: every ``D*`` fixture of the reference through the host-buffer and the resident paths
(Wiener close to the reference and to the fp64 closed form, the median bit-identical, the resident result equal
to the host one bit for bit, two calls equal bit for bit), the chain's size with a strong flat band against the
closed form on row slabs and against SciPy's median filter on blocks with halo, NaN confinement, flat windows,
the all-flat error, and ``impproc denoise`` / ``impdar proc ... -denoise`` on .mat files."""
import contextlib
import io
import sys
from unittest.mock import patch

import numpy as np
import pytest

from conftest import golden, golden_names, rel_max
from test_denoise_cpu import _box, assert_wiener_close, bar_for, median_closed, reflect, wiener_closed

pytestmark = pytest.mark.gpu


def dat_of(data):
    from impdar_amd.lib.RadarData import RadarData
    d = RadarData(None)
    d.data = np.array(data, copy=True)
    d.snum, d.tnum = d.data.shape
    return d


def run(data, ftype, win, noise=None, resident=False):
    d = dat_of(data)
    if resident:
        d.to_device()
    d.denoise(int(win[0]), int(win[1]), noise=noise, ftype=ftype)
    if resident:
        assert d.data is None
        d.from_device()
    return d.data


@pytest.mark.parametrize('name', golden_names('D'))
def test_fixture_host_and_resident(hip, name):
    g = golden(name)
    ftype, win = g['ftype'].item(), tuple(int(w) for w in g['win'])
    noise = None if np.isnan(g['noise']) else float(g['noise'])
    got = run(g['data'], ftype, win, noise)
    assert got.dtype == g['out'].dtype
    if ftype == 'wiener':
        assert_wiener_close(got, g['out'], g['data'], bar_for(g['data']))
        assert_wiener_close(got, wiener_closed(g['data'], *win, noise)[0], g['data'], 1e-10)
    else:
        np.testing.assert_array_equal(got, g['out'])
    again = run(g['data'], ftype, win, noise)
    np.testing.assert_array_equal(again.view(np.uint8), got.view(np.uint8))
    if g['data'].dtype in (np.float32, np.float64):
        r = run(g['data'], ftype, win, noise, resident=True)
        assert r.dtype == got.dtype
        np.testing.assert_array_equal(r.view(np.uint8), got.view(np.uint8))


def banded(snum, tnum, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((snum, tnum))
    x[40:60] += 1000.0                                       # strong flat band on 20 rows (the direct wave)
    j = np.arange(tnum)
    rows = (100 + (j * 0.3).astype(int)) % snum
    x[rows, j] += 50.0                                       # dipping reflector
    return x.astype(np.float32)


SLABS = ((0, 12), (32, 70), (2000, 2010), (4084, 4096))


def box_slab(a, r0, r1, m, n):
    """Zero-padded (m, n) box sums of rows [r0, r1) of the full float64 array `a`: direct sums over the m rows,
    then a running sum along the row of the deviations from each row's mean (so that the long sums of a strong
    flat band keep their digits), plus the mean times the number of in-array columns of each window."""
    snum, tnum = a.shape
    lo, hi = r0 - m // 2, r1 + (m - 1) // 2
    blk = np.zeros((hi - lo, tnum))
    s, e = max(lo, 0), min(hi, snum)
    blk[s - lo:e - lo] = a[s:e]
    v = np.lib.stride_tricks.sliding_window_view(blk, m, axis=0).sum(axis=-1)
    piv = v.mean(axis=1, keepdims=True)
    vp = np.pad(v - piv, ((0, 0), (n // 2, (n - 1) // 2)))
    c = np.concatenate([np.zeros((vp.shape[0], 1)), np.cumsum(vp, axis=1)], axis=1)
    j = np.arange(tnum)
    k = np.minimum(j + (n - 1) // 2, tnum - 1) - np.maximum(j - n // 2, 0) + 1
    return (c[:, n:] - c[:, :-n]) + k[None, :] * piv


@pytest.fixture(scope='module')
def big():
    return banded(4096, 10000)


@pytest.mark.parametrize('win', [(1, 10), (5, 5), (21, 201)])
@pytest.mark.parametrize('given', [False, True])
def test_wiener_chain_size_with_flat_band(hip, big, win, given):
    from impdar_amd import denoise as dn
    from impdar_amd import _hip
    m, n = win
    d_x = _hip.DeviceArray.from_host(_hip.context(), big)
    d_out, noise = dn.wiener_dev(d_x, m, n, noise=0.8 if given else None)
    got = d_out.to_host()
    d_out.free()
    d_x.free()
    assert got.dtype == np.float64 and np.isfinite(got).all()
    x = big.astype(np.float64)
    sq = (big * big).astype(np.float64)
    if given:
        assert noise == 0.8
    else:
        # the noise against a slab-wise fp64 evaluation of mean(lVar) over the whole array
        tot = 0.0
        for r0 in range(0, 4096, 512):
            mean = box_slab(x, r0, r0 + 512, m, n) / (m * n)
            tot += float(np.sum(box_slab(sq, r0, r0 + 512, m, n) / (m * n) - mean ** 2))
        assert abs(noise - tot / x.size) <= 1e-9 * abs(noise), (noise, tot / x.size)
    for r0, r1 in SLABS:
        mean = box_slab(x, r0, r1, m, n) / (m * n)
        var = box_slab(sq, r0, r1, m, n) / (m * n) - mean ** 2
        want = np.where(var < noise, mean, (x[r0:r1] - mean) * (1 - noise / var) + mean)
        err = float(np.max(np.abs(got[r0:r1] - want))) / 1000.0
        assert err <= 1e-10, (r0, err)


@pytest.mark.parametrize('win', [(1, 10), (5, 5), (3, 21), (11, 101)])
def test_median_chain_size_with_flat_band(hip, big, win):
    from scipy.ndimage import median_filter
    from impdar_amd import denoise as dn
    from impdar_amd import _hip
    m, n = win
    d_x = _hip.DeviceArray.from_host(_hip.context(), big)
    d_out = dn.median_dev(d_x, m, n)
    got = d_out.to_host()
    d_out.free()
    d_x.free()
    assert got.dtype == np.float32
    snum, tnum = big.shape
    for r0, r1 in SLABS:
        for c0, c1 in ((0, 300), (5000, 5300), (tnum - 300, tnum)):
            a, b = max(r0 - m, 0), min(r1 + m, snum)
            c, e = max(c0 - n, 0), min(c1 + n, tnum)
            want = median_filter(big[a:b, c:e], size=(m, n))[r0 - a:r1 - a, c0 - c:c1 - c]
            np.testing.assert_array_equal(got[r0:r1, c0:c1], want, err_msg=str((r0, c0)))


def test_median_large_window_float64_matches_closed_form(hip):
    x = np.random.default_rng(3).standard_normal((70, 90))
    for win in ((9, 9), (13, 17), (80, 3), (2, 200)):
        np.testing.assert_array_equal(run(x, 'median', win), median_closed(x, *win))


def test_wiener_nan_confined_with_noise_given(hip):
    x = np.random.default_rng(5).standard_normal((200, 300))
    x[50, 60] = np.nan
    x[150, 7] = np.inf
    x[0, 299] = -np.inf
    for win in ((1, 10), (5, 5), (4, 6)):
        got = run(x, 'wiener', win, noise=0.7)
        want, _ = wiener_closed(x, *win, noise=0.7)
        bad = _box((~np.isfinite(x)).astype(float), *win) > 0
        np.testing.assert_array_equal(np.isnan(got), bad)
        assert np.isfinite(got[~bad]).all()
        assert float(np.max(np.abs(got[~bad] - want[~bad]))) <= 1e-10 * 5
        r = run(x, 'wiener', win, noise=0.7, resident=True)
        np.testing.assert_array_equal(r.view(np.uint8), got.view(np.uint8))
    assert np.isnan(run(x, 'wiener', (1, 10))).all()
    # the median must not fault on non-finite input; windows without one are exact
    y = x.astype(np.float32)
    for win in ((5, 5), (9, 9)):
        got = run(y, 'median', win)
        rows = reflect(np.arange(-(win[0] // 2), y.shape[0] + (win[0] - 1) // 2), y.shape[0])
        cols = reflect(np.arange(-(win[1] // 2), y.shape[1] + (win[1] - 1) // 2), y.shape[1])
        nf = (~np.isfinite(y))[np.ix_(rows, cols)]
        bad = np.lib.stride_tricks.sliding_window_view(nf, win).any(axis=(-2, -1))
        want = median_closed(y, *win)
        assert bad.sum() > 0
        np.testing.assert_array_equal(got[~bad], want[~bad])


def test_flat_block_gives_the_local_mean(hip):
    x = np.random.default_rng(6).standard_normal((120, 160))
    x[30:90, 40:120] = 3.0
    for noise in (None, 0.2):
        got = run(x, 'wiener', (3, 5), noise=noise)
        np.testing.assert_allclose(got[35:85, 45:115], 3.0, rtol=0, atol=1e-12)
        want, _ = wiener_closed(x, 3, 5, noise)
        assert_wiener_close(got, want, x)


def test_all_flat_raises_the_reference_error(hip):
    from impdar_amd import denoise as dn
    for data, win in ((np.zeros((50, 40)), (3, 5)), (np.zeros((50, 40), np.float32), (1, 10)),
                      (np.random.default_rng(1).standard_normal((50, 40)), (1, 1))):
        with pytest.raises(ValueError, match='^Could not compute variance, specify noise for denoise$'):
            dn.wiener_host(data, *win)
        d = dat_of(data)
        d.to_device()
        with pytest.raises(ValueError, match='Could not compute variance'):
            d.denoise(*win)
        d.from_device()                                       # the resident array is left as it was
        np.testing.assert_array_equal(d.data, data)
    out, noise = dn.wiener_host(np.zeros((50, 40)), 3, 5, noise=0.5)
    assert noise == 0.5 and (out == 0).all()


def _line_file(tmp_path, snum=160, tnum=90, seed=4):
    from impdar_amd import synth
    from impdar_amd.lib.NoInitRadarData import NoInitRadarData
    geo = synth.geometry(snum, tnum)
    rng = np.random.default_rng(seed)
    d = NoInitRadarData(big=True)
    d.data = synth.noise_radargram(snum, tnum, seed=seed)
    d.data[10:14] += 20.0
    d.snum, d.tnum = snum, tnum
    for k in ('lat', 'long', 'decday', 'pressure', 'x_coord', 'y_coord', 'elev'):
        setattr(d, k, np.cumsum(rng.random(tnum)))
    d.trig = np.zeros(tnum)
    d.trace_num = np.arange(tnum) + 1.
    d.travel_time, d.dt = geo['travel_time'], geo['dt']
    d.dist = np.hstack(([0.], np.cumsum(0.7 + 0.6 * rng.random(tnum - 1)))) / 1000.
    d.trace_int = np.hstack(([1.], np.diff(d.dist) * 1000.))
    fn = str(tmp_path / 'line_raw.mat')
    d.save(fn)
    return fn


def test_impproc_denoise_on_mat_file(hip, tmp_path):
    from impdar_amd.bin import impproc
    from impdar_amd.lib.RadarData import RadarData
    fn = _line_file(tmp_path)
    for argv, ftype in ((['denoise', '3', '7', fn], 'wiener'), (['denoise', '3', '7', '--filt', 'median', fn], 'median')):
        with patch.object(sys, 'argv', ['impproc'] + argv):
            impproc.main()
        r = RadarData(str(tmp_path / 'line_denoise.mat'))
        want = RadarData(fn)
        want.denoise(3, 7, ftype=ftype)
        np.testing.assert_array_equal(r.data, want.data)


def test_impdar_proc_vbp_ahfilt_denoise_migrate_resident_chain(hip, tmp_path, monkeypatch):
    """`impdar proc -vbp 2 10 -ahfilt 25 -denoise 1 10 -migrate stolt`: one resident chain, equal to the same
    steps run one by one on host buffers."""
    monkeypatch.setenv('IMPDAR_STOLT_FFT', 'own')           # one transform implementation for both runs
    from impdar_amd.bin import impdarexec
    from impdar_amd.lib.RadarData import RadarData
    fn = _line_file(tmp_path, seed=9)
    argv = ['impdar', 'proc', '-vbp', '2', '10', '-ahfilt', '25', '-denoise', '1', '10', '-migrate', 'stolt', fn]
    with patch.object(sys, 'argv', argv):
        impdarexec.main()
    r = RadarData(str(tmp_path / 'line_proc.mat'))
    want = RadarData(fn)
    with contextlib.redirect_stdout(io.StringIO()):
        want.vertical_band_pass(2., 10.)
        want.adaptivehfilt(25)
        want.denoise(1, 10)
        want.migrate(mtype='stolt')
    assert r.flags.mig == 'stolt' and r.data.shape == want.data.shape
    assert rel_max(r.data, want.data) < 1e-12
