"""Horizontal filters on the MI355X: every ``H*`` fixture of the reference through the host-buffer and the
resident paths, the resident result equal to the host one bit for bit, NaN traces where the reference has them,
the chain's size with a strong flat band against an fp64 NumPy restatement (including a radargram wider than
one fp64 row in LDS), and ``impproc hfilt / ahfilt`` and ``impdar proc -vbp -ahfilt -migrate`` on .mat files."""
import contextlib
import io
import os
import sys
from unittest.mock import patch

import numpy as np
import pytest

from conftest import golden, golden_names, rel_max
from test_hfilt_cpu import assert_matches, closed_form

pytestmark = pytest.mark.gpu


def run(d, g):
    with contextlib.redirect_stdout(io.StringIO()):
        if g['kind'].item() == 'hfilt':
            d.hfilt(ftype='hfilt', bounds=tuple(int(b) for b in g['bounds']))
        else:
            d.hfilt(ftype='adaptive', window_size=int(g['window']))


def dat_of(data, travel_time):
    from impdar_amd.lib.RadarData import RadarData
    d = RadarData(None)
    d.data = data.copy()
    d.snum, d.tnum = data.shape
    d.travel_time = np.asarray(travel_time).copy()
    return d


@pytest.mark.parametrize('name', golden_names('H'))
def test_fixture_host_and_resident(hip, name):
    g = golden(name)
    d = dat_of(g['data'], g['travel_time'])
    run(d, g)
    assert d.data.dtype == g['out'].dtype
    assert_matches(d.data, g)
    np.testing.assert_array_equal(np.isnan(np.asarray(d.data, dtype=np.float64)), np.isnan(g['out'].astype(np.float64)))
    assert list(np.asarray(d.flags.hfilt, dtype=float)) == list(g['flags_hfilt'])
    if g['data'].dtype in (np.float32, np.float64):
        r = dat_of(g['data'], g['travel_time'])
        r.to_device()
        run(r, g)
        r.from_device()
        assert r.data.dtype == d.data.dtype
        np.testing.assert_array_equal(r.data.view(np.uint8), d.data.view(np.uint8))     # bit for bit, NaNs included


def banded(snum, tnum, dtype, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((snum, tnum))
    x[40:60] += 1000.0                                       # strong flat band on 20 rows
    j = np.arange(tnum)
    rows = (100 + (j * 0.3).astype(int)) % snum
    x[rows, j] += 50.0                                       # dipping reflector
    return x.astype(dtype)


def check_large(x, kind, bounds=(0, 0), window=0):
    snum, tnum = x.shape
    tt = np.arange(snum) * 0.02
    d = dat_of(x, tt)
    d.to_device()
    run(d, dict(kind=np.array(kind), bounds=np.array(bounds), window=np.array(window)))
    d.from_device()
    want = closed_form(x, tt, kind, bounds, window)
    bar = 1e-12 if x.dtype == np.float64 else 2e-6
    assert np.isnan(d.data).sum() == np.isnan(want).sum() == 0
    err = float(np.max(np.abs(d.data.astype(np.float64) - want.astype(np.float64)))) / float(np.max(np.abs(x)))
    assert err <= bar, err


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('window', [3, 10, 1000, 20000])
def test_ahfilt_chain_size_with_flat_band(hip, dtype, window):
    check_large(banded(4096, 10000, dtype), 'ahfilt', window=window)


@pytest.mark.parametrize('window', [1000, 20000])
def test_ahfilt_wider_than_lds(hip, window):
    check_large(banded(600, 40000, np.float32, seed=3), 'ahfilt', window=window)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_hfilt_chain_size_with_flat_band(hip, dtype):
    check_large(banded(4096, 10000, dtype, seed=1), 'hfilt', bounds=(100, 9000))


def test_ahfilt_snum_12_fails_with_scipys_message(hip):
    from impdar_amd import _hip, hfilt as hf
    d_x = _hip.DeviceArray.from_host(_hip.context(), np.zeros((12, 50), dtype=np.float32))
    lo, hi = hf.ahfilt_windows(50, 10)
    with pytest.raises(ValueError, match='must be greater than padlen, which is 12'):
        hf.ahfilt_dev(d_x, lo, hi, np.ones(12))
    d_x.free()


def _line_file(tmp_path, snum=160, tnum=90, seed=4):
    from impdar_amd import synth
    from impdar_amd.lib.NoInitRadarData import NoInitRadarData
    geo = synth.geometry(snum, tnum)
    rng = np.random.default_rng(seed)
    d = NoInitRadarData(big=True)
    d.data = synth.noise_radargram(snum, tnum, seed=seed)
    d.data[10:14] += 20.0                                    # a flat band for the filters to remove
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


def test_impproc_hfilt_and_ahfilt_on_mat_file(hip, tmp_path):
    from impdar_amd.bin import impproc
    from impdar_amd.lib.RadarData import RadarData
    fn = _line_file(tmp_path)
    with patch.object(sys, 'argv', ['impproc', 'ahfilt', '25', fn]):
        impproc.main()
    r = RadarData(str(tmp_path / 'line_ahfilt.mat'))
    want = RadarData(fn)
    with contextlib.redirect_stdout(io.StringIO()):
        want.adaptivehfilt(1000)                             # the reference's impproc ignores `win`
    np.testing.assert_array_equal(r.data, want.data)
    assert list(np.asarray(r.flags.hfilt, dtype=float)) == [1., 4.]
    with patch.object(sys, 'argv', ['impproc', 'hfilt', '5', '60', fn]):
        impproc.main()
    r = RadarData(str(tmp_path / 'line_hfilted.mat'))
    want = RadarData(fn)
    with contextlib.redirect_stdout(io.StringIO()):
        want.horizontalfilt(5, 60)
    np.testing.assert_array_equal(r.data, want.data)
    assert list(np.asarray(r.flags.hfilt, dtype=float)) == [1., 1.]


def test_impdar_proc_vbp_ahfilt_migrate_resident_chain(hip, tmp_path, monkeypatch):
    """`impdar proc -vbp 2 12 -ahfilt 25 -migrate stolt`: one resident chain, equal to the same steps run one by
    one on host buffers."""
    monkeypatch.setenv('IMPDAR_STOLT_FFT', 'own')           # one transform implementation for both runs
    from impdar_amd.bin import impdarexec
    from impdar_amd.lib.RadarData import RadarData
    fn = _line_file(tmp_path, seed=9)
    with patch.object(sys, 'argv', ['impdar', 'proc', '-vbp', '2', '12', '-ahfilt', '25', '-migrate', 'stolt', fn]):
        impdarexec.main()
    r = RadarData(str(tmp_path / 'line_proc.mat'))
    want = RadarData(fn)
    with contextlib.redirect_stdout(io.StringIO()):
        want.vertical_band_pass(2., 12.)
        want.adaptivehfilt(25)
        want.migrate(mtype='stolt')
    assert r.flags.mig == 'stolt' and r.data.shape == want.data.shape
    assert list(np.asarray(r.flags.hfilt, dtype=float)) == [1., 4.]
    assert rel_max(r.data, want.data) < 1e-12
    assert os.path.exists(fn)
