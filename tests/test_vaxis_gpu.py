"""The sample-axis steps on the MI355X: every ``X*`` fixture of the reference through the host-buffer path and, for
float input, the resident path (equal bit for bit, NaNs included); the copy-only paths (row-range crop, column
shift) equal to the fixture bit for bit and the row blend within 1e-12 of max|expected| (the bar
``constant_space`` is held to); the chain's size, 4096 x 10000 and a trace count that is not a multiple of 4,
against NumPy restatements written here; and ``impproc crop`` -> ``nmo`` -> ``migrate`` on a .mat file."""
import contextlib
import io
import sys
from unittest.mock import patch

import numpy as np
import pytest

from conftest import golden
from test_vaxis_cpu import CASES, TOL, run_fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _one_transform_implementation(monkeypatch):
    monkeypatch.setenv('IMPDAR_STOLT_FFT', 'own')


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize('name', CASES)
def test_fixture_host_and_resident(hip, name, tmp_path):
    g = golden(name)
    _, host = run_fixture(g, tmp_path)
    if g['in_data'].dtype in (np.float32, np.float64):
        r, res = run_fixture(g, tmp_path, resident=True)
        r.from_device()
        for a, b in zip(host, res):
            assert a.dtype == b.dtype and a.shape == b.shape
            np.testing.assert_array_equal(bits(a), bits(b))


def big_dat(x, dt=1e-8):
    from impdar_amd.lib.RadarData import RadarData
    d = RadarData(None)
    d.data = x
    d.snum, d.tnum = x.shape
    d.dt = dt
    d.travel_time = np.arange(d.snum) * dt * 1e6
    d.trig = np.zeros(d.tnum)
    return d


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def nmo_restated(x, tt, dt, ant_sep, uice=1.69e8):
    """The reference's formula in NumPy fp64: move-out times, the new time axis, interp1d's slope form with the
    knot search SciPy uses for the dtype (``np.interp`` for float64, ``searchsorted(...).clip`` for float32)."""
    tsep = 1e6 * (ant_sep / uice)
    nmotime = np.sqrt((tt + tsep) ** 2. - tsep ** 2.)
    new_tt = np.arange(tt.min(), nmotime.max(), dt * 1e6)
    if x.dtype == np.float32:
        hi = np.searchsorted(nmotime, new_tt).clip(1, len(tt) - 1)
    else:
        hi = np.minimum(np.searchsorted(nmotime, new_tt, side='right'), len(tt) - 1)
    lo = hi - 1
    out = np.empty((len(new_tt), x.shape[1]))
    for a in range(0, len(new_tt), 256):                          # in row blocks: the temporaries stay small
        s = slice(a, a + 256)
        slope = (x[hi[s]] - x[lo[s]]) / (nmotime[hi[s]] - nmotime[lo[s]])[:, None]
        out[s] = slope * (new_tt[s] - nmotime[lo[s]])[:, None] + x[lo[s]]
    return new_tt, out


@pytest.fixture(scope='module')
def big_x():
    return np.random.default_rng(11).standard_normal((4096, 10002)).astype(np.float32)


@pytest.mark.parametrize('dtype,tnum', [(np.float32, 10000), (np.float64, 10000), (np.float32, 10001), (np.float64, 10001),
                                        (np.float32, 10002)])
def test_nmo_at_chain_size(hip, big_x, dtype, tnum):
    x = np.ascontiguousarray(big_x[:, :tnum]).astype(dtype)
    d = big_dat(x)
    want_tt, want = nmo_restated(x, d.travel_time, d.dt, 60.)
    d.to_device()
    quiet(d.nmo, 60.)
    d.from_device()
    assert d.data.dtype == np.float64 and d.data.shape == want.shape and d.snum == len(want_tt)
    np.testing.assert_array_equal(d.travel_time, want_tt)
    err = float(np.max(np.abs(d.data - want))) / float(np.max(np.abs(want)))
    print('nmo %s x %d: max|diff| / max|expected| = %.3e' % (np.dtype(dtype).name, tnum, err))
    assert err <= TOL, err
    assert list(d.flags.nmo) == [1, 60.]


@pytest.mark.parametrize('dtype,tnum', [(np.float32, 10000), (np.float32, 10001), (np.float64, 10001)])
def test_pretrigger_crop_and_elev_correct_at_chain_size(hip, big_x, dtype, tnum):
    x = np.ascontiguousarray(big_x[:, :tnum]).astype(dtype)
    snum = x.shape[0]
    rng = np.random.default_rng(12)
    trig = (20 + np.cumsum(rng.integers(-1, 2, tnum)).clip(-15, 15)).astype(int)
    d = big_dat(x)
    d.trig = trig.copy()
    d.to_device()
    quiet(d.crop, 0, dimension='pretrig')
    n_out = snum - trig.min()
    want = np.full((n_out, tnum), np.nan)
    for j in range(tnum):
        want[:snum - trig[j], j] = x[trig[j]:, j]
    cropped = d._dev.to_host()
    assert cropped.dtype == np.float64 and d.snum == n_out and not d.trig.any()
    np.testing.assert_array_equal(bits(cropped), bits(want))
    # elevation correction of the cropped radargram (NaNs travel as they are)
    d.nmo_depth = d.travel_time / 2. * 1.69e8 * 1e-6
    d.elev = 1500. + 8. * np.sin(np.arange(tnum) / 300.) + 0.001 * np.arange(tnum)
    dz = d.dt * 1.69e8 / 2.
    top = ((d.elev.max() - d.elev) / dz).astype(int)
    quiet(d.elev_correct)
    d.from_device()
    want2 = np.full((n_out + top.max(), tnum), np.nan)
    for j in range(tnum):
        want2[top[j]:top[j] + n_out, j] = want[:, j]
    assert d.data.shape == want2.shape and d.flags.elev == 1 and d.snum == n_out
    np.testing.assert_array_equal(bits(d.data), bits(want2))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('tnum', [66, 67, 68])
def test_every_access_width_of_both_kernels(hip, dtype, tnum):
    """Trace counts with tnum % 4 of 2, 3 and 0 on float32 and float64 input: every instantiation of the row
    blend and of the column shift (elev_correct straight on the input dtype), against NumPy."""
    x = np.random.default_rng(tnum).standard_normal((150, tnum)).astype(dtype)
    d = big_dat(x.copy())
    want_tt, want = nmo_restated(x, d.travel_time, d.dt, 60.)
    d.to_device()
    quiet(d.nmo, 60.)
    d.from_device()
    assert d.data.shape == want.shape and float(np.max(np.abs(d.data - want))) <= TOL * float(np.max(np.abs(want)))
    e = big_dat(x.copy())
    e.nmo_depth = e.travel_time / 2. * 1.69e8 * 1e-6
    e.elev = 100. + 3. * np.sin(np.arange(tnum) / 7.)
    top = ((e.elev.max() - e.elev) / (e.dt * 1.69e8 / 2.)).astype(int)
    e.to_device()
    quiet(e.elev_correct)
    e.from_device()
    want = np.full((150 + top.max(), tnum), np.nan)
    for j in range(tnum):
        want[top[j]:top[j] + 150, j] = x[:, j]
    assert e.data.dtype == np.float64
    np.testing.assert_array_equal(bits(e.data), bits(want))


def test_scalar_crop_keeps_dtype_on_both_paths(hip):
    x = np.random.default_rng(13).standard_normal((300, 77)).astype(np.float32)
    h = big_dat(x.copy())
    quiet(h.crop, 41)
    r = big_dat(x.copy())
    r.to_device()
    quiet(r.crop, 41)
    r.from_device()
    assert r.data.dtype == np.float32 and np.array_equal(r.data, x[41:]) and np.array_equal(h.data, x[41:])
    i = big_dat((x * 100).astype(np.int16))
    quiet(i.crop, 1.0, top_or_bottom='bottom', dimension='twtt')
    assert i.data.dtype == np.int16 and i.data.shape == (100, 77)


def test_impproc_crop_nmo_migrate_on_mat_file(hip, tmp_path):
    """`impproc crop top pretrig 0`, `impproc nmo 60`, `impproc migrate --mtype stolt` on files = the same three
    methods one by one; the bookkeeping survives the .mat files."""
    from impdar_amd import synth
    from impdar_amd.bin import impproc
    from impdar_amd.lib.NoInitRadarData import NoInitRadarData
    from impdar_amd.lib.RadarData import RadarData
    snum, tnum, pre = 160, 90, 12
    geo = synth.geometry(snum, tnum)
    d = NoInitRadarData(big=True)
    d.data = synth.noise_radargram(snum, tnum, seed=4)
    d.snum, d.tnum = snum, tnum
    for k in ('lat', 'long', 'decday', 'pressure', 'x_coord', 'y_coord', 'elev'):
        setattr(d, k, np.arange(tnum, dtype=float))
    d.trig = np.full(tnum, pre)
    d.trace_num = np.arange(tnum) + 1.
    d.travel_time, d.dt, d.dist, d.trace_int = geo['travel_time'], geo['dt'], geo['dist'], geo['trace_int']
    fn = str(tmp_path / 'line_raw.mat')
    d.save(fn)
    for argv in (['crop', 'top', 'pretrig', '0', fn], ['nmo', '60', str(tmp_path / 'line_cropped.mat')],
                 ['migrate', '--mtype', 'stolt', str(tmp_path / 'line_cropped_nmo.mat')]):
        with patch.object(sys, 'argv', ['impproc'] + argv):
            quiet(impproc.main)
    r = RadarData(str(tmp_path / 'line_cropped_nmo_migrated.mat'))
    m = RadarData(fn)
    quiet(m.crop, 0., top_or_bottom='top', dimension='pretrig')
    assert m.data.shape[0] == snum - pre and not np.isnan(m.data).any()
    quiet(m.nmo, 60., uice=1.69e8, uair=3.0e8, rho_profile=None)
    quiet(m.migrate, 'stolt', vel=1.69e8, vtaper=1000, htaper=100, tmig=0, verbose=1, vel_fn=None, nxpad=100, nearfield=False)
    assert r.data.shape == m.data.shape
    np.testing.assert_array_equal(r.data, m.data)
    np.testing.assert_array_equal(r.nmo_depth, m.nmo_depth)
    np.testing.assert_array_equal(r.travel_time, m.travel_time)
    assert list(r.flags.crop) == [1., pre, snum] and list(r.flags.nmo) == [1., 60.] and r.flags.mig == 'stolt'
    assert r.snum == m.snum == len(r.travel_time)
