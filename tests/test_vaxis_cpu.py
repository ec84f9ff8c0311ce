"""The sample-axis steps (crop, nmo, elev_correct) without a GPU: the host tables alone reproduce every ``X*``
fixture of the reference in NumPy (row blend within 1e-12 of max|expected|, shifts bit for bit), the attribute
bookkeeping of the ``RadarData`` methods with the device calls replaced by those NumPy restatements, the
reference's errors, the ``impproc`` sub-commands with mocked data, and the new symbols of the C ABI."""
import contextlib
import io
import os
import sys
from unittest.mock import MagicMock, patch

import numpy as np
import pytest

from conftest import ROOT, golden, golden_names
from impdar_amd import vaxis
from impdar_amd.bin import impproc
from impdar_amd.lib.ImpdarError import ImpdarError
from impdar_amd.lib.RadarData import RadarData

TOL = 1e-12
CASES = [n for n in golden_names('X') if n != 'XZ_errors']


# ------------------------------------------------------------------------------- NumPy stand-ins for the kernels
def np_row_lerp(data, tables):
    data = np.asarray(data)
    if data.dtype not in (np.float32, np.float64):
        data = data.astype(np.float64)
    slope = (data[tables.hi] - data[tables.lo]) / tables.den[:, None]
    return slope * tables.t[:, None] + data[tables.lo]


def np_col_shift(data, shift, n_out):
    data = np.asarray(data)
    snum, tnum = data.shape
    out = np.full((n_out, tnum), np.nan)
    for j in range(tnum):
        i0, i1 = max(0, -shift[j]), min(n_out, snum - shift[j])
        if i1 > i0:
            out[i0:i1, j] = data[i0 + shift[j]:i1 + shift[j], j]
    return out


@contextlib.contextmanager
def kernels_in_numpy():
    with patch.object(vaxis, 'row_lerp_host', np_row_lerp), patch.object(vaxis, 'col_shift_host', np_col_shift):
        yield


# ------------------------------------------------------------------------------------------- fixture plumbing
def dat_of(g, prefix='in_', resident=False):
    d = RadarData(None)
    d.data = g[prefix + 'data'].copy()
    d.snum, d.tnum = d.data.shape
    d.dt = float(g['dt'])
    d.travel_time = g[prefix + 'travel_time'].copy()
    trig = g[prefix + 'trig']
    d.trig = trig.copy() if trig.ndim else trig.item()
    d.nmo_depth = g[prefix + 'nmo_depth'].copy() if prefix + 'nmo_depth' in g else None
    d.elev = g['elev'].copy() if 'elev' in g else None
    d.flags.crop = g[prefix + 'flags_crop'].copy()
    d.flags.nmo = g[prefix + 'flags_nmo'].copy()
    if resident:
        d.to_device()
    return d


def steps_of(g, tmp_path):
    """[(callable on a RadarData, prefix of the expected state)] for a fixture."""
    kind = g['kind'].item()
    if kind == 'nmo':
        kw = dict(uice=float(g['uice']), uair=float(g['uair']), const_sample=bool(g['const_sample']))
        if not np.isnan(g['const_firn_offset']):
            kw['const_firn_offset'] = float(g['const_firn_offset'])
        if bool(g['has_profile']):
            fn = str(tmp_path / 'rho.csv')
            np.savetxt(fn, np.column_stack((g['profile_depth'], g['profile_rho'])), delimiter=',')
            kw['rho_profile'] = fn
        return [(lambda d: d.nmo(float(g['ant_sep']), **kw), 'out_')]
    if kind == 'elev':
        return [(lambda d: d.elev_correct(), 'out_')]
    steps = []
    for k in range(int(g['ncalls'])):
        kw = dict(top_or_bottom=g['call%d_top_or_bottom' % k].item(), dimension=g['call%d_dimension' % k].item(),
                  rezero=bool(g['call%d_rezero' % k]), zero_trig=bool(g['call%d_zero_trig' % k]))
        lim = g['call%d_lim' % k].item()
        steps.append((lambda d, lim=lim, kw=kw: d.crop(lim, **kw), 'out%d_' % k))
    return steps


def is_copy_only(g):
    return g['kind'].item() in ('crop', 'elev')


def check_data(got, want, exact):
    assert got.shape == want.shape and got.dtype == want.dtype
    np.testing.assert_array_equal(np.isnan(got.astype(np.float64)), np.isnan(want.astype(np.float64)))
    if exact:
        np.testing.assert_array_equal(got, want)
    else:
        ok = ~np.isnan(want)
        err = float(np.max(np.abs(got[ok] - want[ok]))) / float(np.max(np.abs(want[ok])))
        print('row blend: max|diff| / max|expected| = %.3e' % err)
        assert err <= TOL, err


def check_state(d, g, prefix, data=None):
    data = d.data if data is None else data
    check_data(data, g[prefix + 'data'], exact=is_copy_only(g))
    np.testing.assert_allclose(d.travel_time, g[prefix + 'travel_time'], rtol=1e-13, atol=0)
    assert d.travel_time.shape == g[prefix + 'travel_time'].shape
    assert d.snum == int(g[prefix + 'snum'])
    np.testing.assert_array_equal(np.asarray(d.trig), g[prefix + 'trig'])
    if prefix + 'nmo_depth' in g:
        np.testing.assert_allclose(d.nmo_depth, g[prefix + 'nmo_depth'], rtol=1e-13, atol=0)
    else:
        assert d.nmo_depth is None
    np.testing.assert_array_equal(np.asarray(d.flags.crop, dtype=float), g[prefix + 'flags_crop'])
    np.testing.assert_array_equal(np.asarray(d.flags.nmo, dtype=float), g[prefix + 'flags_nmo'])
    assert d.flags.elev == g[prefix + 'flags_elev']
    if g['kind'].item() == 'elev':
        np.testing.assert_allclose(d.elevation, g['elevation'], rtol=1e-13, atol=0)


def run_fixture(g, tmp_path, resident=False):
    """Every step of a fixture on a host or resident RadarData; the data after each step."""
    d = dat_of(g, resident=resident)
    datas = []
    for step, prefix in steps_of(g, tmp_path):
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            step(d)
        if resident:
            assert d.data is None
            dev = d._dev
            datas.append(dev.to_host())
        else:
            datas.append(d.data)
        check_state(d, g, prefix, datas[-1])
    assert out.getvalue() in g['stdout'].item() if 'stdout' in g else True
    return d, datas


# ------------------------------------------------------------------------------------------------ the tests
def test_fixtures_cover_the_cases():
    kinds = [golden(n)['kind'].item() for n in CASES]
    assert kinds.count('nmo') >= 8 and kinds.count('crop') >= 8 and kinds.count('elev') >= 3
    nmo = [golden(n) for n in CASES if golden(n)['kind'].item() == 'nmo']
    assert {g['in_data'].dtype for g in nmo} == {np.dtype(np.float64), np.dtype(np.float32), np.dtype(np.int16)}
    assert {float(g['ant_sep']) for g in nmo} == {0., 60., 160.}
    assert any(bool(g['has_profile']) and bool(g['const_sample']) for g in nmo)
    assert all(g['out_data'].dtype == np.float64 for g in nmo)
    assert np.isnan(golden('XO_crop_pretrig_vector_f64')['out0_data']).any()
    assert golden('XP_crop_pretrig_vector_f32')['out0_data'].dtype == np.float64
    assert golden('XS_elev_flat_f64')['out_data'].shape == golden('XS_elev_flat_f64')['in_data'].shape
    for n in golden_names('X'):
        assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', n + '.npz')) < 300 * 1024


@pytest.mark.parametrize('name', CASES)
def test_host_tables_and_bookkeeping_match_the_reference(name, tmp_path):
    with kernels_in_numpy():
        run_fixture(golden(name), tmp_path)


@pytest.mark.parametrize('name', ['XB_nmo_f64_sep60', 'XC_nmo_f32_sep60', 'XD_nmo_int16_sep160'])
def test_the_other_knot_search_stays_inside_the_bar(name):
    """The worst case the bar leaves room for: tables built with the other dtype's knot convention."""
    g = golden(name)
    nmotime = vaxis.nmo_times(g['in_travel_time'], float(g['ant_sep']), float(g['uice']))
    for conv in (True, False):
        tables = vaxis.RowLerpTables(nmotime, g['out_travel_time'], conv)
        check_data(np_row_lerp(g['in_data'], tables), g['out_data'], exact=False)


def test_row_lerp_tables_follow_scipy_for_each_dtype():
    from scipy.interpolate import interp1d
    rng = np.random.default_rng(0)
    x = np.cumsum(0.5 + rng.random(40))
    x_new = np.hstack((x[[0, 7, 39]], np.linspace(x[0], x[-1], 57)))
    for dtype in (np.float64, np.float32, np.int16):
        y = (rng.standard_normal((40, 3)) * 100).astype(dtype)
        tables = vaxis.RowLerpTables(x, x_new, vaxis.np_interp_convention(dtype))
        want = np.stack([interp1d(x, y[:, j])(x_new) for j in range(3)], axis=1)
        np.testing.assert_array_equal(np_row_lerp(y, tables), want)
    y = rng.standard_normal((40, 3))
    y[8] = np.nan                                   # a new point ON knot 7 must not see the NaN of knot 8
    tables = vaxis.RowLerpTables(x, x_new, True)
    want = np.stack([interp1d(x, y[:, j])(x_new) for j in range(3)], axis=1)
    np.testing.assert_array_equal(np_row_lerp(y, tables), want)


def test_firn_permittivity_is_the_decomp_formula():
    assert abs(vaxis.firn_permittivity(917.) - (3.12 + 9.5j)) < 1e-12
    assert abs(vaxis.firn_permittivity(0.) - 1.0) < 1e-15
    eps = np.real(vaxis.firn_permittivity(np.array([350., 600.])))
    assert 1.5 < eps[0] < eps[1] < 3.12


def test_errors_are_the_references():
    g = golden('XZ_errors')
    want = {str(l): (str(t), str(m)) for l, t, m in zip(g['label'], g['exc_type'], g['message'])}
    tnum = g['data'].shape[1]

    def dat(t0=0.0, trig=None, elev=None):
        d = RadarData(None)
        d.data = g['data'].copy()
        d.snum, d.tnum = d.data.shape
        d.dt = float(g['dt'])
        d.travel_time = t0 + np.arange(d.snum) * d.dt * 1e6
        d.trig = np.zeros(tnum) if trig is None else trig
        d.elev = elev
        return d
    calls = {'nmo_range': lambda: dat(t0=0.2).nmo(60.),
             'nmo_trig': lambda: dat(trig=np.full(tnum, 3.)).nmo(60.),
             'crop_top_or_bottom': lambda: dat().crop(10, top_or_bottom='side'),
             'crop_dimension': lambda: dat().crop(10, dimension='dist'),
             'crop_bottom_pretrig': lambda: dat().crop(10, top_or_bottom='bottom', dimension='pretrig'),
             'elev_without_nmo': lambda: dat(elev=np.zeros(tnum)).elev_correct()}
    assert set(calls) == set(want)
    types = {'ValueError': ValueError, 'ImpdarError': ImpdarError}
    for label, fn in calls.items():
        with kernels_in_numpy(), pytest.raises(types[want[label][0]]) as e:
            fn()
        assert str(e.value) == want[label][1], label
    d = dat()
    d.picks = object()
    with pytest.raises(NotImplementedError):
        d.crop(5)
    with pytest.raises(AttributeError, match='Call nmo first'):
        dat().constant_sample_depth_spacing()


def run_impproc(argv, loaded):
    with patch.object(sys, 'argv', ['impproc'] + argv), patch('impdar_amd.bin.impproc.load', return_value=loaded):
        impproc.main()


def test_impproc_crop_nmo_elev_forward_and_name_outputs():
    dat = MagicMock()
    run_impproc(['crop', 'top', 'pretrig', '0', 'line_raw.mat'], [dat])
    dat.crop.assert_called_with(0.0, top_or_bottom='top', dimension='pretrig')
    dat.save.assert_called_with('line_cropped.mat')
    dat = MagicMock()
    run_impproc(['crop', 'bottom', 'twtt', '3.5', 'x.mat', '-o', 'y.mat'], [dat])
    dat.crop.assert_called_with(3.5, top_or_bottom='bottom', dimension='twtt')
    dat.save.assert_called_with('y.mat')
    with pytest.raises(SystemExit):
        run_impproc(['crop', 'side', 'snum', '3', 'x.mat'], [MagicMock()])
    dat = MagicMock()
    run_impproc(['nmo', '60', '--uice', '1.7e8', '--const_firn_offset', '4', '--rho_profile', 'rho.csv', 'line_raw.mat'], [dat])
    dat.nmo.assert_called_with(60.0, uice=1.7e8, uair=3.0e8, rho_profile='rho.csv')      # the offset is not forwarded
    dat.save.assert_called_with('line_nmo.mat')
    dat = MagicMock()
    run_impproc(['nmo', '10', 'x.mat'], [dat])
    dat.nmo.assert_called_with(10.0, uice=1.69e8, uair=3.0e8, rho_profile=None)
    dat = MagicMock()
    run_impproc(['elev', 'line_raw.mat'], [dat])
    dat.elev_correct.assert_called_with()
    dat.save.assert_called_with('line_elev.mat')


def test_abi_declares_the_new_entry_points():
    from impdar_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'impdar_hip.h')).read()
    for name in ('impdar_row_lerp', 'impdar_row_lerp_dev', 'impdar_col_shift', 'impdar_col_shift_dev'):
        assert name + '(' in header and name in _hip.SIGNATURES
