"""ApRES range conversion, stacking and phase difference without a GPU: the NumPy restatement in ``apres_ref.py``
reproduces every ``AP_*`` fixture of the reference at the bars the device is held to, and the host logic -- tables, the
crop, shapes, flags, the reference's errors, the holders -- runs with the kernels replaced by that restatement.

The bars (u = 2**-53):
  spec, data   every kept bin of every chirp: |diff| <= E = 64 u log2(N) ||reference spectrum of that chirp||_2
               (``apres_ref.spectrum_bar``)
  Rfine        every bin: |diff| |den_k| <= E / |data_k| + 8 u
  Rcoarse, phiref, shapes, dtypes, flags, snum: equal
  stacking     bit for bit
  co           |diff| <= 4 W u, W = 2 (win // 2) terms; NaN positions and ds equal
"""
import contextlib
import copy
import ctypes
import os
from unittest.mock import patch

import numpy as np
import pytest

import apres_ref as ref
from conftest import ROOT, golden, golden_names
from impdar_amd import apres as apm

RANGE = golden_names('AP_A')
RANGE.remove('AP_AZ_errors')
STACK = golden_names('AP_S')
DIFF = golden_names('AP_P')


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------- NumPy stand-ins for the kernels
@contextlib.contextmanager
def kernels_in_numpy():
    with patch.object(apm, 'range_host', ref.range_rows), patch.object(apm, 'stack_host', ref.stack), \
            patch.object(apm, 'phase_diff_host', ref.phase_diff):
        yield


# ------------------------------------------------------------------------------------------- fixture plumbing
def holder(g, data=None):
    dat = apm.Apres()
    dat.data = (g['raw'] if data is None else data).copy()
    dat.bnum, dat.cnum, dat.snum = dat.data.shape
    for k in g:
        if k.startswith('header_'):
            setattr(dat.header, k[7:], float(g[k]))
    return dat


def range_args(g):
    return int(g['p']), float(g['max_range']), g['winfun'].item()


def run_range(g):
    dat = holder(g)
    p, max_range, winfun = range_args(g)
    apm.apres_range(dat, p, max_range, winfun=winfun)
    return dat


def check_range(dat, g):
    p, max_range, winfun = range_args(g)
    bnum, cnum, snum = g['raw'].shape
    N, nf = p * snum, (p * snum) // 2
    n = int(g['snum'])
    t = apm.range_tables(holder(g), p, max_range, winfun)
    assert t.n == n and t.nf == nf
    assert dat.snum == n and dat.data_dtype == np.complex128 == np.dtype(g['data_dtype'].item())
    assert dat.flags.range == max_range == float(g['flags_range'])
    assert same_bits(dat.Rcoarse, g['Rcoarse']) and same_bits(dat.phiref, g['phiref'])
    assert dat.Rcoarse.shape == (n,) and dat.phiref.shape == (nf,)
    E = ref.spectrum_bar(N, g['spec_norm']).reshape(bnum, cnum, 1)
    for k in ('spec', 'data'):
        got = getattr(dat, k)
        assert got.dtype == np.complex128 and got.shape == (bnum, cnum, n) == g[k].shape
        if n:
            ratio = float(np.max(np.abs(got - g[k]) / E))
            print('%s: max |diff| / E = %.3e' % (k, ratio))
            assert ratio <= 1.0, k
    assert dat.Rfine.dtype == np.float64 and dat.Rfine.shape == (min(bnum, n), cnum, nf) == g['Rfine'].shape
    if n:
        # |data_k| of every bin, the ones beyond the crop too: the restatement's, which the kept bins pin to the reference
        rows = g['raw'].reshape(-1, snum)
        mag = np.abs(np.fft.rfft((rows - rows.mean(axis=1, keepdims=True)) * t.win, N, axis=1)[:, :nf] * t.scale_mul / t.scale_div)
        mag = mag.reshape(bnum, cnum, nf)[:n]
        bar = E[:n] / mag + 8 * ref.U
        assert float(np.max(E[:n] / mag)) < 1e-8
        ratio = float(np.max(np.abs(dat.Rfine - g['Rfine']) * np.abs(t.den) / bar))
        print('Rfine: max |diff| |den| / bar = %.3e' % ratio)
        assert ratio <= 1.0


def stack_holder(g):
    dat = apm.Apres()
    dat.data = g['data_in'].copy()
    dat.bnum, dat.cnum, dat.snum = dat.data.shape
    return dat, (None if int(g['num_chirps']) < 0 else int(g['num_chirps']))


def check_stack(dat, g):
    assert same_bits(dat.data, g['data'])
    assert (dat.bnum, dat.cnum) == (int(g['bnum']), int(g['cnum']))
    assert dat.flags.stack == int(g['flags_stack']) and isinstance(dat.flags.stack, int)


def diff_holder(g):
    diff = apm.TimeDiff()
    diff.data, diff.data2, diff.range = g['data'].copy(), g['data2'].copy(), g['range'].copy()
    diff.snum = len(diff.data)
    return diff, int(g['win']), int(g['step']), (g['range_ext'] if 'range_ext' in g else None)


def check_diff(diff, g):
    want = g['co']
    assert diff.co.dtype == np.complex128 and diff.co.shape == want.shape
    np.testing.assert_array_equal(np.isnan(diff.co.real), np.isnan(want.real))
    np.testing.assert_array_equal(np.isnan(diff.co.imag), np.isnan(want.imag))
    ok = ~np.isnan(want.real)
    bar = 4 * 2 * (int(g['win']) // 2) * ref.U
    err = float(np.max(np.abs(diff.co[ok] - want[ok])))
    print('co: max |diff| = %.3e, bar %.3e' % (err, bar))
    assert err <= bar
    assert same_bits(diff.ds, g['ds'])
    np.testing.assert_array_equal(diff.flags.phase_diff, g['flags_phase_diff'])


# ------------------------------------------------------------------------------------------------ the tests
def test_fixtures_cover_the_cases():
    gs = {n[3:5]: golden(n) for n in RANGE + STACK + DIFF}
    assert sorted(gs) == ['A1', 'A2', 'A3', 'A4', 'A5', 'A6', 'A7', 'P1', 'P2', 'P3', 'P4', 'S1', 'S2', 'S3']
    shape = lambda g: g['raw'].shape + (int(g['p']), int(g['snum']))      # noqa: E731
    assert shape(gs['A1']) == (2, 3, 1001, 2, 714) == shape(gs['A7']) and gs['A7']['winfun'].item() == 'hanning'
    assert shape(gs['A2'])[:4] == (1, 4, 362, 3) and 0 < int(gs['A2']['snum']) < 543
    assert shape(gs['A3'])[:4] == (3, 2, 1001, 1) and shape(gs['A4']) == (3, 2, 1024, 1, 238)
    assert shape(gs['A5']) == (1, 4, 362, 3, 0) and gs['A5']['Rfine'].shape == (0, 4, 543)
    assert shape(gs['A6']) == (5, 2, 64, 1, 3) and gs['A6']['Rfine'].shape == (3, 2, 32)
    assert gs['A1']['Rfine'].shape == (2, 3, 1001)
    for k in ('A1', 'A2', 'A3', 'A4', 'A6', 'A7'):
        assert 0 < float(gs[k]['ref_err']) < 8, k
    assert gs['S1']['data'].shape == (4, 1, 300) and gs['S2']['data'].shape == (1, 1, 300)
    assert gs['S3']['data'].shape == (1, 1, 714) and gs['S3']['data'].dtype == np.complex128
    assert (int(gs['P2']['win']), int(gs['P2']['step'])) == (21, 1)
    nan = np.isnan(gs['P3']['co'].real)
    assert nan.any() and not nan.all() and not any(np.isnan(gs[k]['co']).any() for k in ('P1', 'P2', 'P4'))
    assert 'range_ext' in gs['P4']
    for n in RANGE + STACK + DIFF + ['AP_AZ_errors']:
        assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', n + '.npz')) < 1 << 20


@pytest.mark.parametrize('name', RANGE)
def test_range_restatement_reproduces_the_reference(name):
    g = golden(name)
    with kernels_in_numpy():
        dat = run_range(g)
    check_range(dat, g)


@pytest.mark.parametrize('name', STACK)
def test_stack_restatement_reproduces_the_reference(name):
    g = golden(name)
    dat, num_chirps = stack_holder(g)
    with kernels_in_numpy():
        apm.stacking(dat, num_chirps)
    check_stack(dat, g)


@pytest.mark.parametrize('name', DIFF)
def test_phase_diff_restatement_reproduces_the_reference(name):
    g = golden(name)
    diff, win, step, range_ext = diff_holder(g)
    with kernels_in_numpy():
        apm.phase_diff(diff, win, step, range_ext=range_ext)
    check_diff(diff, g)


def test_errors_are_the_references():
    e = golden('AP_AZ_errors')
    want = {lab: (typ, msg) for lab, typ, msg in zip(e['label'], e['exc_type'], e['message'])}
    g = {'raw': e['raw']}
    g.update({'header_' + k: v for k, v in dict(bandwidth=2.e8, fc=3.e8, chirp_grad=2. * np.pi * 2.e8, ci=1.68e8,
                                                lambdac=0.56).items()})
    with kernels_in_numpy():
        dat = holder(g)
        apm.apres_range(dat, 1, 10.)
        with pytest.raises(TypeError) as exc:
            apm.apres_range(dat, 1, 10.)
        assert want['range_twice'] == ('TypeError', str(exc.value))
        with pytest.raises(TypeError) as exc:
            apm.apres_range(holder(g), 1, 10., winfun='boxcar')
        assert want['window_unknown'] == ('TypeError', str(exc.value))
        assert want['window_kaiser'][0] == 'TypeError'
        with pytest.raises(TypeError):
            apm.apres_range(holder(g), 1, 10., winfun='kaiser')


def test_holders_carry_the_references_defaults():
    dat, diff = apm.Apres(), apm.TimeDiff()
    assert dat.flags.range == 0 and dat.flags.stack == 0 and dat.flags.uncertainty is False
    assert dat.flags.attrs == ['file_read_code', 'range', 'stack', 'uncertainty']
    assert diff.flags.phase_diff is False and diff.flags.unwrap is False and diff.flags.bed_pick is False
    np.testing.assert_array_equal(diff.flags.strain, np.zeros(2))
    assert dat.header.fs == 4e4 and dat.header.fsysclk == 1e9 and dat.header.ci is None
    for k in ('data', 'spec', 'Rcoarse', 'Rfine', 'phiref', 'snum', 'cnum', 'bnum'):
        assert getattr(dat, k) is None
    for k in ('data', 'data2', 'range', 'ds', 'co'):
        assert getattr(diff, k) is None


def test_phase2range_takes_the_references_branches():
    g = golden(RANGE[0])
    dat = holder(g)
    phi = np.linspace(-3, 3, 7)
    lam, K, ci = dat.header.lambdac, dat.header.chirp_grad, dat.header.ci
    rc = np.arange(7) * 10.
    first = lam * phi / (4. * np.pi)
    assert same_bits(apm.phase2range(dat, phi), first)
    assert same_bits(apm.phase2range(dat, phi, lam, rc, None, ci), first)
    assert same_bits(apm.phase2range(dat, phi, lam, None, K, ci), first)
    assert same_bits(apm.phase2range(dat, phi, lam, rc, K, ci), phi / ((4. * np.pi / lam) - (4. * rc * K / ci**2.)))
    # a header without a chirp gradient sends the range conversion down the first-order branch
    dat.header.chirp_grad = 0.
    t = apm.range_tables(dat, 2, 150.)
    assert t.first_order and same_bits(t.den, np.full(1001, 4. * np.pi))
    with kernels_in_numpy():
        apm.apres_range(dat, 2, 150.)
    t_all = copy.copy(t)
    t_all.n = t.nf
    data_all = ref.range_rows(g['raw'].reshape(6, 1001), t_all)[1].reshape(2, 3, 1001)
    assert same_bits(dat.Rfine, lam * np.angle(data_all) / (4. * np.pi))


def test_raw_data_of_any_real_dtype_is_widened_on_the_host():
    g = golden('AP_A6_n3_below_bnum_5x2x64_p1')
    counts = np.round(g['raw'] * 1000).astype(np.int16)
    with kernels_in_numpy():
        a, b = holder(g, counts), holder(g, counts.astype(np.float64))
        apm.apres_range(a, 1, 1.)
        apm.apres_range(b, 1, 1.)
    assert same_bits(a.data, b.data) and same_bits(a.Rfine, b.Rfine)
    with pytest.raises(TypeError):
        apm.raw_rows(holder(g, g['raw'] + 0j))
    bad = holder(g)
    bad.cnum = 3
    with pytest.raises(ValueError):
        apm.raw_rows(bad)


def test_stack_plan_follows_the_references_branches():
    assert apm.stack_plan(4, 5, None) == (20, 1, 20, False)
    assert apm.stack_plan(4, 5, 5) == (5, 4, 5, True)
    assert apm.stack_plan(4, 5, 7.9) == (7, 1, 7, False)
    assert apm.stack_plan(4, 5, 50) == (50, 1, 20, False)       # the reference's slice stops at the chirps there are
    assert apm.stack_plan(1, 5, None) == (5, 1, 5, True)
    with pytest.raises(ValueError):
        apm.stack_plan(4, 5, 0)


def test_stacking_after_an_empty_crop_stays_empty():
    g = golden('AP_A5_all_within_n0_1x4x362_p3')
    with kernels_in_numpy():
        dat = run_range(g)
        apm.stacking(dat)
    assert dat.data.shape == (1, 1, 0) and dat.data.dtype == np.complex128 and dat.flags.stack == 4


def test_phase_diff_windows_and_refusals():
    assert list(apm.phase_diff_windows(30, 21, 4)) == [10, 14, 18]
    assert len(apm.phase_diff_windows(10, 20, 1)) == 0
    diff = apm.TimeDiff()
    diff.data = diff.data2 = np.ones(30, dtype=complex)
    diff.range = np.arange(30.)
    with pytest.raises(TypeError):
        apm.phase_diff(diff, 4.5, 1)
    with pytest.raises(ValueError):
        apm.phase_diff_host(np.ones((3, 4)), np.ones((3, 4)), 2, 1)


def test_abi_exports_the_apres_entries():
    from impdar_amd import _hip
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ('impdar_apres_range', 'impdar_apres_stack', 'impdar_apres_phase_diff'):
        for suffix in ('', '_dev'):
            assert hasattr(lib, name + suffix) and name + suffix in _hip.SIGNATURES
    assert len(_hip.SIGNATURES['impdar_apres_range'][1]) == len(_hip.SIGNATURES['impdar_apres_range_dev'][1]) == 17
