"""The quad-pol chain without a GPU: the NumPy restatement in ``quadpol_ref.py`` reproduces every ``Q*`` fixture of the
reference at the bars the device is held to (rotation: 8 u (|shh| + |shv| + |svh| + |svv|) elementwise; chhvv:
4 N u with N = 4 nrange ntheta, NaN positions equal; dphi_dz: 8 x the fixture's ``dphi_ref_err`` of max|expected|);
the host logic -- azimuth factors, window arithmetic, flags, the reference's errors, the cpe gathers -- with the kernels
replaced by that restatement; the type checks of ``coherence2d_loop``; the new symbols of the C ABI."""
import contextlib
import ctypes
import os
from unittest.mock import patch

import numpy as np
import pytest

import quadpol_ref as ref
from conftest import ROOT, golden, golden_names
from impdar_amd import quadpol as qpm
from impdar_amd.lib.ImpdarError import ImpdarError

CASES = [n for n in golden_names('Q') if n != 'QZ_errors']
IMAGES = ('HH', 'HV', 'VH', 'VV')


# ------------------------------------------------------------------------------- NumPy stand-ins for the kernels
@contextlib.contextmanager
def kernels_in_numpy():
    with patch.object(qpm, 'rotate_host', ref.rotate), patch.object(qpm, 'coherence_host', ref.coherence), \
            patch.object(qpm, 'phase_gradient_host', ref.dphi_dz_from_tables):
        yield


# ------------------------------------------------------------------------------------------- fixture plumbing
def holder(g, cpe=False):
    qp = qpm.QuadPol()
    qp.shh, qp.shv, qp.svh, qp.svv = [g['in_' + k].copy() for k in ('shh', 'shv', 'svh', 'svv')]
    qp.range = g['range'].copy()
    qp.snum = len(qp.range)
    qp.dt = float(g['dt'])
    qp.flags.cpe = cpe
    return qp


def call_args(g):
    filt = g['filt'].item() or None
    return int(g['n_thetas']), float(g['delta_theta']), float(g['delta_range']), filt, float(g['Wn'])


def spec_of(g):
    filt = g['filt'].item()
    return qpm.lowpass_spec(float(g['Wn']), 1. / float(g['dt'])) if filt else None


def rotation_bar(g):
    return 8 * ref.U * sum(np.abs(g['in_' + k]) for k in ('shh', 'shv', 'svh', 'svv'))[:, None]


def chhvv_bar(g):
    return 4 * ref.n_terms(int(g['nrange']), int(g['ntheta'])) * ref.U


def check_rotation(qp, g):
    np.testing.assert_array_equal(qp.thetas, g['thetas'])
    for k in IMAGES:
        got = getattr(qp, k)
        assert got.dtype == np.complex128 and got.shape == (len(g['range']), int(g['n_thetas']))
        if k in g:
            assert (np.abs(got - g[k]) <= rotation_bar(g)).all(), k
    np.testing.assert_array_equal(qp.flags.rotation, g['flags_rotation'])


def check_coherence(qp, g):
    want = g['chhvv']
    assert qp.chhvv.dtype == np.complex128 and qp.chhvv.shape == want.shape
    np.testing.assert_array_equal(np.isnan(qp.chhvv.real), np.isnan(want.real))
    np.testing.assert_array_equal(np.isnan(qp.chhvv.imag), np.isnan(want.imag))
    ok = ~np.isnan(want.real)
    err = float(np.max(np.abs(qp.chhvv[ok] - want[ok])))
    print('chhvv: max|diff| = %.3e, bar %.3e' % (err, chhvv_bar(g)))
    assert err <= chhvv_bar(g)
    np.testing.assert_array_equal(qp.flags.coherence, g['flags_coherence'])


def check_gradient(qp, g):
    """dphi_dz against the reference's formula on the chhvv it was made from."""
    want = ref.dphi_dz(qp.chhvv, g['range'], spec_of(g))
    assert qp.dphi_dz.dtype == np.float64 and qp.dphi_dz.shape == want.shape
    err = ref.rel_err(qp.dphi_dz, want)
    print('dphi_dz: max|diff| / max|expected| = %.3e = %.2f x dphi_ref_err' % (err, err / max(float(g['dphi_ref_err']), 1e-300)))
    assert err <= 8 * float(g['dphi_ref_err'])
    assert qp.flags.phasegradient is True and bool(g['flags_phasegradient'])


# ------------------------------------------------------------------------------------------------ the tests
def test_fixtures_cover_the_cases():
    gs = {n[:2]: golden(n) for n in CASES}
    assert sorted(gs) == ['Q1', 'Q2', 'Q3', 'Q4', 'Q5', 'Q6', 'Q7']
    shape = lambda g: (len(g['range']), int(g['n_thetas']), int(g['nrange']), int(g['ntheta']))      # noqa: E731
    assert shape(gs['Q1']) == (257, 24, 23, 2) and shape(gs['Q4']) == (400, 40, 95, 10)
    assert shape(gs['Q2'])[:3] == (64, 8, 100) and shape(gs['Q3']) == (130, 5, 1, 5)
    assert shape(gs['Q5']) == shape(gs['Q1']) == shape(gs['Q7']) and shape(gs['Q6'])[:2] == (1200, 40)
    nan = np.isnan(gs['Q5']['chhvv'].real)
    assert nan.any() and not nan.all() and not any(np.isnan(gs[k]['chhvv']).any() for k in gs if k != 'Q5')
    for k in ('shh', 'svv'):
        assert not gs['Q5']['in_' + k][90:170].any() and gs['Q5']['in_' + k][:90].all()
    assert gs['Q7']['filt'].item() == 'lowpass' and float(gs['Q7']['Wn']) == 0.1 * 0.5 / float(gs['Q7']['dt'])
    # both rules of numpy.gradient
    uniform = {k: qpm.gradient_coefficients(g['range'])[0] for k, g in gs.items()}
    assert uniform['Q2'] and not uniform['Q4'] and not uniform['Q1']
    for k, g in gs.items():
        assert 0 <= float(g['dphi_ref_err']) < 1e-15, k
    for n in CASES + ['QZ_errors']:
        assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', n + '.npz')) < 1 << 20


@pytest.mark.parametrize('name', CASES)
def test_restatement_reproduces_the_reference(name):
    g = golden(name)
    n_thetas = int(g['n_thetas'])
    thetas = np.linspace(0, np.pi, n_thetas)
    vectors = [g['in_' + k] for k in ('shh', 'shv', 'svh', 'svv')]
    images = dict(zip(IMAGES, ref.rotate(vectors, np.cos(thetas)**2., np.sin(thetas) * np.cos(thetas), np.sin(thetas)**2)))
    for k in IMAGES:
        if k in g:
            assert (np.abs(images[k] - g[k]) <= rotation_bar(g)).all(), k
    chhvv = ref.coherence(images['HH'], images['VV'], int(g['nrange']), int(g['ntheta']))
    np.testing.assert_array_equal(np.isnan(chhvv), np.isnan(g['chhvv']))
    ok = ~np.isnan(g['chhvv'])
    assert np.max(np.abs(chhvv[ok] - g['chhvv'][ok])) <= chhvv_bar(g)
    # the padded form is the periodic one on the columns it writes
    pad = int(g['ntheta'])
    padded = [np.hstack((x[:, -pad:], x, x[:, :pad])) for x in (images['HH'], images['VV'])]
    np.testing.assert_array_equal(ref.coherence(padded[0], padded[1], int(g['nrange']), pad, wrap=False), chhvv)
    for form in (ref.dphi_dz(g['chhvv'], g['range'], spec_of(g)),
                 ref.dphi_dz_from_tables(g['chhvv'], qpm.gradient_coefficients(g['range']), spec_of(g))):
        assert ref.rel_err(form, g['dphi_dz']) <= 8 * float(g['dphi_ref_err'])


@pytest.mark.parametrize('name', CASES)
def test_host_logic_matches_the_reference(name):
    g = golden(name)
    n_thetas, delta_theta, delta_range, filt, Wn = call_args(g)
    qp = holder(g)
    with kernels_in_numpy():
        qpm.rotational_transform(qp, n_thetas=n_thetas)
        check_rotation(qp, g)
        assert qpm.coherence_windows(qp, delta_theta, delta_range) == (int(g['nrange']), int(g['ntheta']))
        qpm.coherence2d(qp, delta_theta=delta_theta, delta_range=delta_range)
        check_coherence(qp, g)
        qpm.phase_gradient2d(qp, filt=filt, Wn=Wn)
        check_gradient(qp, g)
    assert not hasattr(qp, 'chhvv_cpe') and not hasattr(qp, 'dphi_dz_cpe')


def test_holder_and_flags_start_as_the_references():
    qp = qpm.QuadPol()
    for k in ('snum', 'dt', 'range', 'shh', 'shv', 'svh', 'svv', 'thetas', 'HH', 'HV', 'VH', 'VV', 'chhvv', 'dphi_dz'):
        assert getattr(qp, k) is None
    f = qp.flags
    assert f.rotation.shape == (2,) and not f.rotation.any() and f.coherence.shape == (3,) and not f.coherence.any()
    assert f.phasegradient is False and f.cpe is True
    assert f.attrs == ['rotation', 'coherence', 'phasegradient', 'cpe'] and f.attr_dims == [2, 3, None, None]


def test_window_arithmetic_is_the_references():
    qp = holder(golden(CASES[0]))
    with kernels_in_numpy():
        qpm.rotational_transform(qp, n_thetas=24)
    dth, dr = abs(qp.thetas[0] - qp.thetas[1]), abs(qp.range[0] - qp.range[1])
    for delta_theta, delta_range in ((0.349, 100.), (dth, dr), (3 * dth, 7 * dr), (2.999 * dth, 6.999 * dr), (24.5 * dth, 1e4)):
        assert qpm.coherence_windows(qp, delta_theta, delta_range) == (int(delta_range // dr), int(delta_theta // dth))
    for delta_theta, delta_range, word in ((0.5 * dth, 100., 'empty window along azimuth'), (25.5 * dth, 100., 'wider than'),
                                           (0.349, 0.5 * dr, 'empty window along range')):
        with kernels_in_numpy(), pytest.raises(ValueError, match=word):
            qpm.coherence2d(qp, delta_theta=delta_theta, delta_range=delta_range)
        assert qp.chhvv is None and not qp.flags.coherence.any()


def test_errors_are_the_references():
    g = golden('QZ_errors')
    want = {str(l): (str(t), str(m)) for l, t, m in zip(g['label'], g['exc_type'], g['message'])}
    some = golden(CASES[0])

    def rotated():
        qp = holder(some)
        qpm.rotational_transform(qp, n_thetas=12)
        return qp

    def with_coherence():
        qp = rotated()
        qpm.coherence2d(qp)
        return qp

    def flipped(**kw):
        qp = holder(some)
        qp.shh, qp.shv, qp.svh, qp.svv = [g['flipped_' + k].copy() for k in ('shh', 'shv', 'svh', 'svv')]
        qp.range = g['range'].copy()
        qpm.rotational_transform(qp, n_thetas=12, **kw)
        return qp
    calls = {'coherence_before_rotation': lambda: qpm.coherence2d(holder(some)),
             'gradient_before_coherence': lambda: qpm.phase_gradient2d(rotated()),
             'filter_unknown': lambda: qpm.phase_gradient2d(with_coherence(), filt='highpass'),
             'cross_pol_opposite_sign': flipped,
             'flip_force': lambda: qpm.rotational_transform(holder(some), n_thetas=12, flip_force=True)}
    assert set(calls) == set(want)
    types = {'ImpdarError': ImpdarError, 'ValueError': ValueError, 'TypeError': TypeError}
    for label, fn in calls.items():
        with kernels_in_numpy(), pytest.raises(types[want[label][0]]) as e:
            fn()
        assert str(e.value) == want[label][1], label
    # the two flips change the measured vector in place, as the reference does, and rotate what is left
    for which in ('HV', 'VH'):
        with kernels_in_numpy():
            qp = flipped(cross_pol_flip=which)
        np.testing.assert_array_equal(qp.shv, g['flip_%s_shv' % which])
        np.testing.assert_array_equal(qp.svh, g['flip_%s_svh' % which])
        bar = 8 * ref.U * sum(np.abs(g['flipped_' + k]) for k in ('shh', 'shv', 'svh', 'svv'))[:, None]
        assert (np.abs(qp.HH - g['flip_%s_HH' % which]) <= bar).all() and (np.abs(qp.HV - g['flip_%s_HV' % which]) <= bar).all()
    with kernels_in_numpy():
        qp = flipped(cross_pol_exception=True)                       # goes on with the terms as they are
    np.testing.assert_array_equal(qp.svh, g['flipped_svh'])
    assert qp.flags.rotation[0] == 1


def test_nan_edges_and_short_vectors_are_refused():
    qp = holder(golden(CASES[0]))
    with kernels_in_numpy():
        qpm.rotational_transform(qp, n_thetas=24)
        qpm.coherence2d(qp)
        qp.chhvv[:3] = np.nan
        with pytest.raises(NotImplementedError, match='3 NaN rows'):
            qpm.phase_gradient2d(qp, filt='lowpass', Wn=0.05 / qp.dt)
        assert qp.dphi_dz is None and qp.flags.phasegradient is False
        qpm.phase_gradient2d(qp)                                     # unfiltered: the NaN rows just stay NaN
        assert np.isnan(qp.dphi_dz[:4]).all() and np.isfinite(qp.dphi_dz[5:]).all()
        short = holder(golden(CASES[0]))
        short.svv = short.svv[:-1]
        with pytest.raises(ValueError, match='broadcast'):
            qpm.rotational_transform(short, n_thetas=24)


def test_cpe_gathers_follow_the_reference():
    g = golden(CASES[0])
    qp = holder(g, cpe=True)
    with kernels_in_numpy():
        qpm.rotational_transform(qp, n_thetas=24)
        with pytest.raises(AttributeError):                          # the reference's, cpe_idxs not being there
            qpm.coherence2d(qp)
        assert qp.chhvv is not None and not qp.flags.coherence.any()          # ... after chhvv, before the flag (:170-176)
        qp.cpe_idxs = (np.arange(qp.snum) * 7) % 24
        qpm.coherence2d(qp)
        np.testing.assert_array_equal(qp.chhvv_cpe, qp.chhvv[np.arange(qp.snum), qp.cpe_idxs])
        qpm.phase_gradient2d(qp)
        np.testing.assert_array_equal(qp.dphi_dz_cpe, qp.dphi_dz[np.arange(qp.snum), qp.cpe_idxs])
        del qp.cpe_idxs
        with pytest.raises(AttributeError):
            qpm.phase_gradient2d(qp)
        qp.flags.cpe = 1                                             # `is True`, as the reference tests it
        qpm.phase_gradient2d(qp)


def test_coherence2d_loop_takes_what_the_cython_wrapper_takes():
    ok = np.zeros((4, 6), dtype=np.complex128)
    bad = [(None, TypeError), ([[0j] * 6] * 4, TypeError), (ok.astype(np.complex64), ValueError), (ok.real.copy(), ValueError),
           (np.zeros(24, dtype=np.complex128), ValueError), (np.zeros((4, 6, 1), dtype=np.complex128), ValueError),
           (np.zeros((6, 4), dtype=np.complex128).T, ValueError), (np.zeros((4, 12), dtype=np.complex128)[:, ::2], ValueError),
           (np.zeros((3, 6), dtype=np.complex128), ValueError)]
    for arr, exc in bad:
        for pos in range(3):
            args = [ok.copy(), ok.copy(), ok.copy()]
            args[pos] = arr
            with pytest.raises(exc):
                qpm.coherence2d_loop(*args, 2, 1, 4, 6)


def test_hook_refuses_sizes_below_one_before_touching_a_device(capfd):
    """nrange = 0: NaN in the columns it would have written, the pads as they were, one line on stderr."""
    chhvv = np.full((5, 8), 7. - 3.j)
    HH = np.ones((5, 8), dtype=np.complex128)
    capfd.readouterr()
    out = qpm.coherence2d_loop(chhvv, HH, HH.copy(), 0, 2, 5, 8)
    err = capfd.readouterr().err
    assert err.count('\n') == 1 and 'coherence2d' in err and 'NaN' in err
    assert out is not chhvv and np.array_equal(out, chhvv, equal_nan=True)
    assert np.isnan(chhvv[:, 2:6].real).all() and np.isnan(chhvv[:, 2:6].imag).all()
    assert (chhvv[:, :2] == 7. - 3.j).all() and (chhvv[:, 6:] == 7. - 3.j).all()


def test_abi_declares_the_new_entry_points():
    from impdar_amd import _hip, build
    header = open(os.path.join(ROOT, 'include', 'impdar_hip.h')).read()
    for name in ('impdar_qp_rotate', 'impdar_qp_coherence', 'impdar_qp_phase_gradient'):
        for twin in (name, name + '_dev'):
            assert twin + '(' in header and twin in _hip.SIGNATURES
    assert 'void coherence2d(double *chhvv, double *HH, double *VV, int nrange, int ntheta,' in header
    assert list(_hip.HOOKS) == ['coherence2d'] and 'quadpol.hip' in build.SOURCES
    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert hasattr(lib, 'coherence2d')
