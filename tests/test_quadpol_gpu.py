"""The quad-pol chain on the GPU: every ``Q*`` fixture through the three Python functions at the bars of
``test_quadpol_cpu.py`` (rotation 8 u (|shh| + |shv| + |svh| + |svv|); chhvv 4 N u, N = 4 nrange ntheta, NaN positions
equal; dphi_dz against the reference's formula on the device's own chhvv, 8 x the fixture's ``dphi_ref_err``); the
resident chain against the three calls bit for bit; the ``coherence2d`` symbol on padded arrays against the periodic
form; what the hook does when it can do nothing; the resident forms back to back."""
import numpy as np
import pytest

import quadpol_ref as ref
from conftest import golden
from impdar_amd import quadpol as qpm
from test_quadpol_cpu import CASES, call_args, check_coherence, check_gradient, check_rotation, holder

pytestmark = pytest.mark.gpu


def run_steps(g):
    n_thetas, delta_theta, delta_range, filt, Wn = call_args(g)
    qp = holder(g)
    qpm.rotational_transform(qp, n_thetas=n_thetas)
    qpm.coherence2d(qp, delta_theta=delta_theta, delta_range=delta_range)
    qpm.phase_gradient2d(qp, filt=filt, Wn=Wn)
    return qp


@pytest.fixture(scope='module')
def q1_steps(hip):
    return run_steps(golden(CASES[0]))


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('name', CASES)
def test_steps_match_the_reference(hip, name):
    g = golden(name)
    qp = run_steps(g)
    check_rotation(qp, g)
    check_coherence(qp, g)
    check_gradient(qp, g)


@pytest.mark.parametrize('name', [CASES[0], CASES[4], CASES[6]])
def test_chain_equals_the_three_calls_bit_for_bit(hip, name):
    g = golden(name)
    n_thetas, delta_theta, delta_range, filt, Wn = call_args(g)
    want = run_steps(g)
    qp = holder(g)
    qpm.chain(qp, n_thetas=n_thetas, delta_theta=delta_theta, delta_range=delta_range, filt=filt, Wn=Wn)
    for k in ('thetas', 'HH', 'HV', 'VH', 'VV', 'chhvv', 'dphi_dz'):
        assert same_bits(getattr(qp, k), getattr(want, k)), k
    for k in ('rotation', 'coherence'):
        np.testing.assert_array_equal(getattr(qp.flags, k), getattr(want.flags, k))
    assert qp.flags.phasegradient is True


def test_symbol_on_padded_arrays_equals_the_periodic_form(hip, q1_steps):
    g = golden(CASES[0])
    nrange, pad = int(g['nrange']), int(g['ntheta'])
    HH_, VV_ = [np.ascontiguousarray(np.hstack((x[:, -pad:], x, x[:, :pad]))) for x in (q1_steps.HH, q1_steps.VV)]
    sentinel = 12.5 - 0.25j
    chhvv = np.full(HH_.shape, sentinel)
    out = qpm.coherence2d_loop(chhvv, HH_, VV_, nrange, pad, HH_.shape[0], HH_.shape[1])
    assert out is not chhvv and same_bits(out, chhvv)
    assert same_bits(np.ascontiguousarray(chhvv[:, pad:-pad]), q1_steps.chhvv)
    assert (chhvv[:, :pad] == sentinel).all() and (chhvv[:, -pad:] == sentinel).all()
    # the status-code form on the same arrays
    assert same_bits(qpm.coherence_host(HH_, VV_, nrange, pad, wrap=False), q1_steps.chhvv)


def test_hook_with_nothing_to_do_says_so(hip, capfd):
    """range_bins = 0 leaves no row to write; nrange = 0 leaves the rows: NaN in the columns the hook writes, the
    pads untouched.  One line on stderr each, and no work for the device (the sizes are checked first)."""
    sentinel = 3. + 4.j
    chhvv = np.full((6, 9), sentinel)
    HH = np.ones((6, 9), dtype=np.complex128)
    capfd.readouterr()
    out = qpm.coherence2d_loop(chhvv, HH, HH.copy(), 3, 2, 0, 9)
    err = capfd.readouterr().err
    assert err.count('\n') == 1 and 'coherence2d' in err
    assert (chhvv == sentinel).all() and (out == sentinel).all()
    qpm.coherence2d_loop(chhvv, HH, HH.copy(), 0, 2, 6, 9)
    err = capfd.readouterr().err
    assert err.count('\n') == 1 and 'coherence2d' in err
    assert np.isnan(chhvv[:, 2:7].real).all() and np.isnan(chhvv[:, 2:7].imag).all()
    assert (chhvv[:, :2] == sentinel).all() and (chhvv[:, 7:] == sentinel).all()


def test_resident_coherence_follows_resident_rotation_unsynchronised(hip, q1_steps):
    """``*_dev`` rotation, then ``*_dev`` coherence and phase gradient of its images with no host synchronisation in
    between: the stream orders them."""
    g = golden(CASES[0])
    qp = holder(g)
    vectors, thetas, cos2, sincos, sin2 = qpm.rotation_tables(qp, 0, np.pi, int(g['n_thetas']), False, False, False)
    ctx = hip.context()
    d_vec = [hip.DeviceArray.from_host(ctx, v) for v in vectors]
    images = qpm.rotate_dev(d_vec, cos2, sincos, sin2)
    d_chhvv = qpm.coherence_dev(images[0], images[3], int(g['nrange']), int(g['ntheta']))
    d_dphi = qpm.phase_gradient_dev(d_chhvv, qpm.gradient_coefficients(g['range']))
    assert d_chhvv.shape == q1_steps.chhvv.shape and d_chhvv.dtype == np.complex128
    assert same_bits(d_chhvv.to_host(), q1_steps.chhvv)
    assert same_bits(d_dphi.to_host(), q1_steps.dphi_dz)
    assert same_bits(images[1].to_host(), q1_steps.HV)
    for d in d_vec + list(images) + [d_chhvv, d_dphi]:
        d.free()


def test_bad_windows_are_errors_of_the_library(hip):
    HH = np.ones((8, 6), dtype=np.complex128)
    for nrange, ntheta, wrap in ((0, 1, True), (1, 0, True), (1, 7, True), (1, 3, False)):
        with pytest.raises(ValueError):
            qpm.coherence_host(HH, HH, nrange, ntheta, wrap=wrap)
    assert qpm.coherence_host(HH, HH, 1, 6, wrap=True).shape == (8, 6)
    assert qpm.coherence_host(HH, HH, 1, 2, wrap=False).shape == (8, 2)
