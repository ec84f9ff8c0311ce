"""The three full ApRES flows on the GPU (bars: the docstring of ``test_apres_flows_cpu.py``).

Parity on ``AF_QC1`` ... ``AF_QC4``: the device's anomaly of the reference's ``HV`` to 8 x ``pa_ref_err``, real and
imaginary part apart, non-finite kinds equal; the filtered image bit for bit SciPy's ``filtfilt`` of the device's own
anomaly; ``cpe_idxs`` the reference's on every row whose ``gap`` exceeds 1000 x ``filt_sens`` (every row); ``cpe``,
``chhvv_cpe`` and ``dphi_dz_cpe`` the gathers of the device's own images, bit for bit; ``e2e1`` to 4 u relative.

Sweeps at the smallest shapes that can break each kernel, against ``apres_flows_ref.py`` (in longdouble, at
``anomaly_bar``, where a sum is involved):
  anomaly   n_thetas 2, 3, 63, 64, 65, 100, 128, 129 at 5 rows: a plain row, one NaN, all NaN, a zero element (that
            element is -inf + NaN j and, having a NaN, is left out of the row mean like any other: NumPy's rule), a
            plain row
  argmin    windows of 1 column, ending at the last column, starting at column 0 and one past a multiple of 64; a tie
            on the real part broken by the imaginary part, a full tie, a NaN in the middle of the window
  filter    13 rows, the least filtfilt takes at order 3; 12 rows is SciPy's ValueError
  gather    index 0 and index m - 1, both with n = 1; more rows than one block
  entries   each result independent of the call before it, equal on a fresh context and through the resident entry
  flow      ``quadpol_processing`` equals the separate calls bit for bit, with and without the gradient

Time difference: ``time_diff_processing`` equals ``phase_diff`` followed by the four host steps bit for bit, with
``AF_TD1``'s wrap count and bed sample; ``single_processing`` equals ``chain`` then ``phase_uncertainty``."""
import contextlib
import ctypes as C
from unittest.mock import patch

import numpy as np
import pytest

import apres_flows_ref as fr
from conftest import golden
from impdar_amd import apres as apm
from impdar_amd import quadpol as qpm
from test_apres_flows_cpu import (QC, TD, U, check_anomaly, check_idxs, qp_holder, run_host_steps, td_args,
                                  td_holder, wraps_of)
from test_kernel_sweeps_cpu import same_bits

pytestmark = pytest.mark.gpu

DT = 1.0e-8
ANOMALY_M = (2, 3, 63, 64, 65, 100, 128, 129)
# (m, c0, c1): one column; ending at the last column; from column 0; from a column past a multiple of 64
WINDOWS = ((8, 3, 4), (8, 7, 8), (8, 0, 8), (8, 2, 6), (70, 0, 70), (70, 65, 70), (70, 69, 70), (130, 65, 130), (130, 129, 130),
           (130, 0, 129), (130, 129 - 64, 129))


def lowpass(of_nyquist=0.1):
    return qpm.lowpass_spec(of_nyquist * 0.5 / DT, 1. / DT)


@contextlib.contextmanager
def fresh_context(hip):
    """A context of its own, in ``_hip.context()``'s place while the block runs: the kernels' scratch starts empty."""
    lib, ctx = hip.load(), C.c_void_p()
    hip.check(lib.impdar_ctx_create(0, C.byref(ctx)), 'impdar_ctx_create')
    try:
        with patch.object(hip, 'context', lambda device=None: ctx):
            yield ctx
    finally:
        lib.impdar_ctx_destroy(ctx)


def image(n, m, seed):
    rng = np.random.RandomState(seed)
    amp = 10. ** (-2. * np.arange(n) / max(n, 2))[:, None]
    return amp * (rng.standard_normal((n, m)) + 1j * rng.standard_normal((n, m)) + (0.3 + 0.2j))


def special_rows(m, seed):
    z = image(5, m, seed)
    z[1, m // 2] = np.nan + 1j
    z[2, :] = np.nan
    z[3, m - 1] = 0.
    return z


def argmin_image(m, seed):
    """16 rows whose filtered anomaly has, in every row: columns 1 and m - 2 equal (a full tie), column m - 1 the
    conjugate of column 0 (equal real parts, opposite imaginary parts)."""
    z = image(16, m, seed)
    z[:, m - 2] = z[:, 1]
    z[:, m - 1] = np.conj(z[:, 0])
    return z


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize('name', QC)
def test_anomaly_parity(hip, name):
    g = golden(name)
    check_anomaly(qpm.power_anomaly(g['HV']), g, 'device')


@pytest.mark.parametrize('name', QC)
def test_filter_index_and_products_parity(hip, name):
    g = golden(name)
    qp = qp_holder(g)
    qpm.rotational_transform(qp, n_thetas=int(g['n_thetas']))
    spec = qpm.lowpass_spec(float(g['Wn']), 1. / float(g['dt']))
    i0, i1 = int(g['idx_start']), int(g['idx_stop'])
    idxs, planes = qpm.find_cpe_host(qp.HV, spec, i0, i1, filtered=True)
    assert same_bits(planes, fr.lowpass_planes(qpm.anomaly_host(qp.HV), spec))
    assert idxs.dtype == np.int32
    np.testing.assert_array_equal(idxs, fr.row_argmin(planes, i0, i1))
    check_idxs(idxs, g)
    if bool(g['products_first']):
        qp.flags.cpe = False
        qpm.coherence2d(qp)
        qpm.phase_gradient2d(qp)
    qpm.find_cpe(qp, Wn=float(g['Wn']))
    np.testing.assert_array_equal(qp.cpe_idxs, idxs)
    assert same_bits(qp.cpe, qp.thetas[idxs].astype(float)) and qp.flags.cpe is True
    assert hasattr(qp, 'chhvv_cpe') == hasattr(qp, 'dphi_dz_cpe') == bool(g['products_first'])
    if bool(g['products_first']):
        rows = np.arange(qp.snum)
        assert same_bits(qp.chhvv_cpe, qp.chhvv[rows, idxs]) and same_bits(qp.dphi_dz_cpe, qp.dphi_dz[rows, idxs])
        assert same_bits(qpm.cpe_gather_host(qp.chhvv, idxs), qp.chhvv_cpe)
        assert same_bits(qpm.cpe_gather_host(qp.dphi_dz, idxs), qp.dphi_dz_cpe)
        qpm.phase_gradient_to_fabric(qp)
        scale = (300e6 / (4. * np.pi * 300e6)) * (2. * np.sqrt(3.12) / 0.035)
        assert (np.abs(qp.e2e1 - scale * qp.dphi_dz_cpe) <= 4 * U * np.abs(qp.e2e1)).all()


# ------------------------------------------------------------------------------------------------ sweeps
@pytest.mark.parametrize('m', ANOMALY_M)
def test_anomaly_sweep(hip, m):
    z = special_rows(m, 40 + m)
    got = qpm.anomaly_host(z)
    want64 = fr.anomaly_planes(z)
    np.testing.assert_array_equal(fr.kinds(got), fr.kinds(want64))
    exact = fr.power_anomaly(z, np.clongdouble)
    exact = np.hstack((exact.real, exact.imag))
    ok = fr.kinds(want64) == 0
    with np.errstate(invalid='ignore'):
        ratio = np.abs(got.astype(np.longdouble) - exact)[ok] / fr.anomaly_bar(z)[ok]
    print('anomaly m %3d: worst |diff| = %.3f of the bar, %d non-finite' % (m, float(ratio.max()), int((~ok).sum())))
    assert ratio.max() <= 1
    # the rows are what the text above says they are
    zero = fr.to_complex(got)[3, m - 1]
    assert np.isneginf(zero.real) and np.isnan(zero.imag) and np.isfinite(got[3, :m - 1]).all()
    assert np.isnan(got[2]).all() and np.isnan(got[1, m // 2]) and np.isfinite(got[[0, 4]]).all()
    assert int(np.isnan(got[1]).sum()) == 2
    assert same_bits(qpm.power_anomaly(z), fr.to_complex(got))


@pytest.mark.parametrize('window', WINDOWS)
def test_argmin_sweep(hip, window):
    m, c0, c1 = window
    z = argmin_image(m, 7 * m)
    idxs, planes = qpm.find_cpe_host(z, lowpass(), c0, c1, filtered=True)
    np.testing.assert_array_equal(idxs, fr.row_argmin(planes, c0, c1))
    assert ((idxs >= c0) & (idxs < c1)).all()
    # the planted columns are what they were meant to be after the filter
    assert same_bits(planes[:, 1], planes[:, m - 2]) and same_bits(planes[:, m + 1], planes[:, 2 * m - 2])
    assert same_bits(planes[:, 0], planes[:, m - 1]) and (planes[:, m] != planes[:, 2 * m - 1]).all()


def test_argmin_ties_and_nan(hip):
    m = 8
    z = argmin_image(m, 5)
    z[:, 1] *= 1e-3                      # columns 1 and 6: the least of every row, equal
    z[:, 6] = z[:, 1]
    idxs, planes = qpm.find_cpe_host(z, lowpass(), 0, m, filtered=True)
    np.testing.assert_array_equal(idxs, fr.row_argmin(planes, 0, m))
    assert (idxs == 1).all()             # a full tie goes to the lower column
    assert (qpm.find_cpe_host(z, lowpass(), 2, m) == 6).all()
    z = argmin_image(m, 5)
    z[:, 0] *= 1e-3                      # columns 0 and 7: equal real parts, the imaginary part decides
    z[:, 7] = np.conj(z[:, 0])
    idxs, planes = qpm.find_cpe_host(z, lowpass(), 0, m, filtered=True)
    np.testing.assert_array_equal(idxs, fr.row_argmin(planes, 0, m))
    assert set(idxs) <= {0, 7} and same_bits(planes[:, 0], planes[:, 7])
    np.testing.assert_array_equal(idxs, np.where(planes[:, m] < planes[:, 2 * m - 1], 0, 7))
    z[9, 4] = np.nan                     # one NaN: the filter spreads it over its column, and the first NaN wins
    z[3, 5] = np.nan + 0j
    idxs, planes = qpm.find_cpe_host(z, lowpass(), 0, m, filtered=True)
    assert np.isnan(planes[:, 4]).all() and np.isnan(planes[:, 5]).all() and np.isfinite(planes[:, :4]).all()
    assert (idxs == 4).all() and (qpm.find_cpe_host(z, lowpass(), 5, m) == 5).all()
    assert (qpm.find_cpe_host(z, lowpass(), 0, 4) < 4).all()


def test_filter_edges(hip):
    z = image(13, 5, 77)
    idxs, planes = qpm.find_cpe_host(z, lowpass(), 1, 4, filtered=True)
    assert same_bits(planes, fr.lowpass_planes(qpm.anomaly_host(z), lowpass()))
    np.testing.assert_array_equal(idxs, fr.row_argmin(planes, 1, 4))
    with pytest.raises(ValueError) as e:
        qpm.find_cpe_host(z[:12], lowpass(), 1, 4)
    assert 'The length of the input vector x must be greater than padlen, which is 12.' in str(e.value)
    for c0, c1 in ((2, 2), (3, 2), (-1, 3), (0, 6)):
        with pytest.raises(ValueError, match='no window'):
            qpm.find_cpe_host(z, lowpass(), c0, c1)


def test_gather_edges(hip):
    rng = np.random.RandomState(9)
    for n, m in ((1, 1), (1, 5), (300, 7)):
        for img in (rng.standard_normal((n, m)), rng.standard_normal((n, m)) + 1j * rng.standard_normal((n, m))):
            for idx in (np.zeros(n, dtype=int), np.full(n, m - 1), rng.randint(0, m, n), np.full(n, -1)):
                got = qpm.cpe_gather_host(img, idx)
                assert same_bits(got, img[np.arange(n), idx]), (n, m, img.dtype)
    with pytest.raises(IndexError):
        qpm.cpe_gather_host(np.zeros((3, 4)), np.array([0, 4, 1]))
    with pytest.raises(IndexError):
        qpm.cpe_gather_host(np.zeros((3, 4)), np.array([0, 1]))


ORDER = ((13, 2, 0, 2), (16, 8, 2, 6), (14, 65, 64, 65), (40, 130, 0, 130))
LARGEST = (257, 129, 3, 120)


def entry_case(case):
    n, m, c0, c1 = case
    return image(n, m, 100 * n + m), lowpass(), c0, c1


def test_entries_do_not_depend_on_the_call_before(hip):
    first = []
    for case in ORDER:
        with fresh_context(hip):
            z = entry_case(case)[0]
            idx = np.arange(case[0]) % case[1]
            first.append((qpm.anomaly_host(z),) + qpm.find_cpe_host(*entry_case(case), filtered=True) + (qpm.cpe_gather_host(z, idx),))
    for case, want in zip(ORDER, first):
        big = entry_case(LARGEST)
        qpm.anomaly_host(big[0]), qpm.find_cpe_host(*big), qpm.cpe_gather_host(big[0], np.zeros(LARGEST[0], dtype=int))
        z = entry_case(case)[0]
        got = (qpm.anomaly_host(z),) + qpm.find_cpe_host(*entry_case(case), filtered=True) + \
            (qpm.cpe_gather_host(z, np.arange(case[0]) % case[1]),)
        assert all(same_bits(a, b) for a, b in zip(got, want)), case


def test_resident_entries_equal_the_host_buffer_forms(hip):
    ctx = hip.context()
    for case in ORDER + (LARGEST,):
        z, spec, c0, c1 = entry_case(case)
        held = [hip.DeviceArray.from_host(ctx, z)]
        try:
            held.append(qpm.anomaly_dev(held[0]))
            held.append(qpm.anomaly_dev(held[0], 1))
            held.extend(qpm.find_cpe_dev(held[0], spec, c0, c1, filtered=True))
            held.append(qpm.find_cpe_dev(held[0], spec, c0, c1))
            held.append(qpm.cpe_gather_dev(held[0], held[3]))
            pa = qpm.anomaly_host(z)
            idxs, planes = qpm.find_cpe_host(z, spec, c0, c1, filtered=True)
            assert same_bits(held[1].to_host(), pa) and same_bits(held[2].to_host(), pa[:1]), case
            assert same_bits(held[3].to_host(), idxs) and same_bits(held[4].to_host(), planes), case
            assert same_bits(held[5].to_host(), idxs) and same_bits(held[6].to_host(), qpm.cpe_gather_host(z, idxs)), case
            ms = qpm.find_cpe_last_ms(ctx)
            assert len(ms) == 3 and all(t >= 0 for t in ms)
        finally:
            for d in held:
                d.free()


@pytest.mark.parametrize('gradient', (False, True))
def test_flow_equals_the_separate_calls(hip, gradient):
    g = golden(QC[0])
    Wn = float(g['Wn'])
    for filt, Wn_gradient in ((None, 0),) + (((('lowpass', Wn),)) if gradient else ()):
        one, sep = qp_holder(g), qp_holder(g)
        qpm.quadpol_processing(one, nthetas=24, Wn=Wn, gradient=gradient, filt=filt, Wn_gradient=Wn_gradient)
        qpm.rotational_transform(sep, n_thetas=24)
        qpm.find_cpe(sep, Wn=Wn)
        qpm.coherence2d(sep)
        names = ['thetas', 'HH', 'HV', 'VH', 'VV', 'cpe_idxs', 'cpe', 'chhvv', 'chhvv_cpe']
        if gradient:
            qpm.phase_gradient2d(sep, filt=filt, Wn=Wn_gradient)
            qpm.phase_gradient_to_fabric(sep)
            names += ['dphi_dz', 'dphi_dz_cpe', 'e2e1']
        assert sorted(vars(one)) == sorted(vars(sep))
        for k in names:
            assert same_bits(getattr(one, k), getattr(sep, k)), k
        for k in ('rotation', 'coherence', 'phasegradient', 'cpe'):
            np.testing.assert_array_equal(getattr(one.flags, k), getattr(sep.flags, k))
        assert hasattr(one, 'e2e1') == gradient and one.flags.cpe is True
    check_idxs(one.cpe_idxs, g)


# ------------------------------------------------------------------------------------------------ time difference
@pytest.mark.parametrize('name', TD)
def test_time_diff_flow_equals_its_steps(hip, name):
    g = golden(name)
    win, step, thresh, strain_window, w_surf, uncertainty = td_args(g)
    sep = td_holder(g)
    apm.phase_diff(sep, win, step)
    run_host_steps(sep, g)
    assert wraps_of(sep.phi, sep.co) == int(g['wraps']) and sep.bed[0] == g['bed'][0]
    if uncertainty == 'noise_phasor':                        # the flow's own choice
        one = td_holder(g)
        apm.time_diff_processing(one, win=win, step=step, thresh=thresh, strain_window=strain_window, w_surf=w_surf)
        for k in ('ds', 'co', 'phi', 'w', 'bed') + (('w_err',) if bool(g['with_unc']) else ()):
            assert same_bits(getattr(one, k), getattr(sep, k)), k
        assert one.eps_zz == sep.eps_zz and one.w0 == sep.w0
        assert wraps_of(one.phi, one.co) == int(g['wraps']) and one.bed[0] == g['bed'][0]


def test_single_processing_is_chain_then_uncertainty(hip):
    g = golden('AP_A4_pow2_3x2x1024_p1')

    def holder():
        dat = apm.Apres()
        dat.data = g['raw'].copy()
        dat.bnum, dat.cnum, dat.snum = dat.data.shape
        for k in g:
            if k.startswith('header_'):
                setattr(dat.header, k[7:], float(g[k]))
        return dat
    one, sep = holder(), holder()
    bed = float(np.median(g['Rcoarse']))
    np.random.seed(3)
    with np.errstate(invalid='ignore'):
        apm.single_processing(one, p=int(g['p']), max_range=float(g['max_range']), noise_bed_range=bed)
    apm.chain(sep, int(g['p']), float(g['max_range']))
    np.random.seed(3)
    with np.errstate(invalid='ignore'):
        apm.phase_uncertainty(sep, bed)
    assert one.data.shape == (1, 1, int(g['snum'])) and one.flags.uncertainty is True
    for k in ('data', 'spec', 'Rcoarse', 'Rfine', 'uncertainty'):
        assert same_bits(getattr(one, k), getattr(sep, k)), k
    assert one.uncertainty.shape == (int(g['snum']),) and np.isfinite(one.uncertainty).any()
