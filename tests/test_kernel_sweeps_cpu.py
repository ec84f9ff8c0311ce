"""The quad-pol and ApRES kernel sweeps without a GPU.  Every sweep that ``test_quadpol_sweep_gpu.py`` and
``test_apres_sweep_gpu.py`` run on the device is a function here that takes the implementation under test; this file
hands it the float64 restatements (``quadpol_ref``, ``apres_ref``), which shows that every bar is attainable by a
correct float64 implementation on exactly these inputs and keeps the long-double references of ``sweep_ref.py`` under
test where there is no GPU.

The coherence kernels' order of additions -- box sums over the columns, sums over aligned blocks of ``bk`` rows, a
window as head rows + whole blocks + tail rows -- is restated in NumPy (:func:`coherence_blocks`, with a port of
``qp_block_rows``).  It passes the sweep, it visits all five ``bk``, and each of three planted index slips fails the
sweep: that is the evidence that the bar catches a subtly wrong kernel.

The bars (u = 2**-53):
  chhvv, co    per element |got - want| <= 4 (T + 2) u, T the terms of that element's own window: a sequential sum of T
               non-negative terms is off by at most (T - 1) u relative, the products add 2 u, so by Cauchy-Schwarz the
               numerator is off by at most (T + 2) u sqrt(a b) and the quotient by 2 (T + 2) u to first order; the bar
               is twice that.  NaN positions equal in both parts.
  rotation     8 u (|shh| + |shv| + |svh| + |svv|) per element
  dphi_dz      rel_err against the long-double form <= 8 max(e_ref, 16 u), e_ref the float64 formula's own rel_err
  spec, data   E = apres_ref.spectrum_bar(N, ||spectrum of the chirp||_2) per kept bin
  Rfine        |diff| |den_k| <= E / |data_k| + 8 u (modulo 2 pi: a phase on +-pi may come out on either side) on the
               bins where E / |data_k| < 1e-8
  stacking     bit for bit the row-order sum, and numpy.mean for snum >= 2; (m + 2) u max|x| of the long-double mean
               at snum = 1
"""
import numpy as np
import pytest

import apres_ref
import quadpol_ref
import sweep_ref as sw
from conftest import golden
from impdar_amd import apres as apm
from impdar_amd import quadpol as qpm
from test_apres_cpu import RANGE, holder as apres_holder

U = sw.U
DT = 1.0e-8


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_nan_positions(got, want):
    np.testing.assert_array_equal(np.isnan(got.real), np.isnan(want.real))
    np.testing.assert_array_equal(np.isnan(got.imag), np.isnan(want.imag))


def window_ratio(got, want, terms):
    """max |got - want| / (4 (terms + 2) u) over the elements that are not NaN (0 where there is none)."""
    ok = ~np.isnan(want.real)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - want[ok]) / (4 * (terms[ok] + 2) * U)))


# ------------------------------------------------------------------------------------------------ coherence
def sweep_coherence(fn, n):
    """Every nrange and column case at ``n`` rows; ``fn(HH, VV, nrange, ntheta, wrap)``.  Returns the worst
    |diff| / bar and the number of NaN outputs."""
    worst, nans = 0.0, 0
    for nrange in sw.COH_NRANGE:
        for col, (ncols, ntheta, wrap, _) in enumerate(sw.COH_COLS):
            HH, VV = sw.coherence_inputs(n, col)
            want, terms = sw.coherence_want(n, nrange, col)
            got = fn(HH, VV, nrange, ntheta, wrap)
            where = 'n %d nrange %d cols %s' % (n, nrange, sw.COH_COLS[col])
            assert got.dtype == np.complex128 and got.shape == want.shape == (n, ncols if wrap else ncols - 2 * ntheta), where
            assert_nan_positions(got, want)
            ratio = window_ratio(got, want, terms)
            assert ratio <= 1.0, '%s: |diff| = %.3f of the bar' % (where, ratio)
            worst, nans = max(worst, ratio), nans + int(np.isnan(want.real).sum())
            if n == 1:
                assert np.isnan(want.real).all()
    return worst, nans


def block_rows(nrange):
    """``qp_block_rows`` of ``csrc/quadpol.hip``, line for line."""
    bk = 4
    while bk < 64 and bk * bk < nrange:
        bk *= 2
    return bk


def coherence_blocks(HH, VV, nrange, ntheta, wrap, slip=None, seen=None):
    """The three coherence kernels' additions in their order, in float64.  ``slip`` plants one index error:
    'hi_inclusive' (the window takes row hi too), 'b1_ceil' (the last whole block is ceil(hi / bk)), 'wrap_late'
    (the periodic window starts one column late).  ``seen`` collects the ``bk`` that ran."""
    n, ncols = HH.shape
    nout = ncols if wrap else ncols - 2 * ntheta
    c = (np.arange(nout) - ntheta) % ncols if wrap else np.arange(nout)
    if slip == 'wrap_late' and wrap:
        c = (c + 1) % ncols
    box = np.zeros((4, n, nout))
    for _ in range(2 * ntheta):                                     # qp_box_kernel: column order
        x, y = HH[:, c], VV[:, c]
        box[0] += x.real * y.real + x.imag * y.imag
        box[1] += x.imag * y.real - x.real * y.imag
        box[2] += x.real * x.real + x.imag * x.imag
        box[3] += y.real * y.real + y.imag * y.imag
        c = (c + 1) % ncols
    bk = block_rows(nrange)
    if seen is not None:
        seen.add(bk)
    nblk = (n + bk - 1) // bk
    blk = np.zeros((4, nblk, nout))
    for b in range(nblk):                                           # qp_block_kernel: row order
        for r in range(b * bk, min(b * bk + bk, n)):
            blk[:, b] += box[:, r]
    out = np.empty((n, nout), dtype=np.complex128)
    with np.errstate(invalid='ignore', divide='ignore'):
        for j in range(n):                                          # qp_window_kernel
            lo, hi = max(j - nrange, 0), min(j + nrange, n - 1)
            if slip == 'hi_inclusive':
                hi += 1
            b0, b1 = (lo + bk - 1) // bk, ((hi + bk - 1) // bk if slip == 'b1_ceil' else hi // bk)
            e0, e1 = b0 * bk, b1 * bk
            if b0 >= b1:
                b0 = b1 = 0
                e0 = e1 = hi
            s = np.zeros((4, nout))
            for r in range(lo, e0):
                s += box[:, r]
            for b in range(b0, b1):
                s += blk[:, b]
            for r in range(e1, hi):
                s += box[:, r]
            den = np.sqrt(s[2] * s[3])
            out[j] = np.where(den == 0, np.nan, s[0] / den) + 1j * np.where(den == 0, np.nan, s[1] / den)
    return out


# ------------------------------------------------------------------------------------------------ rotation
ROT_SHAPES = ((1, 1), (1, 300), (257, 1), (3, 100), (85, 3))


def rotation_inputs(n, n_thetas):
    rng = np.random.RandomState(31 * n + n_thetas)
    amp = 10. ** (-3. * np.arange(n) / n)
    vectors = [np.ascontiguousarray(amp * (rng.standard_normal(n) + 1j * rng.standard_normal(n))) for _ in range(4)]
    thetas = np.linspace(0, np.pi, n_thetas)
    return vectors, np.cos(thetas)**2., np.sin(thetas) * np.cos(thetas), np.sin(thetas)**2


def check_rotation(fn, n, n_thetas):
    """``fn(vectors, cos2, sincos, sin2)``; returns the worst |diff| / bar over the four images' parts."""
    vectors, cos2, sincos, sin2 = rotation_inputs(n, n_thetas)
    got = fn(vectors, cos2, sincos, sin2)
    want = sw.rotate_ld(vectors, cos2, sincos, sin2)
    bar = (8 * U * sum(np.abs(v) for v in vectors))[:, None].astype(sw.LD)
    worst = 0.0
    for g, (wr, wi) in zip(got, want):
        assert g.dtype == np.complex128 and g.shape == (n, n_thetas)
        for part, w in ((g.real, wr), (g.imag, wi)):
            ratio = float(np.max(np.abs(part.astype(sw.LD) - w) / bar))
            assert ratio <= 1.0, (n, n_thetas, ratio)
            worst = max(worst, ratio)
    return worst


# ------------------------------------------------------------------------------------------------ phase gradient
GRAD_N = (2, 3, 4, 13, 255, 256, 257)
GRAD_M = (1, 2, 5, 24)
GRAD_FILT_N = (13, 14, 64, 257)
GRAD_FILT_M = (1, 5)


def lowpass():
    return qpm.lowpass_spec(0.1 * 0.5 / DT, 1. / DT)


def gradient_ratio(fn, chhvv, rng_axis, spec=None):
    """``fn(chhvv, grad, spec)`` against the long-double form: rel_err / (8 max(e_ref, 16 u))."""
    grad = qpm.gradient_coefficients(rng_axis)
    exact = quadpol_ref.dphi_dz(chhvv, rng_axis, spec, dtype=sw.LD)
    e_ref = quadpol_ref.rel_err(quadpol_ref.dphi_dz(chhvv, rng_axis, spec).astype(sw.LD), exact)
    got = fn(chhvv, grad, spec)
    assert got.dtype == np.float64 and got.shape == chhvv.shape
    ratio = quadpol_ref.rel_err(got.astype(sw.LD), exact) / (8 * max(e_ref, 16 * U))
    assert ratio <= 1.0, (chhvv.shape, grad[0], spec is not None, ratio)
    return ratio


def sweep_gradient(fn, n):
    """Every m and both range axes at ``n`` rows, unfiltered; the worst ratio."""
    worst = 0.0
    for m in GRAD_M:
        chhvv = sw.coherence_image(n, m, 10 * n + m)
        for jittered in (False, True):
            axis = sw.range_axis(n, jittered)
            # two points have one spacing: numpy.gradient and the table both call the jittered axis uniform there
            assert qpm.gradient_coefficients(axis)[0] is (not jittered or n == 2)
            worst = max(worst, gradient_ratio(fn, chhvv, axis))
    return worst


def sweep_gradient_filtered(fn, n):
    worst = 0.0
    for m in GRAD_FILT_M:
        chhvv = sw.coherence_image(n, m, 20 * n + m)
        for jittered in (False, True):
            worst = max(worst, gradient_ratio(fn, chhvv, sw.range_axis(n, jittered), lowpass()))
    return worst


def check_gradient_refuses_twelve_rows(fn):
    chhvv = sw.coherence_image(12, 5, 12)
    with pytest.raises(ValueError, match='The length of the input vector x must be greater than padlen, which is 12.'):
        fn(chhvv, qpm.gradient_coefficients(sw.range_axis(12, False)), lowpass())


def check_gradient_special_images(fn):
    """One image with a NaN element, one with an exactly zero element (0 / 0 there): NaN where the long-double form
    has it (``rel_err`` asserts the positions), the bar everywhere else."""
    worst = 0.0
    for value in (np.nan, 0.):
        for jittered in (False, True):
            chhvv = sw.coherence_image(13, 5, 99)
            chhvv[6, 2] = value
            exact = quadpol_ref.dphi_dz(chhvv, sw.range_axis(13, jittered), dtype=sw.LD)
            assert np.isnan(exact[6, 2]) and np.isnan(exact).sum() == (3 if np.isnan(value) else 1)
            worst = max(worst, gradient_ratio(fn, chhvv, sw.range_axis(13, jittered)))
    return worst


# ------------------------------------------------------------------------------------------------ phase difference
def sweep_phase_diff(fn, length):
    """Every window and step at ``length`` samples; ``fn(s1, s2, win, step)``.  Returns the worst |diff| / bar, the
    number of NaN windows and the number of cases without a window."""
    s1, s2 = sw.phase_diff_inputs(length)
    worst, nans, empty = 0.0, 0, 0
    for win in sw.PD_WIN:
        for step in sw.PD_STEP:
            want, terms = sw.phase_diff_want(length, win, step)
            got = fn(s1, s2, win, step)
            where = 'len %d win %d step %d' % (length, win, step)
            assert got.dtype == np.complex128, where
            assert got.shape == want.shape == (len(apm.phase_diff_windows(length, win, step)),), where
            if not len(want):
                empty += 1
                continue
            assert_nan_positions(got, want)
            if win in (0, 1):
                assert np.isnan(want.real).all(), where
            ratio = window_ratio(got, want, terms)
            assert ratio <= 1.0, '%s: |diff| = %.3f of the bar' % (where, ratio)
            worst, nans = max(worst, ratio), nans + int(np.isnan(want.real).sum())
    return worst, nans, empty


# ------------------------------------------------------------------------------------------------ range conversion
RANGE_SNUM = (2, 3, 5, 255, 256, 257, 513)
RANGE_P = (1, 2, 3)


def range_case(snum, p):
    """5 chirps of ``snum`` samples and their tables: the header of a fixture, window 'hamming' ('blackman' is
    identically zero at 2 samples), ``max_range`` midway between two bins so that 0 < n < nf whenever nf >= 2
    (``argmin`` returns 0 when every bin is within it)."""
    raw = sw.chirps(snum, 50 * snum + p)

    def tables(max_range):
        return apm.range_tables(apres_holder(golden(RANGE[0]), raw.reshape(1, 5, snum)), p, max_range, 'hamming')
    t = tables(1.)
    if t.nf >= 2:
        k = max(0, int(0.7 * t.nf) - 1)
        t = tables(0.5 * (t.Rcoarse[k] + t.Rcoarse[k + 1]))
        assert t.n == k + 1
    assert t.nf == (p * snum) // 2 and not t.first_order
    return raw, t


def check_range(fn, snum, p, chunk=0):
    """``fn(raw, t, chunk)`` -> (spec, data, Rfine).  Returns the worst ratios (spec and data, Rfine) and the number of
    Rfine bins checked and left out."""
    raw, t = range_case(snum, p)
    want = sw.range_ld(raw, t)
    spec, data, rfine = fn(raw, t, chunk)
    E = apres_ref.spectrum_bar(t.p * snum, want.norm)[:, None]
    worst = 0.0
    for k, got in (('spec', spec), ('data', data)):
        assert got.dtype == np.complex128 and got.shape == (5, t.n) == getattr(want, k).shape
        if t.n:
            worst = max(worst, float(np.max(np.abs(got - getattr(want, k)) / E)))
    assert worst <= 1.0, (snum, p, worst)
    assert rfine.dtype == np.float64 and rfine.shape == (5, t.nf) == want.Rfine.shape
    with np.errstate(divide='ignore', invalid='ignore'):
        slack = E / want.mag
        checked = slack < 1e-8                                     # (0 / 0 is left out as well)
    # which bins are left out is the reference's matter, not the implementation's: none from 3 samples on; of a
    # de-meaned pair of samples under a symmetric window only bin 0, which is zero up to rounding
    if snum >= 3:
        assert checked.all()
    else:
        assert checked[:, 1:].all()
    diff = np.abs(rfine - want.Rfine) * np.abs(t.den)
    diff = np.minimum(diff, np.abs(diff - 2 * np.pi))
    rworst = float(np.max(diff[checked] / (slack[checked] + 8 * U))) if checked.any() else 0.0
    assert rworst <= 1.0, (snum, p, rworst)
    return worst, rworst, int(checked.sum()), int((~checked).sum())


# ------------------------------------------------------------------------------------------------ stacking
STACK_SNUM = (1, 2, 255, 256, 257)
STACK_M = (1, 2, 3, 7, 100)
STACK_GROUPS = (1, 3)


def sweep_stack(fn, snum):
    """``fn(data, groups, m)`` on (groups m + 2, snum) real and complex data: the two last rows must not be read."""
    for m in STACK_M:
        for groups in STACK_GROUPS:
            for is_complex in (False, True):
                rng = np.random.RandomState(snum + 7 * m + groups)
                rows = groups * m + 2
                data = rng.standard_normal((rows, snum)) * 10. ** rng.uniform(-3, 0, size=(rows, 1))
                if is_complex:
                    data = data + 1j * rng.standard_normal((rows, snum))
                data[-2:] = 1e30                                   # a row too many shows in every bit
                got = fn(data, groups, m)
                where = (snum, m, groups, is_complex)
                assert same_bits(got, apres_ref.stack(data, groups, m)), where
                view = data[:groups * m].reshape(groups, m, snum)
                if snum >= 2:
                    assert same_bits(got, np.mean(view, axis=1)), where
                else:
                    # one sample per chirp makes the m-axis contiguous: NumPy sums it pairwise, no longer in row order
                    bar = (m + 2) * U * np.max(np.abs(view))
                    assert np.max(np.abs(got - sw.stack_mean_ld(data, groups, m))) <= bar, where


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize('n', sw.COH_N)
def test_coherence_restatement_and_block_order_pass_the_sweep(n):
    worst, nans = sweep_coherence(quadpol_ref.coherence, n)
    seen = set()
    blocks, _ = sweep_coherence(lambda *a: coherence_blocks(*a, seen=seen), n)
    print('n %3d: restatement %.3f of the bar, block order %.3f, %d NaN outputs' % (n, worst, blocks, nans))
    assert seen == {4, 8, 16, 32, 64}
    assert sorted({block_rows(k) for k in (16, 17, 64, 65, 256, 257, 1024, 1025)}) == [4, 8, 16, 32, 64]
    assert [block_rows(k) for k in (1, 16, 17, 64, 65, 256, 257, 1024, 1025, 5000)] == [4, 4, 8, 8, 16, 16, 32, 32, 64, 64]


@pytest.mark.parametrize('slip', ['hi_inclusive', 'b1_ceil', 'wrap_late'])
def test_coherence_sweep_catches_a_planted_slip(slip):
    """The sweep has to fail for the slipped kernel order, at some n; it stops at the first n that does."""
    caught = None
    for n in sw.COH_N:
        try:
            sweep_coherence(lambda *a: coherence_blocks(*a, slip=slip), n)
        except AssertionError as e:
            caught = str(e).strip().splitlines()[0] if str(e).strip() else 'n %d' % n
            break
    print('%s caught: %s' % (slip, caught))
    assert caught is not None, 'the sweep passes a kernel order with the slip %r: it needs another shape' % slip


def test_coherence_sweep_counts():
    assert len(sw.COH_N) * len(sw.COH_NRANGE) * len(sw.COH_COLS) == 1008
    # windows of exactly whole blocks, windows ending on the ragged last block, n below, at and above bk all occur
    assert any(n < block_rows(r) for n in sw.COH_N for r in sw.COH_NRANGE)
    assert any(n == block_rows(r) for n in sw.COH_N for r in sw.COH_NRANGE)
    assert any(n % block_rows(r) for n in sw.COH_N for r in sw.COH_NRANGE)


@pytest.mark.parametrize('shape', ROT_SHAPES)
def test_rotation_restatement(shape):
    print('rotation %s: %.3f of the bar' % (shape, check_rotation(quadpol_ref.rotate, *shape)))


@pytest.mark.parametrize('n', GRAD_N)
def test_gradient_restatement_passes_the_sweep(n):
    print('n %3d: worst ratio %.3f' % (n, sweep_gradient(quadpol_ref.dphi_dz_from_tables, n)))


@pytest.mark.parametrize('n', GRAD_FILT_N)
def test_filtered_gradient_restatement_passes_the_sweep(n):
    print('n %3d filtered: worst ratio %.3f' % (n, sweep_gradient_filtered(quadpol_ref.dphi_dz_from_tables, n)))


def test_gradient_restatement_edges():
    check_gradient_refuses_twelve_rows(quadpol_ref.dphi_dz_from_tables)
    print('special images: worst ratio %.3f' % check_gradient_special_images(quadpol_ref.dphi_dz_from_tables))


def test_phase_diff_restatement_passes_the_sweep():
    worst, nans, empty = 0.0, 0, 0
    for length in sw.PD_LEN:
        w, k, e = sweep_phase_diff(apres_ref.phase_diff, length)
        worst, nans, empty = max(worst, w), nans + k, empty + e
    print('phase difference: %.3f of the bar, %d NaN windows, %d cases without a window' % (worst, nans, empty))
    assert len(sw.PD_LEN) * len(sw.PD_WIN) * len(sw.PD_STEP) == 700 and empty == 340
    assert nans > 1000


@pytest.mark.parametrize('snum', RANGE_SNUM)
def test_range_restatement_passes_the_sweep(snum):
    for p in RANGE_P:
        for chunk in ((0, 2) if snum == 257 else (0,)):
            worst, rworst, checked, left = check_range(apres_ref.range_rows, snum, p, chunk)
            print('snum %3d p %d chunk %d: spec/data %.3f of E, Rfine %.3f of its bar on %d bins, %d left out'
                  % (snum, p, chunk, worst, rworst, checked, left))


@pytest.mark.parametrize('snum', STACK_SNUM)
def test_stack_restatement_passes_the_sweep(snum):
    sweep_stack(apres_ref.stack, snum)


def test_numpy_mean_leaves_row_order_at_one_sample():
    """What the stacking comment says: from m = 8 on, numpy.mean over a contiguous m-axis is not the row-order sum."""
    rng = np.random.RandomState(5)
    differs = []
    for m in (7, 8, 100, 1000):
        for _ in range(20):
            x = rng.standard_normal((1, m, 1))
            if not same_bits(np.mean(x, axis=1), apres_ref.stack(x[0], 1, m)):
                differs.append(m)
    assert 7 not in differs and 1000 in differs
