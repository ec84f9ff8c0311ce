"""Extended-precision references and seeded inputs of the kernel sweeps (``test_kernel_sweeps_cpu.py``,
``test_quadpol_sweep_gpu.py``, ``test_apres_sweep_gpu.py``).

Every reference here takes each output's window directly, in ``numpy.longdouble``: no box sums, no block sums, no
running sums, nothing of the kernels' decomposition.  What a kernel is handed as a table (azimuth factors, the
window, ``comp``, ``den``, the two scale factors) is taken as that float64 number, exactly; all arithmetic on it is
long double.  The phase gradient's long-double form is ``quadpol_ref.dphi_dz(..., dtype=numpy.longdouble)``.
"""
import functools

import numpy as np

import apres_ref

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, 'numpy.longdouble is no wider than float64 here: the sweeps have no reference'

U = 2.0 ** -53


def _parts(z):
    z = np.asarray(z, dtype=np.complex128)
    return z.real.astype(LD), z.imag.astype(LD)


def _products(x, y):
    """Re and Im of x conj(y), |x|^2, |y|^2 elementwise, in long double."""
    xr, xi = _parts(x)
    yr, yi = _parts(y)
    return xr * yr + xi * yi, xi * yr - xr * yi, xr * xr + xi * xi, yr * yr + yi * yi


def _quotient(pr, pi, a, b):
    """complex128 of (pr + i pi) / sqrt(a b); NaN in both parts where the divisor is 0."""
    den = np.sqrt(a * b)
    zero = den == 0
    den = np.where(zero, LD(1), den)
    out = np.empty(den.shape, dtype=np.complex128)
    out.real = np.where(zero, LD(np.nan), pr / den).astype(np.float64)
    out.imag = np.where(zero, LD(np.nan), pi / den).astype(np.float64)
    return out


# ------------------------------------------------------------------------------------------------ references
def coherence_ld(HH, VV, nrange, ntheta, wrap):
    """``(chhvv, terms)``: for output (j, i) the four sums over rows ``[max(0, j - nrange), min(n - 1, j + nrange))`` and
    the ``2 ntheta`` columns from ``i - ntheta`` (periodic) or from ``i`` (a padded pair, ``ncols - 2 ntheta`` outputs),
    each taken on its own; ``terms[j, i]`` is the number of elements in that window."""
    n, ncols = np.shape(HH)
    nout = ncols if wrap else ncols - 2 * ntheta
    first = np.arange(nout) - ntheta if wrap else np.arange(nout)
    cols = (first[:, None] + np.arange(2 * ntheta)[None, :]) % ncols          # (nout, 2 ntheta)
    prods = _products(HH, VV)
    sums = [np.zeros((n, nout), dtype=LD) for _ in prods]
    terms = np.zeros((n, nout), dtype=np.int64)
    for j in range(n):
        lo, hi = max(0, j - nrange), min(n - 1, j + nrange)
        terms[j] = 2 * ntheta * max(hi - lo, 0)
        if hi > lo:
            for s, p in zip(sums, prods):
                s[j] = p[lo:hi][:, cols].sum(axis=(0, 2))
    return _quotient(*sums), terms


def phase_diff_ld(s1, s2, win, step):
    """``(co, terms)``: window i covers samples ``[i step, i step + 2 (win // 2))``, for every i whose window starts
    before ``len - 2 (win // 2)``."""
    length, terms = len(s1), 2 * (win // 2)
    starts = np.arange(0, max(length - terms, 0), step)
    idx = starts[:, None] + np.arange(terms)[None, :]
    sums = [p[idx].sum(axis=1) if terms else np.zeros(len(starts), dtype=LD) for p in _products(s1, s2)]
    return _quotient(*sums), np.full(len(starts), terms, dtype=np.int64)


def rotate_ld(vectors, cos2, sincos, sin2):
    """``(HH, HV, VH, VV)`` as pairs (re, im) of long-double (n, n_thetas) arrays."""
    (hh, hv, vh, vv) = [[part[:, None] for part in _parts(v)] for v in vectors]
    c, m, s = [np.asarray(t, dtype=np.float64).astype(LD)[None, :] for t in (cos2, sincos, sin2)]
    out = []
    for k in (0, 1):
        out.append((hh[k] * c + (vh[k] + hv[k]) * m + vv[k] * s, hv[k] * c + (vv[k] - hh[k]) * m - vh[k] * s,
                    vh[k] * c + (vv[k] - hh[k]) * m - hv[k] * s, vv[k] * c - (vh[k] + hv[k]) * m + hh[k] * s))
    return tuple(zip(*out))


class RangeLd(object):
    """What :func:`range_ld` returns."""


def range_ld(raw, t):
    """The range conversion of (rows, snum) chirps with the tables ``t`` of ``apres.range_tables``: de-mean, window,
    the DFT as a direct sum, the two scale factors, ``comp``, ``atan2`` and ``den`` in long double.  ``spec`` and
    ``data`` (rows, n) complex128, ``Rfine`` (rows, nf) float64, ``mag`` = |data_k| of all nf bins, ``norm`` = the
    2-norm of each chirp's nf-bin spectrum (what ``apres_ref.spectrum_bar`` takes)."""
    raw = np.asarray(raw, dtype=np.float64).astype(LD)
    N = t.p * raw.shape[1]
    y = (raw - raw.sum(axis=1, keepdims=True) / LD(raw.shape[1])) * np.asarray(t.win, dtype=np.float64).astype(LD)
    X = apres_ref.dft_exact(y, N, t.nf)
    scale = LD(t.scale_mul) / LD(t.scale_div)
    sr, si = X.real.astype(LD) * scale, X.imag.astype(LD) * scale
    cr, ci = _parts(t.comp)
    dr, di = cr * sr - ci * si, cr * si + ci * sr
    phi = np.arctan2(di, dr)
    den = np.asarray(t.den, dtype=np.float64).astype(LD)
    r = RangeLd()
    r.Rfine = ((LD(t.lambdac) * phi / den) if t.first_order else phi / den).astype(np.float64)
    r.spec = (sr.astype(np.float64) + 1j * si.astype(np.float64))[:, :t.n]
    r.data = (dr.astype(np.float64) + 1j * di.astype(np.float64))[:, :t.n]
    r.mag = np.sqrt(dr * dr + di * di).astype(np.float64)
    r.norm = np.sqrt((sr * sr + si * si).sum(axis=1)).astype(np.float64)
    return r


def stack_mean_ld(data, groups, m):
    """Means over runs of m rows in long double, rounded to the data's type."""
    data = np.asarray(data)
    view = data[:groups * m].reshape(groups, m, data.shape[1])
    if np.iscomplexobj(data):
        re, im = view.real.astype(LD).sum(axis=1) / LD(m), view.imag.astype(LD).sum(axis=1) / LD(m)
        return re.astype(np.float64) + 1j * im.astype(np.float64)
    return (view.astype(LD).sum(axis=1) / LD(m)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ inputs
def _cnormal(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def image_pair(n, ncols, seed, zero_rows=False):
    """Two (n, ncols) complex128 images: amplitudes ``10**(-3 j / n)`` times complex normal, the second a phase-ramped
    copy of the first plus 30 % noise.  ``zero_rows`` zeroes three neighbouring rows of both where ``n >= 6``."""
    rng = np.random.RandomState(seed)
    amp = (10. ** (-3. * np.arange(n) / n))[:, None]
    HH = amp * _cnormal(rng, (n, ncols))
    VV = HH * np.exp(1j * 0.03 * np.arange(n))[:, None] + 0.3 * amp * _cnormal(rng, (n, ncols))
    if zero_rows and n >= 6:
        HH[n // 2 - 1:n // 2 + 2] = 0.
        VV[n // 2 - 1:n // 2 + 2] = 0.
    return np.ascontiguousarray(HH), np.ascontiguousarray(VV)


def vector_pair(length, seed, zeros=False):
    """The same recipe on two vectors; ``zeros`` zeroes samples 20 ... 29 of both where ``length >= 63``."""
    s1, s2 = [np.ascontiguousarray(x[:, 0]) for x in image_pair(length, 1, seed)]
    if zeros and length >= 63:
        s1[20:30] = 0.
        s2[20:30] = 0.
    return s1, s2


def coherence_image(n, m, seed):
    """A synthetic (n, m) coherence image: |c| in [0.2, 1], the phase a random walk along range."""
    rng = np.random.RandomState(seed)
    mag = 0.2 + 0.8 * rng.uniform(size=(n, m))
    return np.ascontiguousarray(mag * np.exp(1j * np.cumsum(0.3 * rng.standard_normal((n, m)), axis=0)))


def range_axis(n, jittered, seed=0):
    """``0.5 arange(n)`` (numpy.gradient's uniform rule) or a cumulative axis of uneven steps."""
    if not jittered:
        return 0.5 * np.arange(n)
    rng = np.random.RandomState(1000 + seed + n)
    return np.concatenate(([0.], np.cumsum(0.5 * (1. + 0.3 * rng.uniform(-1., 1., size=n - 1)))))


def chirps(snum, seed, rows=5):
    """(rows, snum) chirps: a constant, two cosines at 0.11 and 0.031 cycles per sample, 5 % noise."""
    rng = np.random.RandomState(seed)
    k = np.arange(snum)[None, :]
    ph = rng.uniform(0, 2 * np.pi, size=(rows, 2))
    x = 0.7 + np.cos(2 * np.pi * 0.11 * k + ph[:, :1]) + 0.5 * np.cos(2 * np.pi * 0.031 * k + ph[:, 1:])
    return np.ascontiguousarray(x + 0.05 * rng.standard_normal((rows, snum)))


# ------------------------------------------------------------------------------------------------ the cases
COH_N = (1, 2, 3, 4, 5, 8, 9, 31, 33, 64, 65, 130)
COH_NRANGE = (1, 2, 3, 16, 17, 64, 65, 256, 257, 1024, 1025, 5000)
# (ncols, ntheta, wrap, zero rows)
COH_COLS = ((1, 1, True, False), (2, 1, True, False), (5, 5, True, False), (7, 3, True, True), (24, 2, True, False),
            (3, 1, False, False), (9, 2, False, False))

PD_LEN = (1, 2, 3, 63, 64, 65, 66, 67, 129, 300)
PD_WIN = (0, 1, 2, 3, 9, 63, 64, 65, 66, 67, 128, 129, 130, 200)
PD_STEP = (1, 2, 7, 64, 1000)


@functools.lru_cache(maxsize=None)
def coherence_inputs(n, col):
    ncols, ntheta, wrap, zero_rows = COH_COLS[col]
    HH, VV = image_pair(n, ncols, 100 * n + col, zero_rows)
    HH.setflags(write=False)
    VV.setflags(write=False)
    return HH, VV


@functools.lru_cache(maxsize=None)
def coherence_want(n, nrange, col):
    """``(chhvv, terms)`` of :func:`coherence_ld` for one case of the sweep, computed once."""
    ncols, ntheta, wrap, _ = COH_COLS[col]
    want, terms = coherence_ld(*coherence_inputs(n, col), nrange, ntheta, wrap)
    want.setflags(write=False)
    return want, terms


@functools.lru_cache(maxsize=None)
def phase_diff_inputs(length):
    s1, s2 = vector_pair(length, 7000 + length, zeros=True)
    s1.setflags(write=False)
    s2.setflags(write=False)
    return s1, s2


@functools.lru_cache(maxsize=None)
def phase_diff_want(length, win, step):
    want, terms = phase_diff_ld(*phase_diff_inputs(length), win, step)
    want.setflags(write=False)
    return want, terms
