"""NumPy restatement of the reference's quad-pol chain (``src/impdar/lib/ApresData/_QuadPolProcessing.py:87-99,
153-165, 199-216``), written from its formulas and pinned to its output by ``test_quadpol_cpu.py`` on every ``Q*``
fixture.  The GPU tests use it where a fixture cannot serve: for the phase gradient of the device's own coherence
image, and as the stand-in for the kernels when the host logic is tested without a GPU."""
import numpy as np

U = 2.0 ** -53


def rotate(vectors, cos2, sincos, sin2):
    """``(HH, HV, VH, VV)`` of ``(shh, shv, svh, svv)`` for the per-azimuth factors."""
    shh, shv, svh, svv = [np.asarray(v, dtype=np.complex128)[:, None] for v in vectors]
    c, m, s = cos2[None, :], sincos[None, :], sin2[None, :]
    return (shh * c + (svh + shv) * m + svv * s, shv * c + (svv - shh) * m - svh * s,
            svh * c + (svv - shh) * m - shv * s, svv * c - (svh + shv) * m + shh * s)


def coherence(HH, VV, nrange, ntheta, wrap=True):
    """``chhvv`` over rows ``[max(0, j - nrange), min(n - 1, j + nrange))`` and columns ``[i - ntheta, i + ntheta)``:
    periodic columns (the reference's ``chhvv[:, ntheta:-ntheta]``) or, with ``wrap=False``, the columns of an
    already padded pair that have a whole window.  Sums are additions only."""
    HH, VV = np.asarray(HH, dtype=np.complex128), np.asarray(VV, dtype=np.complex128)
    n, ncols = HH.shape
    if wrap:
        HH = np.hstack((HH[:, ncols - ntheta:], HH, HH[:, :ntheta]))
        VV = np.hstack((VV[:, ncols - ntheta:], VV, VV[:, :ntheta]))
    nout = HH.shape[1] - 2 * ntheta
    prods = (HH * np.conj(VV), np.abs(HH) ** 2., np.abs(VV) ** 2.)
    box = [sum(p[:, k:k + nout] for k in range(2 * ntheta)) for p in prods]
    out = np.empty((n, nout), dtype=np.complex128)
    with np.errstate(invalid='ignore', divide='ignore'):
        for j in range(n):
            lo, hi = max(0, j - nrange), min(n - 1, j + nrange)
            top, a, b = [x[lo:hi].sum(axis=0) for x in box]
            out[j] = top / np.sqrt(a * b)
    return out


def n_terms(nrange, ntheta):
    """Terms of a full window, the N of the 4 N u bar."""
    return 4 * nrange * ntheta


def lowpass(data, spec):
    from scipy.signal import filtfilt
    _, b, a, _ = spec
    return filtfilt(b, a, data, axis=0)


def dphi_dz(chhvv, rng, spec=None, dtype=np.float64):
    """The reference's ``(R dI - I dR) / (R^2 + I^2)`` with ``np.gradient(., range, axis=0)``; ``spec`` is the
    ``('iir', b, a, zi)`` of its lowpass.  ``dtype=np.longdouble`` evaluates everything after the filter in extended
    precision."""
    R, I = np.real(chhvv).copy(), np.imag(chhvv).copy()
    if spec is not None:
        R, I = lowpass(R, spec), lowpass(I, spec)
    R, I, rng = R.astype(dtype), I.astype(dtype), np.asarray(rng).astype(dtype)
    with np.errstate(invalid='ignore', divide='ignore'):
        dR, dI = np.gradient(R, rng, axis=0), np.gradient(I, rng, axis=0)
        return (R * dI - I * dR) / (R ** 2. + I ** 2.)


def dphi_dz_from_tables(chhvv, grad, spec=None):
    """The same from ``mig_hip.gradient_coefficients``' tables, the form the kernel is given."""
    uniform, h, ga, gb, gc = grad
    R, I = np.real(chhvv).copy(), np.imag(chhvv).copy()
    if spec is not None:
        R, I = lowpass(R, spec), lowpass(I, spec)

    def gradient(f):
        g = np.empty_like(f)
        if uniform:
            g[1:-1] = (f[2:] - f[:-2]) / (2. * h)
            g[0], g[-1] = (f[1] - f[0]) / h, (f[-1] - f[-2]) / h
        else:
            g[1:-1] = ga[1:-1, None] * f[:-2] + gb[1:-1, None] * f[1:-1] + gc[1:-1, None] * f[2:]
            g[0], g[-1] = (f[1] - f[0]) / ga[0], (f[-1] - f[-2]) / ga[-1]
        return g
    with np.errstate(invalid='ignore', divide='ignore'):
        return (R * gradient(I) - I * gradient(R)) / (R ** 2. + I ** 2.)


def rel_err(got, want):
    """max |got - want| / max |want| over the entries where ``want`` is finite (0 where nothing differs, whatever
    ``want`` holds: an image whose rows all share one window has a gradient of exactly 0); NaN positions must
    agree."""
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = np.isfinite(want)
    diff = np.max(np.abs(got[ok] - want[ok]))
    return 0.0 if diff == 0 else float(diff / np.max(np.abs(want[ok])))
