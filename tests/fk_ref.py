"""The yardstick of the f-k fan filter and the f-k spectrum (csrc/fk_weight.h states the contract): the same arithmetic in
NumPy, the weight in ``longdouble`` and the transforms through ``scipy.fft`` in ``longdouble`` (``hi``), or in the data's own
precision with the float64 weight (``ref``).  The device is held to ``max|dev - hi| <= 8 max|ref - hi|``, the house margin for
a different order of the same sums.
"""
import numpy as np
import scipy.fft

LD = np.longdouble
MODES = ('pass', 'reject')
DIPS = ('both', 'down_right', 'down_left')


def axes(snum, tnum, dt, dx):
    """``(w (snum,), kx (tnum,))`` float64, both in ``fftfreq`` order."""
    return 2. * np.pi * np.fft.fftfreq(snum, dt), 2. * np.pi * np.fft.fftfreq(tnum, dx)


def edge(p, pc, taper, real):
    """E(p; pc, taper) in the type ``real``."""
    lo = pc * (real(1) - real(taper))
    hi = pc * (real(1) + real(taper))
    out = np.zeros(p.shape, dtype=real)
    mid = (p > lo) & (p < hi)
    pi = real(4) * np.arctan(real(1))
    with np.errstate(invalid='ignore'):
        out[mid] = (real(1) + np.cos(pi * (p[mid] - lo) / (hi - lo))) / real(2)
    out[p <= lo] = 1
    out[np.isnan(p)] = np.nan
    return out


def weight_at(w, kx, nyq, va_lo=None, va_hi=None, taper=0.1, mode='pass', dip='both', real=LD):
    """The fan weight M at the elements (w[i], kx[i]) (signed, float64 in, any common shape); ``nyq``: the element lies on a
    Nyquist row or column."""
    w = np.asarray(w, dtype=np.float64)
    kx = np.asarray(kx, dtype=np.float64)
    aw = np.abs(w).astype(real)
    ak = np.abs(kx).astype(real)
    with np.errstate(divide='ignore', invalid='ignore'):
        p = ak / aw
    p[aw == 0] = np.inf
    p[ak == 0] = 0
    W = np.ones(p.shape, dtype=real)
    if va_lo is not None:
        W = W * edge(p, real(1) / real(va_lo), taper, real)
    if va_hi is not None:
        W = W * (real(1) - edge(p, real(1) / real(va_hi), taper, real))
    if dip != 'both':
        s = np.sign(w) * np.sign(kx)
        off = (s > 0) if dip == 'down_right' else (s < 0)
        W[off & ~np.asarray(nyq, dtype=bool)] = 0
    return real(1) - W if mode == 'reject' else W


def weight(w, kx, nyq_row=None, nyq_col=None, real=LD, **fan):
    """... on the grid ``w`` x ``kx``.  ``nyq_row`` / ``nyq_col``: the index of the Nyquist row / column (None: there is none)."""
    w2, k2 = np.meshgrid(np.asarray(w, dtype=np.float64), np.asarray(kx, dtype=np.float64), indexing='ij')
    nyq = np.zeros(w2.shape, dtype=bool)
    if nyq_row is not None:
        nyq[nyq_row, :] = True
    if nyq_col is not None:
        nyq[:, nyq_col] = True
    return weight_at(w2, k2, nyq, real=real, **fan)


def grid_weight(snum, tnum, w, kx, real=LD, **fan):
    return weight(w, kx, nyq_row=snum // 2 if snum % 2 == 0 else None, nyq_col=tnum // 2 if tnum % 2 == 0 else None, real=real, **fan)


def fan_full(x, w, kx, precision='hi', **fan):
    """``ifft2(M * fft2(x))``, complex: 'hi' in longdouble throughout; 'ref' with the transforms in the dtype of ``x`` and
    the weight in float64."""
    snum, tnum = x.shape
    if precision == 'hi':
        M = grid_weight(snum, tnum, w, kx, real=LD, **fan)
        return scipy.fft.ifft2(M * scipy.fft.fft2(x.astype(LD)))
    M = grid_weight(snum, tnum, w, kx, real=np.float64, **fan)
    ctype = np.complex64 if x.dtype == np.float32 else np.complex128
    return scipy.fft.ifft2((M * scipy.fft.fft2(x)).astype(ctype))


def fan(x, w, kx, precision='hi', **fan_args):
    y = fan_full(x, w, kx, precision, **fan_args).real
    return y if precision == 'hi' else y.astype(x.dtype)


def power(x, precision='hi'):
    """``|fft2(x)|^2`` for the snum // 2 + 1 rows w >= 0, the columns in fftshift order."""
    m = x.shape[0] // 2 + 1
    if precision == 'hi':
        F = scipy.fft.fft2(x.astype(LD))[:m]
        P = F.real * F.real + F.imag * F.imag
    else:
        F = scipy.fft.fft2(x)[:m]
        P = F.real.astype(np.float64) ** 2 + F.imag.astype(np.float64) ** 2
    return np.fft.fftshift(P, axes=1)


def two_events(n=128, period=16.0):
    """The analytic case: plane events of period 16 samples, slopes +0.5 (arrival time grows with distance: down_right,
    slowness 0.5) and -1 (down_left, slowness 1) sample per trace, on an n x n grid with dt = dx = 1."""
    t = np.arange(n, dtype=np.float64)[:, None]
    x = np.arange(n, dtype=np.float64)[None, :]
    return np.cos(2. * np.pi * (t - 0.5 * x) / period), np.cos(2. * np.pi * (t + 1.0 * x) / period)


def radargram(snum, tnum, dtype, seed=0):
    """A small test image: noise and two dipping events."""
    rng = np.random.default_rng(seed + 1000 * snum + tnum)
    t = np.arange(snum)[:, None]
    x = np.arange(tnum)[None, :]
    img = rng.standard_normal((snum, tnum)) + 2.0 * np.cos(0.7 * (t - 0.4 * x)) + np.sin(0.3 * (t + 1.3 * x))
    return np.ascontiguousarray(img.astype(dtype))
