"""The contract of csrc/decon_core.h restated in NumPy, twice, and the fixtures of the deconvolution tests.

``hi``   everything in ``longdouble``: the lag sums, a Levinson recursion written out in a Python loop, the apply.  Not rounded.
``ref``  float64 with ``np.dot``, ``scipy.linalg.solve_toeplitz`` and the shifted subtraction, rounded to the data's dtype at the
         end: what a user without the library would write.

The tests hold the device (and the header's host recursion) to ``max|dev - hi| <= 8 max|ref - hi|`` per array.
"""
import numpy as np

LD = np.longdouble


def window_of(snum, window):
    return (0, snum) if window is None else (int(window[0]), int(window[1]))


def lag_list(oplen, gap):
    """The lags the system needs, rising, none twice."""
    return sorted(set(range(oplen)) | set(range(gap, gap + oplen)))


def lags_1d(x, s0, s1, lags, kind):
    """{l: r[l]} of one trace over [s0, s1); kind 'ref_reversed': float64 with the sums taken from the window's end."""
    if kind == 'hi':
        w = np.asarray(x[s0:s1]).astype(LD)
        return {l: (w[:len(w) - l] * w[l:]).sum(dtype=LD) if l < len(w) else LD(0) for l in lags}
    w = np.asarray(x[s0:s1]).astype(np.float64)
    if kind == 'ref_reversed':
        w = w[::-1]
    with np.errstate(all='ignore'):
        return {l: np.float64(np.dot(w[:len(w) - l], w[l:])) if l < len(w) else np.float64(0) for l in lags}


def alive(r0):
    return bool(np.isfinite(r0) and r0 > 0)


def levinson_hi(c, b):
    """The symmetric Toeplitz system sum_i c[|m - i|] a[i] = b[m] in longdouble; None when an error power leaves (0, inf)."""
    c, b = np.asarray(c, dtype=LD), np.asarray(b, dtype=LD)
    n = len(b)
    v = c[0]
    if not alive(v):
        return None
    p = np.zeros(n, dtype=LD)
    a = np.zeros(n, dtype=LD)
    p[0] = 1
    a[0] = b[0] / v
    for m in range(1, n):
        d = (p[:m] * c[m:0:-1]).sum(dtype=LD)
        e = (a[:m] * c[m:0:-1]).sum(dtype=LD)
        k = -d / v
        v = v + k * d
        if not alive(v):
            return None
        pn = p.copy()
        pn[:m + 1] = p[:m + 1] + k * p[m::-1][:m + 1]
        p = pn
        mu = (b[m] - e) / v
        a[:m + 1] = a[:m + 1] + mu * p[m::-1][:m + 1]
    return a


def solve(r, oplen, gap, eps, kind):
    """The operator from {l: r[l]}, or None for a dead system."""
    if not alive(r[0]):
        return None
    if kind == 'hi':
        c = np.array([r[l] for l in range(oplen)], dtype=LD)
        c[0] = c[0] * (1 + LD(eps))
        return levinson_hi(c, np.array([r[gap + m] for m in range(oplen)], dtype=LD))
    from scipy.linalg import solve_toeplitz
    c = np.array([r[l] for l in range(oplen)], dtype=np.float64)
    c[0] = c[0] * (1.0 + eps)
    return solve_toeplitz(c, np.array([r[gap + m] for m in range(oplen)], dtype=np.float64))


def apply_1d(x, a, gap, kind):
    T = LD if kind == 'hi' else np.float64
    x = np.asarray(x).astype(T)
    y = x.copy()
    with np.errstate(all='ignore'):
        for i in range(len(a)):
            s = gap + i
            if s < len(x):
                y[s:] -= T(a[i]) * x[:len(x) - s]
    return y


def decon(data, oplen, gap=1, prewhiten=0.1, window=None, design='each', kind='hi'):
    """``(y (snum, tnum), operators (oplen, tnum))``; ``hi``: longdouble, not rounded; ``ref``: y in the data's dtype."""
    data = np.asarray(data)
    snum, tnum = data.shape
    s0, s1 = window_of(snum, window)
    T = LD if kind == 'hi' else np.float64
    eps = prewhiten / 100.0
    lags = lag_list(oplen, gap)
    rs = [lags_1d(data[:, j], s0, s1, lags, kind) for j in range(tnum)]
    live = [alive(r[0]) for r in rs]
    ops = np.zeros((oplen, tnum), dtype=T)
    y = data.astype(T)
    if design == 'mean':
        a = None
        if any(live):
            R = {l: np.sum(np.array([rs[j][l] for j in range(tnum) if live[j]], dtype=T), dtype=T) for l in lags}
            a = solve(R, oplen, gap, eps, kind)
        for j in range(tnum):
            if a is not None and live[j]:
                ops[:, j] = a
                y[:, j] = apply_1d(data[:, j], a, gap, kind)
    else:
        for j in range(tnum):
            a = solve(rs[j], oplen, gap, eps, kind) if live[j] else None
            if a is not None:
                ops[:, j] = a
                y[:, j] = apply_1d(data[:, j], a, gap, kind)
    return (y if kind == 'hi' else y.astype(data.dtype)), ops


def acorr(data, maxlag, window=None, normalize=True, kind='hi'):
    """The autocorrelogram (maxlag + 1, tnum); normalised, a dead trace's column is NaN."""
    data = np.asarray(data)
    snum, tnum = data.shape
    s0, s1 = window_of(snum, window)
    T = LD if kind == 'hi' else np.float64
    A = np.empty((maxlag + 1, tnum), dtype=T)
    for j in range(tnum):
        r = lags_1d(data[:, j], s0, s1, range(maxlag + 1), kind)
        col = np.array([r[l] for l in range(maxlag + 1)], dtype=T)
        if normalize:
            with np.errstate(all='ignore'):
                col = col / col[0] if alive(col[0]) else np.full(maxlag + 1, np.nan, dtype=T)
        A[:, j] = col
    return A


def err(a, hi):
    """max |a - hi| in longdouble (both finite where it matters)."""
    return float(np.max(np.abs(np.asarray(a).astype(LD) - np.asarray(hi).astype(LD))))


# ---- fixtures -------------------------------------------------------------------------------------------------------------

def noise(snum, tnum, dtype, seed=11):
    return np.random.default_rng(seed).standard_normal((snum, tnum)).astype(dtype)


def wavelet(period=6.0, decay=0.82, length=40):
    """A ringing antenna pulse: a decaying cosine."""
    k = np.arange(length)
    return decay ** k * np.cos(2.0 * np.pi * k / period)


def ringing(snum, tnum, dtype, seed=5, density=0.06):
    """Sparse reflectors convolved with the ringing wavelet, a little noise on top."""
    rng = np.random.default_rng(seed)
    refl = rng.standard_normal((snum, tnum)) * (rng.random((snum, tnum)) < density)
    w = wavelet()
    out = np.empty((snum, tnum))
    for j in range(tnum):
        out[:, j] = np.convolve(refl[:, j], w)[:snum]
    return (out + 1.0e-3 * rng.standard_normal((snum, tnum))).astype(dtype)


def near_constant(snum, tnum, dtype, seed=3):
    rng = np.random.default_rng(seed)
    return (1.0 + 1.0e-3 * rng.standard_normal((snum, tnum))).astype(dtype)


FIXTURES = {'noise': noise, 'ringing': ringing, 'near_constant': near_constant}

# ---- the GPU suite's shapes (tests/test_decon_gpu.py; their plans are checked in tests/test_decon_route.py) --------------------
C = 64                  # DECON_C, the kernels' sample block
# (snum, tnum, oplen, gap, window): tnum 1 / 3 / 65 (V = 1), 130 (V = 2), 64 / 256 (V = 4), an odd rest and several trace
# groups; snum 16, 97, C - 1, C, C + 1, 2 C + 3; oplen 1, 2, 31, 64; gap 1, 2, oplen, oplen + 5, C + 1; the whole trace, a
# window strictly inside it and one of exactly gap + oplen samples
CASES = [(16, 1, 1, 1, None), (16, 3, 2, 2, None), (97, 64, 31, 1, None), (C - 1, 65, 31, 31, None), (C, 130, 2, 7, None),
         (C + 1, 256, 1, 6, None), (2 * C + 3, 65, 31, C + 1, None), (2 * C + 3, 130, 64, 1, None), (2 * C + 3, 64, 64, C + 1, None),
         (97, 3, 31, 36, (5, 90)), (97, 64, 31, 2, (10, 43)), (2 * C + 3, 256, 64, 64, None), (C, 1, 2, 1, (0, C)),
         (C + 1, 3, 2, 2, (1, C + 1))]
BIG = (600, 5, 256, 1, None)        # oplen 256, against ``ref`` only


def case_id(c):
    return '%dx%d-n%d-g%d%s' % (c[0], c[1], c[2], c[3], '' if c[4] is None else '-w%d_%d' % c[4])
