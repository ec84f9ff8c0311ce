"""The contract of csrc/attr_route.h restated in NumPy, twice, the bars of the attribute tests and their fixtures.

``hi``   everything in ``longdouble``: a mixed-radix transform written out here (direct sums for the prime lengths), the
         analytic signal of ``scipy.signal.hilbert``'s definition, ``hypot`` / ``arctan2`` of longdouble, the window sums with
         ``j`` rising.  Not rounded.
``ref``  ``scipy.signal.hilbert(x, axis=0)`` on the data's own dtype, then ``np.abs``, ``np.angle``,
         ``np.diff(np.unwrap(.)) / (2 pi dt)`` with the last sample repeated and the weighted mean in float64: what a user
         without the library writes.

The bars are the house margin, 8 x the distance of ``ref`` from ``hi``:
  quadrature, envelope   max|dev - hi| <= 8 max|ref - hi|
  phase                  the same of e_hi[k] circ(phi - phi_hi[k]), circ the distance on the circle: phase is ill-conditioned
                         where the envelope vanishes
  frequency              the same of min(e_hi[k], e_hi[k + 1]) circ((f - f_hi) dt), the distance in cycles per sample on the
                         circle: a step that sits on +-pi does not count as 2 pi
  smoothed frequency     the same of sqrt(sum_window e_hi^2 / W) |f - f_hi| dt over the samples whose ``hi`` window holds no step
                         within 1e-6 rad of +-pi; at most 1 % of the samples may be left out
"""
import functools

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
PI = 4 * np.arctan(LD(1))
KINDS = ('quadrature', 'envelope', 'phase', 'frequency')
DT = 2.5e-9


# ---- hi ---------------------------------------------------------------------------------------------------------------------

def _smallest_factor(n):
    p = 2
    while p * p <= n:
        if n % p == 0:
            return p
        p += 1
    return n


@functools.lru_cache(maxsize=8)
def _roots(n, sign):
    a = sign * 2 * PI * np.arange(n, dtype=LD) / LD(n)
    w = np.empty(n, dtype=CLD)
    w.real, w.imag = np.cos(a), np.sin(a)
    return w


def _dft_direct(x, sign):
    n = x.shape[0]
    w = _roots(n, sign)
    out = np.empty_like(x)
    k = np.arange(n)
    for r0 in range(0, n, 256):         # (rows of the matrix in blocks: 2731^2 longdouble complex numbers at once are 240 MB)
        rows = k[r0:r0 + 256]
        out[rows] = w[(rows[:, None] * k[None, :]) % n] @ x
    return out


def fft_ld(x, sign=-1):
    """The unnormalised transform along axis 0 of a (n, c) clongdouble array, e^{sign 2 pi i j k / n}: decimation in time by the
    smallest prime factor, a direct sum at a prime length."""
    n, c = x.shape
    if n == 1:
        return x.copy()
    p = _smallest_factor(n)
    if p == n:
        return _dft_direct(x, sign)
    m = n // p
    sub = fft_ld(np.ascontiguousarray(x.reshape(m, p * c)), sign).reshape(m, p, c)      # sub[k', r] = sum_j x[j p + r] w_m^{j k'}
    w = _roots(n, sign)
    kk = np.arange(m)
    tw = w[(kk[:, None] * np.arange(p)[None, :]) % n]                                   # w_n^{r k'}
    t = sub * tw[:, :, None]
    wp = _roots(p, sign)
    out = np.empty((p, m, c), dtype=CLD)
    for s in range(p):                  # out[k' + m s] = sum_r w_p^{r s} t[k', r]
        acc = np.zeros((m, c), dtype=CLD)
        for r in range(p):
            acc += wp[(r * s) % p] * t[:, r, :]
        out[s] = acc
    return out.reshape(n, c)


def quadrature_hi(x):
    """imag(hilbert(x)) along axis 0 in longdouble; a column with a sample that is not finite is NaN."""
    x = np.asarray(x).astype(LD)
    n = x.shape[0]
    X = fft_ld(np.where(np.isfinite(x), x, 0).astype(CLD))
    h = np.zeros(n, dtype=LD)
    if n % 2 == 0:
        h[0] = h[n // 2] = 1
        h[1:n // 2] = 2
    else:
        h[0] = 1
        h[1:(n + 1) // 2] = 2
    q = (fft_ld(X * h[:, None], +1) / LD(n)).imag
    q[:, ~np.all(np.isfinite(x), axis=0)] = np.nan
    return q


def steps_of(x, q):
    """arg(z[k + 1] conj z[k]) for k < n - 1, the last one repeated (zeros for n = 1), in the arrays' precision."""
    n = x.shape[0]
    if n == 1:
        return np.zeros_like(x)
    with np.errstate(all='ignore'):
        s = np.arctan2(q[1:] * x[:-1] - x[1:] * q[:-1], x[1:] * x[:-1] + q[1:] * q[:-1])
    return np.concatenate([s, s[-1:]], axis=0)


def window_sum(a, half):
    """sum over |j - k| <= half, clipped, j rising (zeros beyond the ends add nothing)."""
    n = a.shape[0]
    pad = np.zeros((half,) + a.shape[1:], dtype=a.dtype)
    b = np.concatenate([pad, a, pad], axis=0)
    out = np.zeros_like(a)
    for off in range(2 * half + 1):
        out = out + b[off:off + n]
    return out


def attr_hi(x, kind, smooth=1, dt=DT):
    """The contract in longdouble, not rounded."""
    x = np.asarray(x)
    bad = ~np.all(np.isfinite(x), axis=0)
    xl = x.astype(LD)
    q = quadrature_hi(x)
    with np.errstate(all='ignore'):
        if kind == 'quadrature':
            out = q
        elif kind == 'envelope':
            out = np.hypot(xl, q)
        elif kind == 'phase':
            out = np.arctan2(q, xl)
        else:
            f = steps_of(xl, q) / (2 * PI * LD(dt))
            if smooth > 1:
                w = xl * xl + q * q
                num, den = window_sum(w * f, smooth // 2), window_sum(w, smooth // 2)
                f = np.where(den == 0, LD(0), num / np.where(den == 0, LD(1), den))
            out = f
    out = np.array(out, dtype=LD)
    out[:, bad] = np.nan
    return out


# ---- ref --------------------------------------------------------------------------------------------------------------------

def attr_ref(x, kind, smooth=1, dt=DT):
    """SciPy / NumPy on the data's own dtype."""
    from scipy.signal import hilbert
    x = np.asarray(x)
    bad = ~np.all(np.isfinite(x), axis=0)
    with np.errstate(all='ignore'):
        z = hilbert(np.where(np.isfinite(x), x, 0).astype(x.dtype), axis=0)
        if kind == 'quadrature':
            out = z.imag
        elif kind == 'envelope':
            out = np.abs(z)
        elif kind == 'phase':
            out = np.angle(z)
        else:
            n = x.shape[0]
            if n == 1:
                f = np.zeros(x.shape)
            else:
                f = np.diff(np.unwrap(np.angle(z), axis=0), axis=0) / (2.0 * np.pi * dt)
                f = np.concatenate([f, f[-1:]], axis=0)
            if smooth > 1:
                e2 = np.abs(z).astype(np.float64) ** 2
                f = f.astype(np.float64)
                ones = np.ones(smooth)
                num = np.stack([np.convolve(e2[:, j] * f[:, j], ones)[smooth // 2:smooth // 2 + n] for j in range(x.shape[1])], axis=1)
                den = np.stack([np.convolve(e2[:, j], ones)[smooth // 2:smooth // 2 + n] for j in range(x.shape[1])], axis=1)
                f = np.where(den == 0, 0.0, num / np.where(den == 0, 1.0, den))
            out = f
    out = np.array(out).astype(x.dtype if x.dtype in (np.float32, np.float64) else np.float64)
    out[:, bad] = np.nan
    return out


# ---- the bars ---------------------------------------------------------------------------------------------------------------

def circ(d, period):
    d = np.abs(d)
    return np.minimum(d % period, period - d % period)


class Yard(object):
    """``hi`` of every kind of one radargram (live traces: no sample that is not finite), computed once."""

    def __init__(self, x, dt=DT):
        self.x, self.dt = x, dt
        self.xl = np.asarray(x).astype(LD)
        self.q = quadrature_hi(x)
        self.e = np.hypot(self.xl, self.q)
        self.steps = steps_of(self.xl, self.q)

    def hi(self, kind, smooth=1):
        if kind == 'quadrature':
            return self.q
        if kind == 'envelope':
            return self.e
        if kind == 'phase':
            return np.arctan2(self.q, self.xl)
        return attr_hi(self.x, 'frequency', smooth, self.dt)

    def distance(self, got, kind, smooth=1):
        """``(the weighted distance of `got` from hi, the share of samples left out)``."""
        hi = self.hi(kind, smooth)
        d = np.asarray(got).astype(LD) - hi
        if kind in ('quadrature', 'envelope'):
            return float(np.max(np.abs(d))), 0.0
        if kind == 'phase':
            return float(np.max(self.e * circ(d, 2 * PI))), 0.0
        n = self.x.shape[0]
        if smooth == 1:
            e_next = np.concatenate([self.e[1:], self.e[-1:]], axis=0)
            wgt = np.minimum(self.e, e_next)
            if n > 1:
                wgt[-1] = wgt[-2]       # (the last sample repeats the step before it)
            return float(np.max(wgt * circ(d * LD(self.dt), LD(1)))), 0.0
        half = smooth // 2
        near = (np.abs(self.steps) > PI - LD(1e-6)).astype(np.int64)
        keep = window_sum(near, half) == 0
        wgt = np.sqrt(window_sum(self.e * self.e, half) / LD(smooth))
        val = np.where(keep, wgt * np.abs(d) * LD(self.dt), LD(0))
        return float(np.max(val)), float(1.0 - np.mean(keep))


def held(what, yard, got, ref, kind, smooth=1):
    """Print the ratio and hold ``got`` to 8 x the distance of ``ref``; the share left out is a condition of the fixture."""
    e_dev, out_dev = yard.distance(got, kind, smooth)
    e_ref, _ = yard.distance(ref, kind, smooth)
    print('%s: dev %.3e ref %.3e ratio %.2f left out %.4f' % (what, e_dev, e_ref, e_dev / e_ref if e_ref else float(e_dev > 0), out_dev))
    assert out_dev <= 0.01, what
    assert e_dev <= 8 * e_ref, what
    return e_dev / e_ref if e_ref else float(e_dev > 0)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------

def ricker(t, fp):
    a = (np.pi * fp * t) ** 2
    return (1.0 - 2.0 * a) * np.exp(-a)


def rickers(snum, tnum, dtype, seed=1):
    """A few Ricker wavelets per trace at 0.05 .. 0.3 of Nyquist plus 5 % noise."""
    rng = np.random.default_rng(seed)
    k = np.arange(snum, dtype=np.float64)
    out = np.zeros((snum, tnum))
    for j in range(tnum):
        for _ in range(4):
            fp = 0.5 * rng.uniform(0.05, 0.3)
            out[:, j] += rng.uniform(0.3, 1.0) * rng.choice([-1.0, 1.0]) * ricker(k - rng.uniform(0, snum), fp)
    return (out + 0.05 * rng.standard_normal((snum, tnum))).astype(dtype)


def chirp(snum, tnum, dtype, seed=2):
    """A linear sweep from 0.05 to 0.3 of Nyquist, a little different in every trace."""
    rng = np.random.default_rng(seed)
    k = np.arange(snum, dtype=np.float64)[:, None]
    f0 = 0.5 * (0.05 + 0.02 * rng.random(tnum))[None, :]
    f1 = 0.5 * (0.3 - 0.02 * rng.random(tnum))[None, :]
    phase = 2.0 * np.pi * (f0 * k + 0.5 * (f1 - f0) * k * k / max(snum - 1, 1))
    return np.cos(phase + rng.uniform(0, 2 * np.pi, tnum)[None, :]).astype(dtype)


FIXTURES = {'rickers': rickers, 'chirp': chirp}

# ---- the GPU suite's shapes (tests/test_attr_gpu.py; their routes are checked in tests/test_attr_route.py): n x tnum ---------
OWN_POW2, OWN_MIXED, ROCFFT = 0, 1, 2
# (n, tnum, route, threads of the row kernel)
CASES = [(1, 3, ROCFFT, 0), (2, 3, ROCFFT, 0),          # degenerate
         (30, 5, ROCFFT, 0),                            # half 15 < 16
         (32, 33, OWN_POW2, 64),                        # the smallest power-of-two half; a ragged 32-tile of the transposes
         (33, 4, ROCFFT, 0),                            # odd
         (44, 7, ROCFFT, 0),                            # factor 11
         (60, 31, OWN_MIXED, 64),                       # 2 3 5
         (126, 65, OWN_MIXED, 64),                      # factor 7
         (2048, 3, OWN_POW2, 256), (4096, 2, OWN_POW2, 512), (8192, 2, OWN_POW2, 1024),
         (16384, 2, OWN_POW2, 1024),                    # half 8192, the LDS limit
         (16386, 2, ROCFFT, 0),                         # just past it
         (32, 2100, OWN_POW2, 64)]                      # more traces than workgroups: rows_per_wg > 1, a short last block
SMOOTH_CASES = [(60, 31), (300, 5)]
SMOOTHS = (1, 3, 9, 255)


def case_id(c):
    return '%dx%d' % (c[0], c[1])


def fixture(n, tnum, dtype, name='rickers'):
    x = FIXTURES[name](n, tnum, np.dtype(dtype).type, seed=n + tnum)
    x.setflags(write=False)
    return x
