"""The yardstick of the layer-slope steps (csrc/slope_route.h states the contract; csrc/slope.hip runs it).

``hi``   the contract in ``longdouble``: gradients, products, the two Gaussian passes with clamped indices, the field kinds and
         the dip-steered mean, nothing rounded.
``ref``  what a user would write in float64: ``np.gradient``, ``scipy.ndimage.gaussian_filter(mode='nearest', truncate=4.0)``
         and the same formulas; ``dipsmooth`` rounded to the data's dtype.

The bar (``held``): the device's distance from ``hi`` is at most 8 x ``ref``'s.  Distances: the tensor planes (kinds 3 .. 5) plain
max; coherence weighted by ``(a + c)_hi``; dip weighted by ``D_hi``, on the circle of period pi; slope weighted by
``D_hi / (1 + p_hi^2)`` with ``p_hi`` the unclamped slope, the samples whose unclamped ``|p_hi|`` lies within 1e-6 ``max_slope`` of
``max_slope`` left out (the clamp can go either way) -- at most 1 % of them, a condition of the fixture; ``dipsmooth`` plain max
with a GIVEN float64 slope (``hi``'s, rounded).  ``dipsmooth`` with its own slope is ill-conditioned where ``D`` is small and is not
held to a bar: it equals ``dipsmooth(slope=slope_host(kind 0))`` bit for bit instead.
"""
import numpy as np

LD = np.longdouble
PI = LD(4) * np.arctan(LD(1))
KINDS = ('slope', 'dip', 'coherence', 'jzz', 'jzx', 'jxx')
MAX_SLOPE = 4.0

# the route header's constants (tests/test_slope_route.py holds them to csrc/slope_route.h)
ROW_TX, COL_TX, COL_SEG, MAX_R, MAX_HALF = 256, 32, 64, 64, 32


def radius(sigma):
    return int(4.0 * sigma + 0.5)


def weights(sigma, dtype=np.float64):
    r = radius(sigma)
    if r == 0:
        return np.ones(1, dtype=dtype)
    i = np.arange(-r, r + 1).astype(dtype)
    e = np.exp(-(i * i) / (dtype(2) * dtype(sigma) * dtype(sigma))).astype(LD)        # e in `dtype`, the normalisation in longdouble
    s = LD(0)
    for v in e:
        s = s + v
    return (e / s).astype(dtype)


def _loaded(x, dtype):
    x = np.asarray(x)
    return np.where(np.isfinite(x), x, np.nan).astype(dtype)


def gradient(x, axis):
    """Rule 2 in x's own precision."""
    n = x.shape[axis]
    g = np.zeros_like(x)
    if n == 1:
        return g
    x = np.moveaxis(x, axis, 0)
    g = np.moveaxis(g, axis, 0)
    g[1:-1] = (x[2:] - x[:-2]) / x.dtype.type(2)
    g[0] = x[1] - x[0]
    g[-1] = x[-1] - x[-2]
    return np.moveaxis(g, 0, axis)


def smooth(P, sigma, axis):
    """Rule 4 along one axis: s = 0; i rising: s = s + w[i] P[clamp(index + i)]."""
    w = weights(sigma, P.dtype.type)
    r = (len(w) - 1) // 2
    n = P.shape[axis]
    idx = np.arange(n)
    s = np.zeros_like(P)
    with np.errstate(invalid='ignore'):
        for i in range(-r, r + 1):
            s = s + w[i + r] * np.take(P, np.clip(idx + i, 0, n - 1), axis=axis)
    return s


def planes_hi(x, sigma):
    """(a, b, c) in longdouble: traces first, then samples."""
    xl = _loaded(x, LD)
    with np.errstate(invalid='ignore'):
        gz, gx = gradient(xl, 0), gradient(xl, 1)
        return tuple(smooth(smooth(P, sigma[1], 1), sigma[0], 0) for P in (gz * gz, gz * gx, gx * gx))


def fields(a, b, c, max_slope=MAX_SLOPE):
    """Rule 5 in the precision of a, b, c: a dict of every kind plus 'D' and 'p' (the unclamped slope)."""
    t = a.dtype.type
    with np.errstate(all='ignore'):
        d = a - c
        D = np.sqrt(d * d + t(4) * b * b)
        p = np.where(D == 0, t(0), np.where(d >= 0, t(-2) * b / (d + D), -(D - d) / (t(2) * b)))
        p = np.where(np.isnan(D) | np.isnan(d), t(np.nan), p)
        slope = np.where(p > t(max_slope), t(max_slope), np.where(p < -t(max_slope), -t(max_slope), p))
        dip = np.arctan2(t(-2) * b, d) / t(2)
        s = a + c
        coh = np.where(s > 0, D / np.where(s > 0, s, t(1)), t(0))
        coh = np.where(np.isnan(s) | np.isnan(D), t(np.nan), coh)
    return {'slope': slope, 'dip': dip, 'coherence': coh, 'jzz': a, 'jzx': b, 'jxx': c, 'D': D, 'p': p, 'd': d}


def slope_hi(x, kind, sigma, max_slope=MAX_SLOPE):
    return fields(*planes_hi(x, sigma), max_slope=max_slope)[kind]


def dipsmooth_in(x, half, slope, dtype):
    """Rule 6 in `dtype` arithmetic, not rounded to the data's dtype."""
    xl = _loaded(x, dtype)
    n, m = xl.shape
    p = np.asarray(slope).astype(dtype)
    k = np.arange(n).astype(dtype)[:, None]
    jj = np.arange(m)[None, :] + np.zeros((n, 1), dtype=np.int64)
    total = np.zeros((n, m), dtype=dtype)
    count = np.zeros((n, m), dtype=dtype)
    with np.errstate(invalid='ignore'):
        for i in range(-half, half + 1):
            ok = (jj + i >= 0) & (jj + i < m)
            jc = np.clip(jj + i, 0, m - 1)
            s = k + p * dtype(i)
            nan = np.isnan(s)
            s = np.minimum(np.maximum(np.where(nan, dtype(0), s), dtype(0)), dtype(n - 1))
            k0 = np.floor(s).astype(np.int64)
            k1 = np.minimum(k0 + 1, n - 1)
            f = s - k0.astype(dtype)
            v = xl[k0, jc] + f * (xl[k1, jc] - xl[k0, jc])
            v = np.where(nan, dtype(np.nan), v)
            total = total + np.where(ok, v, dtype(0))
            count = count + ok.astype(dtype)
        y = total / count
    return np.where(np.isnan(p), dtype(np.nan), y)


def dipsmooth_hi(x, half, slope):
    return dipsmooth_in(x, half, slope, LD)


def out_dtype(x):
    return np.asarray(x).dtype if np.asarray(x).dtype in (np.float32, np.float64) else np.dtype(np.float64)


def planes_ref(x, sigma):
    from scipy.ndimage import gaussian_filter
    x64 = _loaded(x, np.float64)
    n, m = x64.shape
    with np.errstate(invalid='ignore'):
        gz = np.gradient(x64, axis=0) if n > 1 else np.zeros_like(x64)
        gx = np.gradient(x64, axis=1) if m > 1 else np.zeros_like(x64)
        return tuple(gaussian_filter(P, sigma=tuple(sigma), mode='nearest', truncate=4.0) for P in (gz * gz, gz * gx, gx * gx))


def slope_ref(x, kind, sigma, max_slope=MAX_SLOPE):
    """np.gradient, scipy.ndimage.gaussian_filter and the formulas, in float64."""
    return fields(*planes_ref(x, sigma), max_slope=max_slope)[kind]


def dipsmooth_ref(x, half, slope):
    """NumPy in float64, rounded to the data's dtype."""
    with np.errstate(invalid='ignore'):
        return dipsmooth_in(x, half, np.asarray(slope, dtype=np.float64), np.float64).astype(out_dtype(x))


def rowmean_ref(x, half):
    """The plain clipped row mean: dipsmooth with an all-zero slope."""
    return dipsmooth_ref(x, half, np.zeros(np.asarray(x).shape))


# ---- the bars ---------------------------------------------------------------------------------------------------------------

def circ(d, period):
    d = np.abs(d)
    return np.minimum(d % period, period - d % period)


def _max(v):
    v = np.asarray(v)
    v = v[~np.isnan(v)]
    return float(v.max()) if v.size else 0.0


class Yard(object):
    """``hi`` of every kind of one radargram at one sigma pair, computed once."""

    def __init__(self, x, sigma, max_slope=MAX_SLOPE):
        self.x, self.sigma, self.max_slope = x, tuple(sigma), max_slope
        self.f = fields(*planes_hi(x, sigma), max_slope=max_slope)

    def hi(self, kind):
        return self.f[kind]

    def given_slope(self):
        """hi's slope rounded to float64: what dipsmooth's bar is measured with."""
        return np.ascontiguousarray(self.f['slope'].astype(np.float64))

    def left_out(self):
        """The samples the slope's distance leaves out: the unclamped |p_hi| within 1e-6 max_slope of max_slope."""
        with np.errstate(invalid='ignore'):
            return np.abs(np.abs(self.f['p']) - LD(self.max_slope)) <= LD(1e-6) * LD(self.max_slope)

    def vertical(self):
        """Samples with d < 0 and b = 0: the slope is infinite there and its sign arbitrary."""
        return (self.f['d'] < 0) & (self.f['jzx'] == 0)

    def distance(self, got, kind):
        """``(the weighted distance of `got` from hi over the samples where hi is a number, the share of samples left out)``."""
        f = self.f
        with np.errstate(all='ignore'):
            d = np.asarray(got).astype(LD) - f[kind]
            if kind in ('jzz', 'jzx', 'jxx'):
                return _max(np.abs(d)), 0.0
            if kind == 'coherence':
                return _max((f['jzz'] + f['jxx']) * np.abs(d)), 0.0
            if kind == 'dip':
                return _max(f['D'] * circ(d, PI)), 0.0
            out = self.left_out()
            p2 = np.where(np.isinf(f['p']), LD(0), f['p']) ** 2
            w = np.where(np.isinf(f['p']), LD(0), f['D'] / (LD(1) + p2))
            return _max(np.where(out, LD(0), w * np.abs(d))), float(np.mean(out))


def ratio(e_dev, e_ref):
    return e_dev / e_ref if e_ref else float(e_dev > 0)


def held(what, yard, got, ref, kind):
    """Print the ratio and hold ``got`` to 8 x the distance of ``ref``; the share left out is a condition of the fixture."""
    e_dev, out = yard.distance(got, kind)
    e_ref, _ = yard.distance(ref, kind)
    print('%s: dev %.3e ref %.3e ratio %.2f left out %.4f' % (what, e_dev, e_ref, ratio(e_dev, e_ref), out))
    assert out <= 0.01, what
    assert e_dev <= 8 * e_ref, what
    return ratio(e_dev, e_ref)


def held_dipsmooth(what, x, half, slope, got):
    """``dipsmooth`` with a given float64 slope: plain max distance from hi, 8 x ref's."""
    hi = dipsmooth_hi(x, half, slope)
    e_dev = _max(np.abs(np.asarray(got).astype(LD) - hi))
    e_ref = _max(np.abs(dipsmooth_ref(x, half, slope).astype(LD) - hi))
    print('%s: dev %.3e ref %.3e ratio %.2f' % (what, e_dev, e_ref, ratio(e_dev, e_ref)))
    assert np.array_equal(np.isnan(np.asarray(got)), np.isnan(hi)), what
    assert e_dev <= 8 * e_ref, what
    return ratio(e_dev, e_ref)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------

def ricker(t, fp):
    a = (np.pi * fp * t) ** 2
    return (1.0 - 2.0 * a) * np.exp(-a)


def layers(snum, tnum, dtype, seed=1):
    """At least snum / 12 Ricker layers with a random slope in +-0.8 and slight curvature, plus 5 % noise."""
    rng = np.random.default_rng(seed)
    k = np.arange(snum, dtype=np.float64)[:, None]
    u = np.arange(tnum, dtype=np.float64)[None, :] - 0.5 * (tnum - 1)
    out = np.zeros((snum, tnum))
    for _ in range(snum // 12 + 2):
        depth = rng.uniform(0, snum) + rng.uniform(-0.8, 0.8) * u + rng.uniform(-0.2, 0.2) * u * u / max(tnum, 1)
        out += rng.uniform(0.3, 1.0) * rng.choice([-1.0, 1.0]) * ricker(k - depth, 0.5 * rng.uniform(0.1, 0.3))
    return (out + 0.05 * rng.standard_normal((snum, tnum))).astype(dtype)


def fixture(snum, tnum, dtype):
    x = layers(snum, tnum, np.dtype(dtype).type, seed=1000 * snum + tnum)
    x.setflags(write=False)
    return x


SIGMAS = ((1.0, 1.0), (2.0, 4.0), (0.0, 3.0), (8.0, 0.5), (0.0, 0.0))
HALVES = (1, 4, MAX_HALF)
CPU_SHAPES = ((60, 31), (33, 70), (130, 257))
CPU_SIGMAS = SIGMAS[:4]
# the GPU suite's shapes, (snum, tnum): degenerate; one trace count below, at and past each trace-block width (the column pass'
# COL_TX, the row pass' ROW_TX; 31, 33, 255 and 257 are no multiple of a vector width either); one sample count below, at and
# past the column pass' segment; the CPU suite's three
CASES = ([(1, 1), (1, 5), (5, 1), (2, 2)]
         + [(9, COL_TX - 1), (9, COL_TX), (9, COL_TX + 1), (7, ROW_TX - 1), (7, ROW_TX), (7, ROW_TX + 1)]
         + [(COL_SEG - 1, 5), (COL_SEG, 6), (COL_SEG + 1, 3)]
         + list(CPU_SHAPES))
WIDE = ((8, 8), (16.0, 16.0))           # the radius (64) passes the radargram on both axes


def case_id(c):
    return '%dx%d' % (c[0], c[1])
