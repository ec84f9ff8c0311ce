"""Host side of what a plot reads from the radargram: the percentiles of a window (the colour limits of the reference's
``plot_radargram`` and the x-limits of ``plot_traces``), the image distorted so that a picked layer lies flat, and a
window of a resident radargram as a dense host array.  Everything that reads the (snum, tnum) radargram runs in
``csrc/display.hip`` through the C ABI, on a host buffer or on an array that is already resident in HBM; the ranks are
formed inside the library, and the interpolation between the two order statistics of every percentage -- O(len(q)) -- is
done here, in NumPy's own order of operations, so that the result is ``np.percentile``'s bit for bit (float64 for both
dtypes; the sign of a zero is not pinned).

Reference: ``src/impdar/lib/plot.py:187-188, 240-254, 410``.
"""
import ctypes as C

import numpy as np

from . import _hip

MAX_Q = 8                               # percentages of one call of the library (display_route.h)
NO_SHIFT = -2 ** 31                     # IMPDAR_FLATTEN_NONE


def resolve_range(rng, size, what):
    """``(lo, hi)`` of a ``(lo, hi)`` pair in the reference's convention: None is everything, a last value of -1 the end;
    an end past the array is the array's, as in a slice."""
    if rng is None:
        rng = (0, -1)
    lo, hi = int(rng[0]), int(rng[-1])
    if hi == -1:
        hi = size
    hi = min(hi, size)
    if lo < 0 or lo > hi:
        raise ValueError('%s (%d, %d) is not a range of an axis of length %d' % (what, lo, int(rng[-1]), size))
    return lo, hi


def _q_array(q):
    qa = np.asarray(q, dtype=np.float64)
    if qa.ndim > 1:
        raise ValueError('q must be a number or a sequence of numbers')
    if qa.size == 0:
        raise ValueError('q is empty')
    if not np.all((qa >= 0.0) & (qa <= 100.0)):
        raise ValueError('Percentiles must be in the range [0, 100]')
    return qa


def lerp(a, b, g):
    """NumPy's interpolation between the neighbours ``a`` and ``b`` (arrays of the data's dtype) at the float64
    fractions ``g``: ``a + (b - a) g``, replaced by ``b - (b - a) (1 - g)`` where ``g >= 0.5``; the difference is formed in
    the data's dtype."""
    with np.errstate(invalid='ignore', over='ignore'):
        d = b - a
        out = np.asarray(a + d * g, dtype=np.float64)
        upper = np.asarray(b - d * (1.0 - g), dtype=np.float64)
    return np.where(g >= 0.5, upper, out)


def interpolate(qa, n, vals):
    """The percentiles ``qa`` of ``n`` values from ``vals``: for every percentage the values of rank
    ``floor((n - 1) q / 100)`` and the next one (clipped to ``n - 1``), in that order."""
    v = (n - 1) * np.true_divide(qa, 100.0)
    g = v - np.floor(v)
    return lerp(vals[0::2], vals[1::2], g)


def _percentile(fn, ctx, ptr, dtype, shape, q, y_range, x_range, skip_nan):
    snum, tnum = shape
    dtype = np.dtype(dtype)
    qa = _q_array(q)
    flat = np.atleast_1d(qa)
    out = np.empty(flat.shape, dtype=np.float64)
    counts = (C.c_longlong * 2)()
    for i0 in range(0, flat.size, MAX_Q):
        part = np.ascontiguousarray(flat[i0:i0 + MAX_Q])
        vals = np.empty((2 * part.size,), dtype=dtype)
        rc = fn(ctx, ptr, _hip.dtype_code(dtype), snum, tnum, y_range[0], y_range[1], x_range[0], x_range[1], _hip.as_dp(part)[1],
                part.size, 1 if skip_nan else 0, counts, vals.ctypes.data_as(C.c_void_p))
        _hip.check(rc, 'impdar_order_stats')
        n = counts[0] - counts[1]
        if counts[0] == 0 or (n == 0 and skip_nan):
            raise IndexError('index -1 is out of bounds for axis 0 with size 0')
        if counts[1] > 0 and not skip_nan:
            out[i0:i0 + part.size] = np.nan
        else:
            out[i0:i0 + part.size] = interpolate(part, n, vals)
    return out[0] if qa.ndim == 0 else out


def _prepare(shape, q, y_range, x_range):
    if len(shape) != 2:
        raise ValueError('data must be (snum, tnum)')
    if shape[0] < 1 or shape[1] < 1:
        raise IndexError('index -1 is out of bounds for axis 0 with size 0')
    _q_array(q)
    return resolve_range(y_range, shape[0], 'y_range'), resolve_range(x_range, shape[1], 'x_range')


def percentile_host(data, q, y_range=(0, -1), x_range=(0, -1), skip_nan=True):
    """``np.percentile(w, q)`` of the window ``w = data[y0:y1, x0:x1]`` of a host radargram -- with ``skip_nan`` of
    ``w[~isnan(w)]``; without it a NaN in the window makes every percentile NaN, as NumPy does.  float64 whatever the
    data's dtype; a scalar ``q`` gives the scalar ``np.percentile(w, [q])[0]`` (NumPy's own scalar form hands back the
    data's dtype).  An empty selection is NumPy's ``IndexError``."""
    work = _hip.work_array(data, 'percentiles of complex data are', copy=False)
    yr, xr = _prepare(work.shape, q, y_range, x_range)
    return _percentile(_hip.load().impdar_order_stats, _hip.context(), work.ctypes.data_as(C.c_void_p), work.dtype, work.shape, q, yr,
                       xr, skip_nan)


def percentile_dev(d_arr, q, y_range=(0, -1), x_range=(0, -1), skip_nan=True):
    """The same of a resident :class:`impdar_amd._hip.DeviceArray` (float32 / float64), which stays where it is."""
    yr, xr = _prepare(d_arr.shape, q, y_range, x_range)
    return _percentile(_hip.load().impdar_order_stats_dev, d_arr.ctx, d_arr.ptr, d_arr.dtype, d_arr.shape, q, yr, xr, skip_nan)


def shifts_from_offset(offset, snum):
    """int32 row shifts of the flattened image from the reference's float offsets: ``int(offset)`` (towards zero), a
    NaN offset -- no pick on that trace -- as ``NO_SHIFT``.  Offsets of ``snum`` rows or more leave nothing of a trace
    whatever their size, so they are clipped to ``snum``."""
    offset = np.asarray(offset, dtype=np.float64)
    if offset.ndim != 1:
        raise ValueError('offset must be one value per trace')
    none = np.isnan(offset)
    k = np.trunc(np.clip(np.where(none, 0.0, offset), -float(snum), float(snum))).astype(np.int32)
    k[none] = NO_SHIFT
    return np.ascontiguousarray(k)


def _flatten_args(shape, shift, x_range):
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError('the radargram is empty')
    x0, x1 = resolve_range(x_range, shape[1], 'x_range')
    if x1 == x0:
        raise ValueError('x_range holds no traces')
    shift = np.ascontiguousarray(shift)
    if shift.dtype != np.int32 or shift.shape != (x1 - x0,):
        raise ValueError('shift must be one int32 per trace of x_range (%d), got %s of shape %s' % (x1 - x0, shift.dtype, shift.shape))
    return x0, x1, shift


def flatten_host(data, shift, x_range=(0, -1)):
    """``out[i, j] = data[i - shift[j], x0 + j]`` where that row exists, NaN elsewhere and in the columns with
    ``NO_SHIFT``: the (snum, x1 - x0) image of a host radargram, in its dtype."""
    work = _hip.work_array(data, 'flattened images of complex data are', copy=False)
    x0, x1, shift = _flatten_args(work.shape, shift, x_range)
    out = np.empty((work.shape[0], x1 - x0), dtype=work.dtype)
    rc = _hip.load().impdar_flatten(_hip.context(), work.ctypes.data_as(C.c_void_p), _hip.dtype_code(work.dtype), work.shape[0],
                                    work.shape[1], x0, x1, shift.ctypes.data_as(C.POINTER(C.c_int)), out.ctypes.data_as(C.c_void_p))
    _hip.check(rc, 'impdar_flatten')
    return out


def flatten_dev(d_arr, shift, x_range=(0, -1), resident=False):
    """The same of a resident :class:`impdar_amd._hip.DeviceArray`; ``resident=True`` leaves the image in HBM and
    returns a ``DeviceArray`` in place of the host array."""
    x0, x1, shift = _flatten_args(d_arr.shape, shift, x_range)
    with _hip.new_device_array(d_arr.ctx, (d_arr.shape[0], x1 - x0), d_arr.dtype) as d_out:
        rc = _hip.load().impdar_flatten_dev(d_arr.ctx, d_arr.ptr, _hip.dtype_code(d_arr.dtype), d_arr.shape[0], d_arr.shape[1], x0, x1,
                                            shift.ctypes.data_as(C.POINTER(C.c_int)), d_out.ptr)
        _hip.check(rc, 'impdar_flatten_dev')
    if resident:
        return d_out
    out = d_out.to_host()
    d_out.free()
    return out


def window_host(data, y_range=(0, -1), x_range=(0, -1)):
    """``data[y0:y1, x0:x1]`` of a host radargram as a dense array of its own (any dtype; no device is involved)."""
    data = np.asarray(data)
    if data.ndim != 2:
        raise ValueError('data must be (snum, tnum)')
    (y0, y1), (x0, x1) = resolve_range(y_range, data.shape[0], 'y_range'), resolve_range(x_range, data.shape[1], 'x_range')
    return np.array(data[y0:y1, x0:x1], order='C')


def window_dev(d_arr, y_range=(0, -1), x_range=(0, -1)):
    """The same of a resident :class:`impdar_amd._hip.DeviceArray`: only the window crosses PCIe, as a strided copy."""
    if len(d_arr.shape) != 2:
        raise ValueError('data must be (snum, tnum)')
    (y0, y1), (x0, x1) = resolve_range(y_range, d_arr.shape[0], 'y_range'), resolve_range(x_range, d_arr.shape[1], 'x_range')
    out = np.empty((y1 - y0, x1 - x0), dtype=d_arr.dtype)
    if out.size:
        rc = _hip.load().impdar_window_dev(d_arr.ctx, d_arr.ptr, _hip.dtype_code(d_arr.dtype), d_arr.shape[0], d_arr.shape[1], y0, y1,
                                           x0, x1, out.ctypes.data_as(C.c_void_p))
        _hip.check(rc, 'impdar_window_dev')
    return out
