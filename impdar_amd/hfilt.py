"""Host side of the horizontal filters an impproc chain runs between the band pass and the migration:
``horizontalfilt`` (remove the mean trace of a range of traces), ``adaptivehfilt`` (remove a moving,
vertically smoothed mean trace) and ``winavg_hfilt`` (remove a moving mean trace as it is).  The O(snum + tnum) tables -- the clamped bounds, the adaptive windows and the
taper -- are built here; everything that touches the (snum, tnum) radargram runs in ``csrc/hfilt.hip`` through
the C ABI, on host buffers or on an array that is already resident in HBM.

Reference: ``src/impdar/lib/RadarData/_RadarDataFiltering.py:19-135, 353-440``.
"""
import ctypes as C

import numpy as np

from . import _hip

# scipy.signal.filtfilt's guard for the adaptive filter's 4-tap box (padlen = 3 * 4)
PADLEN_MESSAGE = 'The length of the input vector x must be greater than padlen, which is 12.'


def taper(travel_time):
    """``exp(-tt * 0.05) / exp(-tt[0] * 0.05)`` for ``tt = travel_time.flatten()`` (microseconds), float64."""
    tt = np.asarray(travel_time, dtype=np.float64).flatten()
    return np.ascontiguousarray(np.exp(-tt * 0.05) / np.exp(-tt[0] * 0.05))


def hfilt_bounds(ntr1, ntr2, tnum):
    """The reference's clamp of the averaging range (:126-127): ``[htr1, htrn)`` inside ``[0, tnum)``."""
    htr1 = int(max(0, min(ntr1, tnum - 1)))
    htrn = int(max(htr1 + 1, min(ntr2, tnum)))
    return htr1, htrn


def _slice_bound(v, tnum):
    """``slice(...).indices(tnum)``'s treatment of a start or stop (step 1), element-wise."""
    v = np.where(v < 0, v + tnum, v)
    return np.clip(v, 0, tnum)


def ahfilt_windows(tnum, window_size):
    """(lo, hi) int32 arrays of length tnum: trace i of ``adaptivehfilt`` averages ``data[:, lo[i]:hi[i]]``.
    The three branches of the reference's loop (:65-71), with Python's slice semantics (a negative start wraps
    once, then everything clamps to [0, tnum]); an empty window has lo == hi."""
    tnum = int(tnum)
    w = int(window_size)
    h = w // 2
    i = np.arange(tnum, dtype=np.int64)
    first = i <= h
    last = ~first & (i >= tnum - h)
    start = np.where(first, 0, np.where(last, tnum - w, i - h + 1))
    stop = np.where(first, h + i, np.where(last, tnum, i + h))
    lo = _slice_bound(start, tnum)
    hi = np.maximum(_slice_bound(stop, tnum), lo)
    return np.ascontiguousarray(lo, dtype=np.int32), np.ascontiguousarray(hi, dtype=np.int32)


def winavg_window(avg_win, tnum):
    """The window ``winavg_hfilt`` filters with (:390-396): no more than ``tnum`` traces, then the next odd
    number, with the reference's messages."""
    if avg_win > tnum:
        print('Cannot average over more than the whole data matrix. Reducing avg_win to tnum')
        avg_win = tnum
    if avg_win % 2 == 0:
        avg_win = avg_win + 1
        print('The averaging window must be an odd number of traces.')
        print('The averaging window has been changed to {:d}'.format(avg_win))
    return avg_win


def winavg_windows(tnum, avg_win):
    """(lo, hi) int32 arrays of length tnum: trace i of ``winavg_hfilt`` averages ``data[:, lo[i]:hi[i]]`` with
    ``lo = max(0, i - h)``, ``hi = min(i + h, tnum)`` and ``h = (avg_win - 1) // 2`` (:421-431).  The window is
    half-open, so trace ``i + h`` is not in it, and ``avg_win = 1`` leaves it empty (lo == hi: a NaN mean)."""
    h = (int(avg_win) - 1) // 2
    i = np.arange(int(tnum), dtype=np.int64)
    lo = np.maximum(i - h, 0)
    hi = np.maximum(np.minimum(i + h, tnum), lo)
    return np.ascontiguousarray(lo, dtype=np.int32), np.ascontiguousarray(hi, dtype=np.int32)


def winavg_taper(travel_time, kind='full', filtdepth=100):
    """The depth taper of ``winavg_hfilt`` (:397-416), float64: ``full`` is :func:`taper`; ``pexp`` makes it reach
    zero at sample ``filtdepth``, stay there, and start from one."""
    scale = taper(travel_time)
    if kind == 'full':
        return scale
    if kind == 'pexp':
        scale[:filtdepth] = scale[:filtdepth] - scale[filtdepth]
        scale[filtdepth:] = 0
        return np.ascontiguousarray(scale / np.max(scale))
    if kind == 'tukey':
        raise NotImplementedError('the tukey taper of winavg_hfilt is not part of the MI355X engine (the reference\'s '
                                  'fails on an undefined name)')
    raise ValueError('Unrecognized taper. Options are full, pexp, or tukey')


def _check_scale(scale, snum):
    scale = np.ascontiguousarray(scale, dtype=np.float64)
    if scale.shape != (snum,):
        raise ValueError('travel_time has %d samples but the data has %d' % (scale.size, snum))
    return scale


def _work(data):
    """Working copy for the in-place C calls (integers widened to float64, as ``filter_host`` does)."""
    return _hip.work_array(data, 'horizontal filters on complex data are', copy=True)


def _ahfilt_args(shape, lo, hi, scale):
    snum, tnum = shape
    if snum <= 12:
        raise ValueError(PADLEN_MESSAGE)
    lo = np.ascontiguousarray(lo, dtype=np.int32)
    hi = np.ascontiguousarray(hi, dtype=np.int32)
    if lo.shape != (tnum,) or hi.shape != (tnum,):
        raise ValueError('window tables must have tnum = %d entries' % tnum)
    ip = C.POINTER(C.c_int)
    scale = _check_scale(scale, snum)
    return lo, hi, scale, lo.ctypes.data_as(ip), hi.ctypes.data_as(ip), _hip.as_dp(scale)[1]


def hfilt_host(data, lo, hi, scale):
    """Copy of a host radargram with the tapered mean of traces [lo, hi) removed from every trace."""
    data = np.asarray(data)
    work = _work(data)
    snum, tnum = work.shape
    scale = _check_scale(scale, snum)
    rc = _hip.load().impdar_hfilt(_hip.context(), work.ctypes.data_as(C.c_void_p), _hip.dtype_code(work.dtype),
                                  snum, tnum, int(lo), int(hi), _hip.as_dp(scale)[1])
    _hip.check(rc, 'impdar_hfilt')
    return work.astype(data.dtype) if work.dtype != data.dtype else work


def hfilt_dev(d_arr, lo, hi, scale):
    """In place on a resident :class:`impdar_amd._hip.DeviceArray` (float32 / float64)."""
    snum, tnum = d_arr.shape
    scale = _check_scale(scale, snum)
    rc = _hip.load().impdar_hfilt_dev(d_arr.ctx, d_arr.ptr, _hip.dtype_code(d_arr.dtype), snum, tnum, int(lo), int(hi),
                                      _hip.as_dp(scale)[1])
    _hip.check(rc, 'impdar_hfilt')


def ahfilt_host(data, lo, hi, scale):
    """Adaptively filtered copy of a host radargram in its own dtype (integers: computed in float64, then
    ``astype``, which truncates toward zero as the reference's store into ``zeros_like(data)`` does)."""
    data = np.asarray(data)
    if data.ndim == 2:
        _ahfilt_args(data.shape, lo, hi, scale)       # argument errors before any device work
    work = _work(data)
    snum, tnum = work.shape
    lo, hi, scale, p_lo, p_hi, p_scale = _ahfilt_args(work.shape, lo, hi, scale)
    rc = _hip.load().impdar_ahfilt(_hip.context(), work.ctypes.data_as(C.c_void_p), _hip.dtype_code(work.dtype),
                                   snum, tnum, p_lo, p_hi, p_scale)
    _hip.check(rc, 'impdar_ahfilt')
    return work.astype(data.dtype) if work.dtype != data.dtype else work


def ahfilt_dev(d_arr, lo, hi, scale):
    """In place on a resident :class:`impdar_amd._hip.DeviceArray` (float32 / float64)."""
    snum, tnum = d_arr.shape
    lo, hi, scale, p_lo, p_hi, p_scale = _ahfilt_args(d_arr.shape, lo, hi, scale)
    rc = _hip.load().impdar_ahfilt_dev(d_arr.ctx, d_arr.ptr, _hip.dtype_code(d_arr.dtype), snum, tnum, p_lo, p_hi,
                                       p_scale)
    _hip.check(rc, 'impdar_ahfilt')


def _winavg_args(shape, lo, hi, scale):
    snum, tnum = shape
    lo = np.ascontiguousarray(lo, dtype=np.int32)
    hi = np.ascontiguousarray(hi, dtype=np.int32)
    if lo.shape != (tnum,) or hi.shape != (tnum,):
        raise ValueError('window tables must have tnum = %d entries' % tnum)
    ip = C.POINTER(C.c_int)
    scale = _check_scale(scale, snum)
    return lo, hi, scale, lo.ctypes.data_as(ip), hi.ctypes.data_as(ip), _hip.as_dp(scale)[1]


def winavg_host(data, lo, hi, scale):
    """Copy of a host radargram with the tapered moving mean trace removed, in its own dtype (integers: computed
    in float64, then ``astype``, as :func:`ahfilt_host`)."""
    data = np.asarray(data)
    work = _work(data)
    snum, tnum = work.shape
    lo, hi, scale, p_lo, p_hi, p_scale = _winavg_args(work.shape, lo, hi, scale)
    rc = _hip.load().impdar_winavg(_hip.context(), work.ctypes.data_as(C.c_void_p), _hip.dtype_code(work.dtype),
                                   snum, tnum, p_lo, p_hi, p_scale)
    _hip.check(rc, 'impdar_winavg')
    return work.astype(data.dtype) if work.dtype != data.dtype else work


def winavg_dev(d_arr, lo, hi, scale):
    """In place on a resident :class:`impdar_amd._hip.DeviceArray` (float32 / float64)."""
    snum, tnum = d_arr.shape
    lo, hi, scale, p_lo, p_hi, p_scale = _winavg_args(d_arr.shape, lo, hi, scale)
    rc = _hip.load().impdar_winavg_dev(d_arr.ctx, d_arr.ptr, _hip.dtype_code(d_arr.dtype), snum, tnum, p_lo, p_hi,
                                       p_scale)
    _hip.check(rc, 'impdar_winavg')
