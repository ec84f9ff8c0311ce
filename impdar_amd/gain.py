"""Host side of the two gains, ``rangegain`` and ``agc``.  The O(snum) and O(tnum) tables -- the gain of every
sample, the first multiplied sample of every trace -- are NumPy here; everything that touches the (snum, tnum)
radargram runs in ``csrc/gain.hip`` through the C ABI, on host buffers or on an array that is already resident in
HBM.  ``agc`` of integer data multiplies by a truncated integer scale, as the reference does: the row maxima come
from the device, the integer product is NumPy.

Reference: ``src/impdar/lib/RadarData/_RadarDataProcessing.py:456-496``.
"""
import ctypes as C

import numpy as np

from . import _hip

_IP = C.POINTER(C.c_int)


# ------------------------------------------------------------------------------------------------ range gain
def rangegain_tables(travel_time, trig, slope, snum, tnum):
    """``(gain, start)``: ``gain[i] = travel_time[i] * slope`` (float64, snum) and, per trace, the first row of
    ``slice(int(trig) + 1, None)`` (int32, tnum; Python's slice semantics, so a trigger of -1 multiplies the whole
    trace and one of -3 its last two samples).  ``trig`` is a scalar or one value per trace."""
    gain = np.ascontiguousarray(np.asarray(travel_time, dtype=np.float64).flatten() * slope)
    if gain.shape != (snum,):
        raise ValueError('travel_time has %d samples but the data has %d' % (gain.size, snum))
    trig = np.asarray(trig)
    if trig.ndim == 0:
        trig = np.full((tnum,), trig.item())
    if trig.shape != (tnum,):
        raise ValueError('trig needs length tnum %d' % tnum)
    start = np.array([slice(int(t) + 1, None).indices(snum)[0] for t in trig], dtype=np.int32)
    return gain, start


def refuse_integers(dtype):
    """NumPy's refusal to store a float64 product in an integer array (the reference's ``UFuncTypeError``)."""
    if np.dtype(dtype).kind not in 'fc':
        raise TypeError("Cannot cast ufunc 'multiply' output from dtype('float64') to dtype('%s') with casting rule "
                        "'same_kind'" % np.dtype(dtype).name)


def _work(data):
    return _hip.work_array(data, 'gains on complex data are', copy=True)


def rangegain_host(data, gain, start):
    """Copy of a float host radargram with the range gain applied."""
    refuse_integers(np.asarray(data).dtype)
    work = _work(data)
    snum, tnum = work.shape
    rc = _hip.load().impdar_rangegain(_hip.context(), work.ctypes.data_as(C.c_void_p), _hip.dtype_code(work.dtype), snum,
                                     tnum, _hip.as_dp(gain)[1], start.ctypes.data_as(_IP))
    _hip.check(rc, 'impdar_rangegain')
    return work


def rangegain_dev(d_arr, gain, start):
    """In place on a resident :class:`impdar_amd._hip.DeviceArray` (float32 / float64)."""
    snum, tnum = d_arr.shape
    rc = _hip.load().impdar_rangegain_dev(d_arr.ctx, d_arr.ptr, _hip.dtype_code(d_arr.dtype), snum, tnum,
                                         _hip.as_dp(gain)[1], start.ctypes.data_as(_IP))
    _hip.check(rc, 'impdar_rangegain')


# ------------------------------------------------------------------------------------------------ agc
def agc_half(window):
    """``window // 2``, the rows taken above a sample (one fewer below it); 0 leaves nothing to take the maximum
    of, which is NumPy's error in the reference."""
    half = int(window) // 2
    if half < 1:
        raise ValueError('zero-size array to reduction operation maximum which has no identity')
    return half


def window_max(rowmax, half):
    """``maxamp`` of the reference from the row maxima: the maximum over rows ``[max(0, i - half), min(i + half,
    snum))``, NaN where one of them is NaN, zeros replaced by 1e-6."""
    snum = len(rowmax)
    maxamp = np.array([np.max(rowmax[max(0, i - half):min(i + half, snum)]) for i in range(snum)])
    maxamp[maxamp == 0] = 1.0e-6
    return maxamp


def row_absmax_host(data):
    """float64 ``max |data[i, :]|`` of every row of a host radargram, from the device (integers widened first)."""
    work = _hip.work_array(data, 'gains on complex data are', copy=False)
    snum, tnum = work.shape
    rowmax = np.empty((snum,), dtype=np.float64)
    rc = _hip.load().impdar_row_absmax(_hip.context(), work.ctypes.data_as(C.c_void_p), _hip.dtype_code(work.dtype), snum,
                                      tnum, _hip.as_dp(rowmax)[1])
    _hip.check(rc, 'impdar_row_absmax')
    return rowmax


def agc_host(data, half, scaling_factor):
    """Copy of a host radargram with the automatic gain applied, in its own dtype."""
    data = np.asarray(data)
    if data.dtype not in (np.float32, np.float64):
        scale = (scaling_factor / window_max(row_absmax_host(data), half)).astype(data.dtype)
        return data * scale[:, None]
    work = _work(data)
    snum, tnum = work.shape
    rc = _hip.load().impdar_agc(_hip.context(), work.ctypes.data_as(C.c_void_p), _hip.dtype_code(work.dtype), snum, tnum,
                               int(half), float(scaling_factor))
    _hip.check(rc, 'impdar_agc')
    return work


def agc_dev(d_arr, half, scaling_factor):
    """In place on a resident :class:`impdar_amd._hip.DeviceArray` (float32 / float64)."""
    snum, tnum = d_arr.shape
    rc = _hip.load().impdar_agc_dev(d_arr.ctx, d_arr.ptr, _hip.dtype_code(d_arr.dtype), snum, tnum, int(half),
                                   float(scaling_factor))
    _hip.check(rc, 'impdar_agc')
