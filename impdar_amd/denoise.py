"""Host side of the denoise step an impproc chain runs between the horizontal filters and the re-spacing:
``scipy.signal.wiener`` and ``scipy.ndimage.median_filter`` over a (vert_win, hor_win) window.  Argument checks,
the widening of integer data and the reference's errors live here; everything that touches the (snum, tnum)
radargram runs in ``csrc/denoise.hip`` through the C ABI, on host buffers or on an array resident in HBM.

Reference: ``src/impdar/lib/RadarData/_RadarDataFiltering.py:552-587``.  Deliberate differences:

* integer data is widened to float64 before it is squared (the reference squares int16 in int16, which wraps);
  float32 keeps the reference's float32-rounded squares;
* with ``noise=None`` a flat window (``lVar == 0``) gives ``lMean``, as the reference's ``where`` selects; the
  reference's ``ValueError`` is raised only when the estimated noise is exactly 0 (every window flat);
* window sizes below 1 raise ``ValueError``;
* with ``noise`` given, an output is NaN exactly when its window holds a non-finite value; with ``noise=None``
  any non-finite input makes the whole output NaN, as in the reference.
"""
import ctypes as C

import numpy as np

from . import _hip

NOISE_MESSAGE = 'Could not compute variance, specify noise for denoise'
FTYPE_MESSAGE = 'Only the wiener filter has been implemented for denoising.'


def check_windows(vert_win, hor_win):
    """Two integers >= 1 (numpy integers included), returned as ints."""
    out = []
    for name, w in (('vert_win', vert_win), ('hor_win', hor_win)):
        if isinstance(w, (bool, np.bool_)) or not isinstance(w, (int, np.integer)):
            raise ValueError('%s must be an integer window size, got %r' % (name, w))
        if w < 1:
            raise ValueError('%s must be at least 1, got %d' % (name, w))
        out.append(int(w))
    if max(out) >= 1 << 30 or out[0] * out[1] > 0x7fffffff:
        raise ValueError('window of %d x %d elements is too large' % tuple(out))
    return out


def _work(data):
    work = _hip.work_array(data, 'denoising complex data is', copy=False)
    if work.size == 0:
        raise ValueError('data is empty')
    return work


def _noise_args(noise):
    if noise is None:
        return 0.0, 0
    return float(noise), 1


def _check_wiener(rc):
    if rc == _hip.ERR_ARG and _hip.last_error() == NOISE_MESSAGE:
        raise ValueError(NOISE_MESSAGE)                   # the reference's message, unprefixed
    _hip.check(rc, 'impdar_wiener')


def wiener_host(data, vert_win=1, hor_win=10, noise=None):
    """``scipy.signal.wiener(data, (vert_win, hor_win), noise)`` of a host radargram, float64.  Returns
    ``(out, noise_used)``."""
    m, n = check_windows(vert_win, hor_win)
    work = _work(data)
    snum, tnum = work.shape
    out = np.empty((snum, tnum), dtype=np.float64)
    nz, given = _noise_args(noise)
    used = C.c_double(0.0)
    rc = _hip.load().impdar_wiener(_hip.context(), work.ctypes.data_as(C.c_void_p), _hip.dtype_code(work.dtype),
                                   snum, tnum, m, n, nz, given, out.ctypes.data_as(_hip._dp), C.byref(used))
    _check_wiener(rc)
    return out, used.value


def wiener_dev(d_arr, vert_win=1, hor_win=10, noise=None):
    """Wiener filter of a resident :class:`impdar_amd._hip.DeviceArray` (float32 / float64) into a NEW resident
    float64 array; the caller frees the old one.  Returns ``(d_out, noise_used)``."""
    m, n = check_windows(vert_win, hor_win)
    snum, tnum = d_arr.shape
    nz, given = _noise_args(noise)
    used = C.c_double(0.0)
    with _hip.new_device_array(d_arr.ctx, (snum, tnum), np.float64) as d_out:
        rc = _hip.load().impdar_wiener_dev(d_arr.ctx, d_arr.ptr, _hip.dtype_code(d_arr.dtype), snum, tnum, m, n, nz,
                                           given, d_out.ptr, C.byref(used))
        _check_wiener(rc)
    return d_out, used.value


def median_host(data, vert_win=1, hor_win=10):
    """``scipy.ndimage.median_filter(data, size=(vert_win, hor_win))`` of a host radargram, in its own dtype
    (integers run widened to float64 and come back exactly)."""
    m, n = check_windows(vert_win, hor_win)
    data = np.asarray(data)
    work = _work(data)
    snum, tnum = work.shape
    out = np.empty_like(work)
    rc = _hip.load().impdar_median(_hip.context(), work.ctypes.data_as(C.c_void_p), _hip.dtype_code(work.dtype),
                                   snum, tnum, m, n, out.ctypes.data_as(C.c_void_p))
    _hip.check(rc, 'impdar_median')
    return out.astype(data.dtype) if out.dtype != data.dtype else out


def median_dev(d_arr, vert_win=1, hor_win=10):
    """Median filter of a resident array into a NEW resident array of the same dtype; the caller frees the old
    one."""
    m, n = check_windows(vert_win, hor_win)
    snum, tnum = d_arr.shape
    with _hip.new_device_array(d_arr.ctx, (snum, tnum), d_arr.dtype) as d_out:
        rc = _hip.load().impdar_median_dev(d_arr.ctx, d_arr.ptr, _hip.dtype_code(d_arr.dtype), snum, tnum, m, n,
                                           d_out.ptr)
        _hip.check(rc, 'impdar_median')
    return d_out
