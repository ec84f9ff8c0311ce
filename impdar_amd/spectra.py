"""Host side of the spectra of a radargram: the mean power spectrum along either axis (the reference's ``plot_ft`` and
``plot_hft``) and the periodogram of every trace (``plot_spectrogram``, through ``scipy.signal.periodogram``).  The
window and the scale factor -- O(snum) -- are formed here; everything that reads the (snum, tnum) radargram runs in
``csrc/spectrum.hip`` through the C ABI, on a host buffer or on an array that is already resident in HBM.  A mean
spectrum comes back as ``n`` doubles; the periodogram image as ``(snum // 2 + 1, tnum)`` float64, on the host or, with
``resident=True``, as a :class:`impdar_amd._hip.DeviceArray`.

Data of either float dtype is widened to float64 on load and all arithmetic is float64: the result is the reference's
on the data widened to float64 (NumPy >= 2 and SciPy keep float32 for float32 files).

Reference: ``src/impdar/lib/plot.py:310-312, 346-347, 654-674``.
"""
import ctypes as C

import numpy as np

from . import _hip


def _axis(axis):
    if axis not in (0, 1):
        raise ValueError('axis must be 0 (along the samples) or 1 (along the traces), got %r' % (axis,))
    return int(axis)


def _mean_spectrum(fn, ctx, ptr, dtype, shape, axis):
    snum, tnum = shape
    out = np.empty((shape[axis],), dtype=np.float64)
    if out.size == 0 or snum * tnum == 0:
        raise ValueError('the radargram is empty')
    _hip.check(fn(ctx, ptr, _hip.dtype_code(dtype), snum, tnum, axis, _hip.as_dp(out)[1]), 'impdar_mean_spectrum')
    return out


def mean_spectrum_host(data, axis):
    """``mean(abs(fft(data, axis=axis)) ** 2, axis=1 - axis)`` of a host radargram, float64, in ``fftfreq`` order."""
    axis = _axis(axis)
    work = _hip.work_array(data, 'spectra of complex data are', copy=False)
    return _mean_spectrum(_hip.load().impdar_mean_spectrum, _hip.context(), work.ctypes.data_as(C.c_void_p), work.dtype,
                          work.shape, axis)


def mean_spectrum_dev(d_arr, axis):
    """The same of a resident :class:`impdar_amd._hip.DeviceArray` (float32 / float64), which stays where it is."""
    axis = _axis(axis)
    return _mean_spectrum(_hip.load().impdar_mean_spectrum_dev, d_arr.ctx, d_arr.ptr, d_arr.dtype, d_arr.shape, axis)


def window_and_scale(snum, fs, window=None, scaling='density'):
    """``(w, scale)`` of ``scipy.signal.periodogram``: ``w`` the float64 window of ``snum`` samples (None for a boxcar,
    which multiplies nothing), ``scale`` what ``|rfft|**2`` is multiplied by.  Raises before any device call."""
    if scaling not in ('density', 'spectrum'):
        raise ValueError('Unknown scaling: %r' % scaling)
    fs = float(fs)
    if not (fs > 0.0 and np.isfinite(fs)):
        raise ValueError('fs must be positive, got %r' % (fs,))
    if window is None or isinstance(window, (str, tuple)):
        from scipy.signal import get_window
        w = np.asarray(get_window(window or 'boxcar', snum), dtype=np.float64)
    else:
        w = np.asarray(window, dtype=np.float64)
        if w.ndim != 1:
            raise ValueError('window must be 1-D')
        if w.shape[0] != snum:
            raise ValueError('window has length %d, the traces have %d samples' % (w.shape[0], snum))
    scale = 1.0 / w.sum() ** 2 if scaling == 'spectrum' else 1.0 / (fs * (w * w).sum())
    if not (np.isfinite(scale) and scale > 0.0):
        raise ValueError('the window sums to zero')
    boxcar = bool(np.all(w == 1.0))
    return (None if boxcar else np.ascontiguousarray(w)), float(scale)


def _periodogram(fn, ctx, ptr, dtype, shape, fs, window, scaling, out_ptr):
    snum, tnum = shape
    w, scale = window_and_scale(snum, fs, window, scaling)
    rc = fn(ctx, ptr, _hip.dtype_code(dtype), snum, tnum, None if w is None else _hip.as_dp(w)[1], scale, out_ptr)
    _hip.check(rc, 'impdar_periodogram')
    return np.fft.rfftfreq(snum, 1.0 / float(fs))


def _check_shape(shape):
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError('the radargram is empty')


def periodogram_host(data, fs, window=None, scaling='density'):
    """``scipy.signal.periodogram(data[:, t], fs, window, scaling=scaling)`` of every trace of a host radargram:
    ``(freq, power)`` with ``freq = rfftfreq(snum, 1 / fs)`` and ``power`` (snum // 2 + 1, tnum) float64."""
    work = _hip.work_array(data, 'spectra of complex data are', copy=False)
    _check_shape(work.shape)
    window_and_scale(work.shape[0], fs, window, scaling)        # (errors before the library is loaded)
    out = np.empty((work.shape[0] // 2 + 1, work.shape[1]), dtype=np.float64)
    freq = _periodogram(_hip.load().impdar_periodogram, _hip.context(), work.ctypes.data_as(C.c_void_p), work.dtype, work.shape,
                        fs, window, scaling, out.ctypes.data_as(C.c_void_p))
    return freq, out


def periodogram_dev(d_arr, fs, window=None, scaling='density', resident=False):
    """The same of a resident :class:`impdar_amd._hip.DeviceArray`; ``resident=True`` leaves the image in HBM and returns
    a ``DeviceArray`` in place of the host array."""
    _check_shape(d_arr.shape)
    window_and_scale(d_arr.shape[0], fs, window, scaling)
    with _hip.new_device_array(d_arr.ctx, (d_arr.shape[0] // 2 + 1, d_arr.shape[1]), np.float64) as d_out:
        freq = _periodogram(_hip.load().impdar_periodogram_dev, d_arr.ctx, d_arr.ptr, d_arr.dtype, d_arr.shape, fs, window,
                            scaling, d_out.ptr)
    if resident:
        return freq, d_out
    out = d_out.to_host()
    d_out.free()
    return freq, out
