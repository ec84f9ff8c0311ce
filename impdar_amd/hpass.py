"""Host side of the horizontal frequency filters an impproc chain runs after ``constant_space``:
``horizontal_band_pass``, ``highpass`` and ``lowpass``, a Butterworth ``scipy.signal.filtfilt`` along the trace
axis.  The checks, the corner frequencies and the design (SciPy, so that its exceptions are the reference's own)
live here; the filtering of the (snum, tnum) radargram runs in ``csrc/hpass.hip`` through the C ABI, on host
buffers or on an array resident in HBM.

Reference: ``src/impdar/lib/RadarData/_RadarDataFiltering.py:138-350``.  One deliberate difference (DESIGN.md
4.7): integer data is widened to float64 before the odd extension.  The reference forms ``2 * x0 - x`` of an
int16 radargram in int16, which wraps wherever the extension leaves the int16 range.
"""
import ctypes as C

import numpy as np

from . import _hip
from .lib.ImpdarError import ImpdarError

INTERP_MESSAGE = 'This method can only be used on constantly spaced data'
ELEV_MESSAGE = 'This will not work with elevation corrected data'
PADLEN_MESSAGE = 'The length of the input vector x must be greater than padlen, which is {:d}.'
FSAMP = 100.   # the reference's approximate sampling frequency (10 ns ~ 10 m -> 100 MHz)


def trace_spacing(flags):
    """``flags.interp[1]`` after the reference's two flag checks."""
    if flags.interp is None or not flags.interp[0]:
        raise ImpdarError(INTERP_MESSAGE)
    if flags.elev:
        raise ImpdarError(ELEV_MESSAGE)
    return flags.interp[1]


def _spec(b, a):
    """(b, a, zi) as float64 arrays of one length, zi = ``lfilter_zi(b, a)`` (SciPy's own solve)."""
    from scipy import signal
    zi = signal.lfilter_zi(b, a)
    n = max(len(a), len(b))
    b = np.r_[b, np.zeros(n - len(b))]
    a = np.r_[a, np.zeros(n - len(a))]
    return (np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(a, dtype=np.float64),
            np.ascontiguousarray(zi, dtype=np.float64))


def band_pass_design(low, high, tracespace, tnum):
    """(b, a, zi) of ``horizontal_band_pass(low, high)`` (:311-345), with its checks and messages."""
    from scipy.signal import butter
    if low >= high:
        raise ValueError('Low must be less than high')
    if low <= 0.0:
        raise ValueError('Low must be larger than 0 but is {:f}'.format(low))
    nsamp_high = int(low / tracespace)
    nsamp_low = int(high / tracespace)
    if nsamp_high < 1:
        raise ValueError('Minimum wavelength is too small, causing no samples per wavelength')
    if nsamp_low > tnum:
        raise ValueError('Maximum wavelength is too long, causing more samples per wavelength than tnum, use '
                         'lowpass instead?')
    print('Sample resolution high = {:d}'.format(nsamp_high))
    print('Sample resolution low = {:d}'.format(nsamp_low))
    high_corner_freq = FSAMP / float(nsamp_high)
    low_corner_freq = FSAMP / float(nsamp_low)
    nyquist_freq = FSAMP / 2.0
    corner_freq = np.zeros((2,))
    corner_freq[0] = low_corner_freq / nyquist_freq
    corner_freq[1] = high_corner_freq / nyquist_freq
    b, a = butter(5, corner_freq, 'bandpass')
    return _spec(b, a)


def pass_design(kind, wavelength, tracespace, tnum, dt):
    """(b, a, zi) of ``highpass(wavelength)`` (kind 'high', :180-206) or ``lowpass(wavelength)`` (kind 'low',
    :250-276).  The corner ``(100 / nsamp) MHz / (0.5 / dt)`` mixes units as the reference's does."""
    from scipy.signal import butter
    wavelength = int(wavelength)
    nsamp = int(wavelength / tracespace)
    if nsamp < 1:
        raise ValueError('wavelength is too small, causing no samples per wavelength')
    if nsamp > tnum:
        raise ValueError('wavelength is too large, bigger than the whole radargram')
    print('Sample resolution = {:d}'.format(nsamp))
    high_corner_freq = FSAMP / float(nsamp)
    print('{:s} cutoff at {:4.2f} MHz...'.format('High' if kind == 'high' else 'Low', high_corner_freq))
    sample_freq = 1. / dt
    nyquist_freq = sample_freq / 2.0
    high_corner_freq = high_corner_freq * 1.0e6
    corner_freq = high_corner_freq / nyquist_freq
    if kind == 'high':
        b, a = butter(5, corner_freq, 'high')
    else:
        b, a = butter(3, corner_freq, 'low')
    return _spec(b, a)


def check_length(spec, tnum):
    """``scipy.signal.filtfilt``'s padlen guard, raised before any data is touched."""
    padlen = 3 * len(spec[0])
    if tnum <= padlen:
        raise ValueError(PADLEN_MESSAGE.format(padlen))


def _call(fn, ctx, ptr, code, snum, tnum, spec, out_ptr):
    b, a, zi = spec
    rc = fn(ctx, ptr, code, snum, tnum, _hip.as_dp(b)[1], _hip.as_dp(a)[1], len(b), _hip.as_dp(zi)[1], out_ptr)
    _hip.check(rc, 'impdar_hfiltfilt')


def filtfilt_host(data, spec):
    """``filtfilt(b, a, data, axis=1)`` of a host radargram as a new float64 array (integers widened first)."""
    work = _hip.work_array(data, 'horizontal filtering of complex data is', copy=False)
    snum, tnum = work.shape
    check_length(spec, tnum)
    out = np.empty((snum, tnum), dtype=np.float64)
    if out.size == 0:
        return out
    _call(_hip.load().impdar_hfiltfilt, _hip.context(), work.ctypes.data_as(C.c_void_p), _hip.dtype_code(work.dtype),
          snum, tnum, spec, out.ctypes.data_as(_hip._dp))
    return out


def filtfilt_dev(d_arr, spec):
    """``filtfilt(b, a, ., axis=1)`` of a resident array.  float64 is filtered in place and returned; float32
    goes to a NEW resident float64 array, and the caller frees the old one."""
    snum, tnum = d_arr.shape
    check_length(spec, tnum)
    lib = _hip.load()
    if d_arr.dtype == np.float64:
        _call(lib.impdar_hfiltfilt_dev, d_arr.ctx, d_arr.ptr, _hip.dtype_code(d_arr.dtype), snum, tnum, spec,
              d_arr.ptr)
        return d_arr
    with _hip.new_device_array(d_arr.ctx, (snum, tnum), np.float64) as d_out:
        _call(lib.impdar_hfiltfilt_dev, d_arr.ctx, d_arr.ptr, _hip.dtype_code(d_arr.dtype), snum, tnum, spec,
              d_out.ptr)
    return d_out
