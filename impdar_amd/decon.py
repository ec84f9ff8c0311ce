"""Predictive (gapped, Wiener-Levinson) deconvolution and the autocorrelogram of a radargram (an extension: the reference
has neither).

``predictive_decon(dat, oplen, gap, prewhiten, window, design)`` shortens the wavelet of every trace: from the trace's
autocorrelation over the design window it finds the ``oplen``-sample operator that predicts the trace ``gap`` samples
ahead and subtracts the prediction -- ringing, a long source pulse and short-period multiples are predictable, the
reflectivity is not.  ``gap=1`` is spiking deconvolution.  ``autocorrelation(dat, maxlag)`` is the picture ``gap`` and
``oplen`` are chosen from.  Both run in HIP (``csrc/decon.hip``), on a host radargram or on one held in HBM with
``to_device()``, which stays there.

The contract is stated once, in ``csrc/decon_core.h``.  ``decon_host``, ``decon_dev``, ``acorr_host`` and ``acorr_dev``
are the only functions here that reach the library.
"""
import ctypes as C
import math

import numpy as np

from . import _hip

DESIGNS = {'each': 0, 'mean': 1}
MAX_OPLEN = 256


def _window(snum, window):
    if window is None:
        return 0, int(snum)
    s0, s1 = window
    if int(s0) != s0 or int(s1) != s1:
        raise ValueError('the window must be a pair of sample indices, got %r' % (window,))
    return int(s0), int(s1)


def _check_window(shape, window):
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError('empty radargram: %r' % (tuple(shape),))
    s0, s1 = _window(shape[0], window)
    if not (0 <= s0 < s1 <= shape[0]):
        raise ValueError('the window must satisfy 0 <= s0 < s1 <= snum, got [%d, %d) of %d samples' % (s0, s1, shape[0]))
    return s0, s1


def check_decon(shape, oplen, gap=1, prewhiten=0.1, window=None, design='each'):
    """``(s0, s1, oplen, gap, prewhiten, design code)`` for the C ABI, or ``ValueError`` with the reason of
    ``csrc/decon_route.h``: ``oplen`` outside 1 .. 256, ``gap`` below 1, a window that is not ``0 <= s0 < s1 <= snum``,
    ``gap + oplen`` above the window's length, ``prewhiten`` negative or not finite, an unknown ``design``.  No device
    call."""
    s0, s1 = _check_window(shape, window)
    if int(oplen) != oplen or not (1 <= oplen <= MAX_OPLEN):
        raise ValueError('oplen must lie in 1 .. %d, got %r' % (MAX_OPLEN, oplen))
    if int(gap) != gap or gap < 1:
        raise ValueError('gap must be at least 1, got %r' % (gap,))
    if int(gap) + int(oplen) > s1 - s0:
        raise ValueError("gap + oplen must not exceed the window's length: %d + %d > %d" % (gap, oplen, s1 - s0))
    prewhiten = float(prewhiten)
    if not (math.isfinite(prewhiten) and prewhiten >= 0.0):
        raise ValueError('prewhiten must be finite and not negative, got %r' % (prewhiten,))
    if design not in DESIGNS:
        raise ValueError("design must be 'each' or 'mean', got %r" % (design,))
    return s0, s1, int(oplen), int(gap), prewhiten, DESIGNS[design]


def check_acorr(shape, maxlag, window=None):
    """``(s0, s1, maxlag)`` or ``ValueError``: a bad window, ``maxlag`` negative or not below the window's length."""
    s0, s1 = _check_window(shape, window)
    if int(maxlag) != maxlag or maxlag < 0:
        raise ValueError('maxlag must not be negative, got %r' % (maxlag,))
    if maxlag >= s1 - s0:
        raise ValueError("maxlag must be below the window's length: %d >= %d" % (maxlag, s1 - s0))
    return s0, s1, int(maxlag)


def decon_host(data, args, operators=False):
    """``impdar_decon`` on a host array (float32 / float64, (snum, tnum)); ``args`` from :func:`check_decon`.  A new
    array, and with ``operators`` the (oplen, tnum) float64 operators as well."""
    data = np.ascontiguousarray(data)
    snum, tnum = data.shape
    s0, s1, oplen, gap, prewhiten, design = args
    out = np.empty_like(data)
    ops = np.empty((oplen, tnum), dtype=np.float64) if operators else None
    rc = _hip.load().impdar_decon(_hip.context(), data.ctypes.data_as(C.c_void_p), _hip.dtype_code(data.dtype), snum, tnum, s0, s1,
                                  oplen, gap, prewhiten, design, out.ctypes.data_as(C.c_void_p), _hip.as_dp(ops)[1])
    _hip.check(rc, 'impdar_decon')
    return (out, ops) if operators else out


def decon_dev(dev, args, out=None, operators=False):
    """``impdar_decon_dev`` on a resident :class:`_hip.DeviceArray`, in place (or into ``out``); with ``operators`` the
    host copy of the (oplen, tnum) operators is returned beside it."""
    snum, tnum = dev.shape
    s0, s1, oplen, gap, prewhiten, design = args
    res = out if out is not None else dev
    d_op = _hip.DeviceArray(dev.ctx, (oplen, tnum), np.float64) if operators else None
    try:
        rc = _hip.load().impdar_decon_dev(dev.ctx, dev.ptr, _hip.dtype_code(dev.dtype), snum, tnum, s0, s1, oplen, gap, prewhiten,
                                          design, res.ptr, d_op.ptr if operators else None)
        _hip.check(rc, 'impdar_decon')
        return (res, d_op.to_host()) if operators else res
    finally:
        if d_op is not None:
            d_op.free()


def acorr_host(data, args, normalize=True):
    """``impdar_acorr`` on a host array: (maxlag + 1, tnum) float64; ``args`` from :func:`check_acorr`."""
    data = np.ascontiguousarray(data)
    snum, tnum = data.shape
    s0, s1, maxlag = args
    out = np.empty((maxlag + 1, tnum), dtype=np.float64)
    rc = _hip.load().impdar_acorr(_hip.context(), data.ctypes.data_as(C.c_void_p), _hip.dtype_code(data.dtype), snum, tnum, s0, s1,
                                  maxlag, 1 if normalize else 0, _hip.as_dp(out)[1])
    _hip.check(rc, 'impdar_acorr')
    return out


def acorr_dev(dev, args, normalize=True):
    """``impdar_acorr_dev`` on a resident :class:`_hip.DeviceArray`; only the autocorrelogram comes back."""
    snum, tnum = dev.shape
    s0, s1, maxlag = args
    with _hip.new_device_array(dev.ctx, (maxlag + 1, tnum), np.float64) as d_out:
        rc = _hip.load().impdar_acorr_dev(dev.ctx, dev.ptr, _hip.dtype_code(dev.dtype), snum, tnum, s0, s1, maxlag,
                                          1 if normalize else 0, d_out.ptr)
        _hip.check(rc, 'impdar_acorr')
    out = d_out.to_host()
    d_out.free()
    return out


def _shape(dat):
    from .lib.migrationlib.mig_hip import _check_data_shape
    dev = getattr(dat, '_dev', None)
    if dev is None:
        _check_data_shape(dat)
    elif dev.shape != (dat.snum, dat.tnum):
        raise ValueError('The input array must be of size (snum, tnum)')
    return dev, (int(dat.snum), int(dat.tnum))


def predictive_decon(dat, oplen, gap=1, prewhiten=0.1, window=None, design='each'):
    """Predictive deconvolution of ``dat`` in place.

    ``oplen`` (1 .. 256): the operator's length in samples -- as long as the wavelet or the multiple's period train
    to be removed; ``gap`` (>= 1): the prediction distance in samples -- 1 spikes the wavelet, the wavelet's wanted
    length keeps it, a multiple's period removes the multiple; ``prewhiten``: per cent of the zero lag added to it
    (stabilises the solve); ``window``: ``(s0, s1)``, the samples the operator is designed on (default: the whole
    trace; it is applied to the whole trace); ``design``: 'each' (every trace its own operator) or 'mean' (one operator
    from the autocorrelations summed over the traces).  Shape and dtype stay (integer data becomes float64); a
    resident radargram stays in HBM.  Traces that are all zero or not finite inside the window pass unchanged.
    ``flags`` are left alone: the reference's flag struct has no slot for the step."""
    from .lib.migrationlib.mig_hip import _device_data
    dev, shape = _shape(dat)
    args = check_decon(shape, oplen, gap, prewhiten, window, design)
    if dev is not None:
        decon_dev(dev, args)
    else:
        dat.data = decon_host(_device_data(dat.data)[0], args)


def decon_operators(dat, oplen, gap=1, prewhiten=0.1, window=None, design='each'):
    """The (oplen, tnum) float64 prediction operators :func:`predictive_decon` would apply (zeros for a trace that
    passes unchanged), with the data untouched."""
    from .lib.migrationlib.mig_hip import _device_data
    dev, shape = _shape(dat)
    args = check_decon(shape, oplen, gap, prewhiten, window, design)
    if dev is not None:
        with _hip.new_device_array(dev.ctx, dev.shape, dev.dtype) as d_tmp:
            ops = decon_dev(dev, args, out=d_tmp, operators=True)[1]
        d_tmp.free()
        return ops
    return decon_host(_device_data(dat.data)[0], args, operators=True)[1]


def autocorrelation(dat, maxlag, window=None, normalize=True):
    """``(lag_times_s (maxlag + 1,), A (maxlag + 1, tnum))``: ``A[l, j] = sum_k x_j[k] x_j[k + l]`` over the window
    (default: the whole trace), float64, divided by ``A[0, j]`` when ``normalize`` (a dead trace's column is NaN then);
    the lag times are ``arange(maxlag + 1) * dt``."""
    from .lib.migrationlib.mig_hip import _device_data
    dev, shape = _shape(dat)
    args = check_acorr(shape, maxlag, window)
    A = acorr_dev(dev, args, normalize) if dev is not None else acorr_host(_device_data(dat.data)[0], args, normalize)
    return np.arange(args[2] + 1) * float(dat.dt), A
