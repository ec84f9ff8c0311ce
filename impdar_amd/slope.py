"""Layer slopes of a radargram: the structure-tensor dip field and the mean along the layers (an extension: the reference
has no slope field).

``layer_slope`` gives, for every sample, the local slope of the internal layers in samples per trace (or their dip in
radians, the coherence of the estimate, or a component of the smoothed structure tensor); ``dip_smooth`` averages every
sample over ``2 half + 1`` traces *along* that slope, which does not cancel a dipping layer as a mean along the rows
does.  All of it runs in HIP (``csrc/slope.hip``) in float64, on a host radargram or on one held in HBM with
``to_device()``, which stays there.

The contract is stated once, in ``csrc/slope_route.h``.  ``slope_host``, ``slope_dev``, ``dipsmooth_host`` and
``dipsmooth_dev`` are the only functions here that reach the library.
"""
import ctypes as C
import math

import numpy as np

from . import _hip

KINDS = {'slope': 0, 'dip': 1, 'coherence': 2, 'jzz': 3, 'jzx': 4, 'jxx': 5}
MAX_SIGMA = 16.0
MAX_HALF = 32


def _check_shape(shape, dtype):
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError('empty radargram: %r' % (tuple(shape),))
    if dtype is not None and np.dtype(dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError('dtype must be float32 or float64, got %s' % np.dtype(dtype))


def _check_sigma(sigma, max_slope):
    try:
        sz, sx = (float(s) for s in sigma)
    except (TypeError, ValueError):
        raise ValueError('sigma must be a pair (sigma_z, sigma_x), got %r' % (sigma,))
    for s in (sz, sx):
        if not (math.isfinite(s) and 0.0 <= s <= MAX_SIGMA):
            raise ValueError('sigma must be finite and lie in 0 .. 16, got %r' % (sigma,))
    max_slope = float(max_slope)
    if not (math.isfinite(max_slope) and max_slope > 0.0):
        raise ValueError('max_slope must be finite and positive, got %r' % (max_slope,))
    return sz, sx, max_slope


def check_slope(shape, kind='slope', sigma=(2.0, 8.0), max_slope=4.0, dtype=None):
    """``(kind code, sigma_z, sigma_x, max_slope)`` for the C ABI, or ``ValueError`` with the reason of
    ``csrc/slope_route.h``: an unknown ``kind`` (a name of ``KINDS`` or its code), a sigma that is not finite, negative
    or above 16, a ``max_slope`` that is not finite or not positive, an empty radargram, a ``dtype`` other than
    float32 / float64.  No device call."""
    code = KINDS.get(kind, kind) if isinstance(kind, str) else kind
    if isinstance(code, bool) or not isinstance(code, (int, np.integer)) or code not in KINDS.values():
        raise ValueError('kind must be 0 (slope), 1 (dip), 2 (coherence), 3 (jzz), 4 (jzx) or 5 (jxx), got %r' % (kind,))
    sz, sx, max_slope = _check_sigma(sigma, max_slope)
    _check_shape(shape, dtype)
    return int(code), sz, sx, max_slope


def check_dipsmooth(shape, half, sigma=(2.0, 8.0), max_slope=4.0, slope=None, dtype=None):
    """``(half, sigma_z, sigma_x, max_slope)`` or ``ValueError``: ``half`` outside 1 .. 32; with no ``slope`` given, what
    :func:`check_slope` refuses; a given ``slope`` (a host array or a :class:`_hip.DeviceArray`) that is not float64 of
    the radargram's shape; an empty radargram; another ``dtype``.  No device call."""
    if isinstance(half, bool) or not isinstance(half, (int, np.integer)) or not (1 <= half <= MAX_HALF):
        raise ValueError('half must lie in 1 .. 32, got %r' % (half,))
    if slope is None:
        sz, sx, max_slope = _check_sigma(sigma, max_slope)
    else:
        sz, sx, max_slope = 0.0, 0.0, 1.0           # (not read)
        if tuple(slope.shape) != tuple(shape) or np.dtype(slope.dtype) != np.dtype(np.float64):
            raise ValueError('slope must be a float64 array of shape %r, got %s %r' % (tuple(shape), slope.dtype, tuple(slope.shape)))
    _check_shape(shape, dtype)
    return int(half), sz, sx, max_slope


def slope_host(data, args):
    """``impdar_slope`` on a host array (float32 / float64, (snum, tnum)); ``args`` from :func:`check_slope`.  A new
    float64 array."""
    data = np.ascontiguousarray(data)
    snum, tnum = data.shape
    kind, sz, sx, max_slope = args
    out = np.empty((snum, tnum), dtype=np.float64)
    rc = _hip.load().impdar_slope(_hip.context(), data.ctypes.data_as(C.c_void_p), _hip.dtype_code(data.dtype), snum, tnum, kind, sz, sx,
                                  max_slope, _hip.as_dp(out)[1])
    _hip.check(rc, 'impdar_slope')
    return out


def slope_dev(dev, args, out):
    """``impdar_slope_dev`` on a resident :class:`_hip.DeviceArray` into ``out``, a float64 one of the same shape."""
    snum, tnum = dev.shape
    kind, sz, sx, max_slope = args
    if out.shape != dev.shape or out.dtype != np.float64:
        raise ValueError('the field is a float64 array of shape %r' % (dev.shape,))
    rc = _hip.load().impdar_slope_dev(dev.ctx, dev.ptr, _hip.dtype_code(dev.dtype), snum, tnum, kind, sz, sx, max_slope, out.ptr)
    _hip.check(rc, 'impdar_slope')
    return out


def dipsmooth_host(data, args, slope=None):
    """``impdar_dipsmooth`` on a host array; ``args`` from :func:`check_dipsmooth`, ``slope`` the float64 host array
    given to it (or none).  A new array of the data's dtype."""
    data = np.ascontiguousarray(data)
    snum, tnum = data.shape
    half, sz, sx, max_slope = args
    out = np.empty_like(data)
    keep, ptr = _hip.as_dp(slope)
    rc = _hip.load().impdar_dipsmooth(_hip.context(), data.ctypes.data_as(C.c_void_p), _hip.dtype_code(data.dtype), snum, tnum, half, ptr,
                                      sz, sx, max_slope, out.ctypes.data_as(C.c_void_p))
    _hip.check(rc, 'impdar_dipsmooth')
    return out


def dipsmooth_dev(dev, args, slope=None, out=None):
    """``impdar_dipsmooth_dev`` on a resident :class:`_hip.DeviceArray`, in place (or into ``out``); ``slope`` a resident
    float64 array (or none)."""
    snum, tnum = dev.shape
    half, sz, sx, max_slope = args
    res = out if out is not None else dev
    rc = _hip.load().impdar_dipsmooth_dev(dev.ctx, dev.ptr, _hip.dtype_code(dev.dtype), snum, tnum, half,
                                          slope.ptr if slope is not None else None, sz, sx, max_slope, res.ptr)
    _hip.check(rc, 'impdar_dipsmooth')
    return res


def _shape(dat):
    from .lib.migrationlib.mig_hip import _check_data_shape
    dev = getattr(dat, '_dev', None)
    if dev is None:
        _check_data_shape(dat)
        if np.iscomplexobj(dat.data):
            raise TypeError('layer slopes of complex data are not supported by the MI355X engine')
    elif dev.shape != (dat.snum, dat.tnum):
        raise ValueError('The input array must be of size (snum, tnum)')
    return dev, (int(dat.snum), int(dat.tnum))


def layer_slope(dat, sigma=(2.0, 8.0), kind='slope', max_slope=4.0):
    """The float64 (snum, tnum) host array of one field of the layers' local orientation, with the data untouched.

    ``kind``: 'slope' -- samples per trace along the layer, clamped to ``+-max_slope``; 'dip' -- its angle in radians,
    not clamped; 'coherence' -- how well one orientation describes the neighbourhood, 0 .. 1; 'jzz', 'jzx', 'jxx' -- the
    smoothed structure tensor itself.  ``sigma = (sigma_z, sigma_x)``: the Gaussian neighbourhood in samples and in
    traces (each 0 .. 16; 0 leaves the axis alone).  A sample that is not finite makes the field NaN within the
    neighbourhood's reach."""
    from .lib.migrationlib.mig_hip import _device_data
    dev, shape = _shape(dat)
    args = check_slope(shape, kind, sigma, max_slope)
    if dev is not None:
        with _hip.new_device_array(dev.ctx, dev.shape, np.float64) as d_tmp:
            slope_dev(dev, args, d_tmp)
        out = d_tmp.to_host()
        d_tmp.free()
        return out
    return slope_host(_device_data(dat.data)[0], args)


def dip_smooth(dat, half, sigma=(2.0, 8.0), max_slope=4.0, slope=None):
    """Replace every sample of ``dat`` by the mean over the ``2 half + 1`` traces around it (those inside the radargram),
    each read -- linearly interpolated -- where the layer through the sample crosses it: at ``k + p i`` for trace
    ``j + i``, ``p`` the slope at the sample.  ``slope``: a float64 (snum, tnum) array, for instance an edited
    :func:`layer_slope`; with none given it is ``layer_slope(dat, sigma, 'slope', max_slope)``, computed first and never
    rounded.  ``half``: 1 .. 32.  Shape and dtype stay (integer data becomes float64); a resident radargram stays in HBM.
    A NaN slope gives a NaN sample.  ``flags`` are left alone: the reference's flag struct has no slot for the step."""
    from .lib.migrationlib.mig_hip import _device_data
    dev, shape = _shape(dat)
    if slope is not None and not isinstance(slope, _hip.DeviceArray):
        slope = np.asarray(slope)
    args = check_dipsmooth(shape, half, sigma, max_slope, slope)
    if dev is None:
        if isinstance(slope, _hip.DeviceArray):
            slope = slope.to_host()
        dat.data = dipsmooth_host(_device_data(dat.data)[0], args, slope)
    elif slope is None or isinstance(slope, _hip.DeviceArray):
        dipsmooth_dev(dev, args, slope)
    else:
        d_slope = _hip.DeviceArray.from_host(dev.ctx, slope)
        try:
            dipsmooth_dev(dev, args, d_slope)
        finally:
            d_slope.free()
