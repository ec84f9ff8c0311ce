"""f-k fan (dip) filter and f-k power spectrum of a radargram (an extension: the reference has neither).

``fk_filter(dat, va_lo, va_hi, taper, mode, dip)`` multiplies the 2-D spectrum of ``dat`` by a real fan weight and
transforms back: events whose apparent velocity ``|w| / |kx|`` lies between ``va_lo`` and ``va_hi`` pass (or, with
``mode='reject'``, are removed), with raised-cosine tapers of relative width ``taper`` in slowness around either edge,
for events that dip either way or one way only.  ``fk_spectrum(dat)`` is ``|fft2|^2`` over the frequencies >= 0, the
wavenumbers in ``fftshift`` order -- what the fan is chosen from.  Both run on the transforms and the cached plan of the
Stolt migration (``csrc/fk.hip``), on a host radargram or on one held in HBM with ``to_device()``, which stays there.

The contract is stated once, in ``csrc/fk_weight.h``.  ``fan_host``, ``fan_dev``, ``power_host`` and ``power_dev`` are
the only functions here that reach the library.
"""
import ctypes as C
import math

import numpy as np

from . import _hip

MODES = {'pass': 0, 'reject': 1}
DIPS = {'both': 0, 'down_right': 1, 'down_left': 2}


def check_fan(shape, va_lo=None, va_hi=None, taper=0.1, mode='pass', dip='both'):
    """``(va_lo, va_hi, taper, mode code, dip code)`` for the C ABI (NaN: no edge), or ``ValueError``: neither edge
    given, an edge that is not finite and positive, ``taper`` outside [0, 1), overlapping tapers, a radargram with
    fewer than two samples or traces, an unknown mode or dip.  No device call."""
    if len(shape) != 2 or shape[0] < 2 or shape[1] < 2:
        raise ValueError('the f-k filter needs snum >= 2 and tnum >= 2, got %r' % (tuple(shape),))
    if mode not in MODES:
        raise ValueError("mode must be 'pass' or 'reject', got %r" % (mode,))
    if dip not in DIPS:
        raise ValueError("dip must be 'both', 'down_right' or 'down_left', got %r" % (dip,))
    if va_lo is None and va_hi is None:
        raise ValueError('give va_lo, va_hi or both')
    edges = []
    for name, va in (('va_lo', va_lo), ('va_hi', va_hi)):
        if va is None:
            edges.append(float('nan'))
            continue
        va = float(va)
        if not (math.isfinite(va) and va > 0.0):
            raise ValueError('%s must be finite and positive, got %r' % (name, va))
        edges.append(va)
    taper = float(taper)
    if not (0.0 <= taper < 1.0):
        raise ValueError('taper must lie in [0, 1), got %r' % (taper,))
    if va_lo is not None and va_hi is not None and (1.0 / edges[1]) * (1.0 + taper) > (1.0 / edges[0]) * (1.0 - taper):
        raise ValueError('the tapers of va_lo = %r and va_hi = %r overlap (taper %r)' % (edges[0], edges[1], taper))
    return edges[0], edges[1], taper, MODES[mode], DIPS[dip]


def fan_host(data, kx, ws, fan):
    """``impdar_fk_fan`` on a host array (float32 / float64, (snum, tnum)); ``fan`` from :func:`check_fan`.  A new array."""
    data = np.ascontiguousarray(data)
    snum, tnum = data.shape
    out = np.empty_like(data)
    rc = _hip.load().impdar_fk_fan(_hip.context(), data.ctypes.data_as(C.c_void_p), _hip.dtype_code(data.dtype), snum, tnum,
                                   _hip.as_dp(kx)[1], _hip.as_dp(ws)[1], fan[0], fan[1], fan[2], fan[3], fan[4],
                                   out.ctypes.data_as(C.c_void_p))
    _hip.check(rc, 'impdar_fk_fan')
    return out


def fan_dev(dev, kx, ws, fan, out=None):
    """``impdar_fk_fan_dev`` on a resident :class:`_hip.DeviceArray`, in place (or into ``out``)."""
    snum, tnum = dev.shape
    rc = _hip.load().impdar_fk_fan_dev(dev.ctx, dev.ptr, _hip.dtype_code(dev.dtype), snum, tnum, _hip.as_dp(kx)[1],
                                       _hip.as_dp(ws)[1], fan[0], fan[1], fan[2], fan[3], fan[4],
                                       (out if out is not None else dev).ptr)
    _hip.check(rc, 'impdar_fk_fan')
    return out if out is not None else dev


def power_host(data, kx, ws):
    """``impdar_fk_power`` on a host array: (snum // 2 + 1, tnum) float64."""
    data = np.ascontiguousarray(data)
    snum, tnum = data.shape
    out = np.empty((snum // 2 + 1, tnum), dtype=np.float64)
    rc = _hip.load().impdar_fk_power(_hip.context(), data.ctypes.data_as(C.c_void_p), _hip.dtype_code(data.dtype), snum, tnum,
                                     _hip.as_dp(kx)[1], _hip.as_dp(ws)[1], _hip.as_dp(out)[1])
    _hip.check(rc, 'impdar_fk_power')
    return out


def power_dev(dev, kx, ws):
    """``impdar_fk_power_dev`` on a resident :class:`_hip.DeviceArray`; only the spectrum comes back."""
    snum, tnum = dev.shape
    with _hip.new_device_array(dev.ctx, (snum // 2 + 1, tnum), np.float64) as d_out:
        rc = _hip.load().impdar_fk_power_dev(dev.ctx, dev.ptr, _hip.dtype_code(dev.dtype), snum, tnum, _hip.as_dp(kx)[1],
                                             _hip.as_dp(ws)[1], d_out.ptr)
        _hip.check(rc, 'impdar_fk_power')
    out = d_out.to_host()
    d_out.free()
    return out


def _axes(dat):
    from .lib.migrationlib.mig_hip import _kx
    return _kx(dat), 2. * np.pi * np.fft.rfftfreq(dat.snum, d=dat.dt)


def _shape(dat):
    from .lib.migrationlib.mig_hip import _check_data_shape
    dev = getattr(dat, '_dev', None)
    if dev is None:
        _check_data_shape(dat)
    elif dev.shape != (dat.snum, dat.tnum):
        raise ValueError('The input array must be of size (snum, tnum)')
    return dev, (int(dat.snum), int(dat.tnum))


def fk_filter(dat, va_lo=None, va_hi=None, taper=0.1, mode='pass', dip='both'):
    """Fan filter ``dat`` in place: ``y = Re ifft2(M * fft2(x))`` with the weight ``M`` of the module's docstring.

    ``va_lo`` / ``va_hi`` (m/s along the profile, one of them may be None): the apparent velocities that bound the fan;
    ``taper``: the relative half-width of the cosine tapers in slowness, in [0, 1); ``mode``: 'pass' or 'reject';
    ``dip``: 'both', 'down_right' (arrival time grows with distance) or 'down_left'.  Shape and dtype stay (integer data
    becomes float64); a resident radargram stays in HBM.  ``flags`` are left alone: the reference's flag struct has no
    slot for the step.  No zero padding: events wrap around the edges as in any DFT filter."""
    from .lib.migrationlib.mig_hip import _device_data
    dev, shape = _shape(dat)
    fan = check_fan(shape, va_lo, va_hi, taper, mode, dip)
    kx, ws = _axes(dat)
    if dev is not None:
        fan_dev(dev, kx, ws, fan)
    else:
        dat.data = fan_host(_device_data(dat.data)[0], kx, ws, fan)


def fk_spectrum(dat):
    """``(freq_MHz (m,), k_per_m (tnum,), P (m, tnum))`` with ``m = snum // 2 + 1``: ``P = |fft2(data)|^2`` (float64, not
    normalised) at the frequencies ``rfftfreq(snum, dt) / 1e6`` and the wavenumbers ``fftshift(fftfreq(tnum, dx))`` in
    cycles per metre, ``dx`` the mean trace spacing."""
    from .lib.migrationlib.mig_hip import _device_data
    dev, shape = _shape(dat)
    if shape[0] < 2 or shape[1] < 2:
        raise ValueError('the f-k spectrum needs snum >= 2 and tnum >= 2, got %r' % (shape,))
    kx, ws = _axes(dat)
    power = power_dev(dev, kx, ws) if dev is not None else power_host(_device_data(dat.data)[0], kx, ws)
    return ws / (2. * np.pi) * 1.0e-6, np.fft.fftshift(kx) / (2. * np.pi), power
