"""Complex-trace attributes of a radargram: reflection strength, instantaneous phase and instantaneous frequency (an
extension: the reference has no Hilbert transform).

Every trace ``x`` gets its quadrature ``q = imag(scipy.signal.hilbert(x))`` and, from the analytic signal
``z = x + 1j q``, the envelope ``|z|`` (``envelope``), the phase ``arg z`` in radians (``instantaneous_phase``) or the
frequency ``arg(z[k + 1] conj z[k]) / (2 pi dt)`` in Hz (``instantaneous_frequency``, with ``smooth=W`` its mean over
``W`` samples weighted by ``|z|^2``).  All of it runs in HIP (``csrc/attr.hip``) in float64, on a host radargram or on
one held in HBM with ``to_device()``, which stays there.

The contract is stated once, in ``csrc/attr_route.h``.  ``attr_host`` and ``attr_dev`` are the only functions here that
reach the library.
"""
import ctypes as C
import math

import numpy as np

from . import _hip

KINDS = {'quadrature': 0, 'envelope': 1, 'phase': 2, 'frequency': 3}
MAX_SMOOTH = 255


def check_attr(shape, kind, smooth=1, dt=1.0):
    """``(kind code, smooth, dt)`` for the C ABI, or ``ValueError`` with the reason of ``csrc/attr_route.h``: an unknown
    ``kind`` (a name of ``KINDS`` or its code), ``smooth`` even or outside 1 .. 255, ``smooth > 1`` with a kind other than
    frequency, ``dt`` not finite or not positive (frequency only), an empty radargram.  No device call."""
    code = KINDS.get(kind, kind) if isinstance(kind, str) else kind
    if isinstance(code, bool) or not isinstance(code, (int, np.integer)) or code not in KINDS.values():
        raise ValueError('kind must be 0 (quadrature), 1 (envelope), 2 (phase) or 3 (frequency), got %r' % (kind,))
    if isinstance(smooth, bool) or int(smooth) != smooth or not (1 <= smooth <= MAX_SMOOTH) or int(smooth) % 2 == 0:
        raise ValueError('smooth must be odd and lie in 1 .. %d, got %r' % (MAX_SMOOTH, smooth))
    if smooth > 1 and code != KINDS['frequency']:
        raise ValueError('smooth above 1 goes with kind 3 (frequency) alone, got kind %r' % (kind,))
    if code == KINDS['frequency']:
        dt = float(dt)
        if not (math.isfinite(dt) and dt > 0.0):
            raise ValueError('dt must be finite and positive, got %r' % (dt,))
    else:
        dt = 1.0            # (not read)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError('empty radargram: %r' % (tuple(shape),))
    return int(code), int(smooth), dt


def attr_host(data, args):
    """``impdar_attr`` on a host array (float32 / float64, (snum, tnum)); ``args`` from :func:`check_attr`.  A new array."""
    data = np.ascontiguousarray(data)
    snum, tnum = data.shape
    kind, smooth, dt = args
    out = np.empty_like(data)
    rc = _hip.load().impdar_attr(_hip.context(), data.ctypes.data_as(C.c_void_p), _hip.dtype_code(data.dtype), snum, tnum, kind, smooth,
                                 dt, out.ctypes.data_as(C.c_void_p))
    _hip.check(rc, 'impdar_attr')
    return out


def attr_dev(dev, args, out=None):
    """``impdar_attr_dev`` on a resident :class:`_hip.DeviceArray`, in place (or into ``out``)."""
    snum, tnum = dev.shape
    kind, smooth, dt = args
    res = out if out is not None else dev
    rc = _hip.load().impdar_attr_dev(dev.ctx, dev.ptr, _hip.dtype_code(dev.dtype), snum, tnum, kind, smooth, dt, res.ptr)
    _hip.check(rc, 'impdar_attr')
    return res


def _shape(dat):
    from .lib.migrationlib.mig_hip import _check_data_shape
    dev = getattr(dat, '_dev', None)
    if dev is None:
        _check_data_shape(dat)
        if np.iscomplexobj(dat.data):
            raise TypeError('attributes of complex data are not supported by the MI355X engine')
    elif dev.shape != (dat.snum, dat.tnum):
        raise ValueError('The input array must be of size (snum, tnum)')
    return dev, (int(dat.snum), int(dat.tnum))


def complex_attribute(dat, kind, smooth=1):
    """The (snum, tnum) array of one attribute -- ``kind`` 'quadrature', 'envelope', 'phase' or 'frequency' -- in the
    radargram's dtype (integer data: float64), with the data untouched."""
    from .lib.migrationlib.mig_hip import _device_data
    dev, shape = _shape(dat)
    args = check_attr(shape, kind, smooth, dat.dt)
    if dev is not None:
        with _hip.new_device_array(dev.ctx, dev.shape, dev.dtype) as d_tmp:
            attr_dev(dev, args, out=d_tmp)
        out = d_tmp.to_host()
        d_tmp.free()
        return out
    return attr_host(_device_data(dat.data)[0], args)


def _in_place(dat, kind, smooth=1):
    from .lib.migrationlib.mig_hip import _device_data
    dev, shape = _shape(dat)
    args = check_attr(shape, kind, smooth, dat.dt)
    if dev is not None:
        attr_dev(dev, args)
    else:
        dat.data = attr_host(_device_data(dat.data)[0], args)


def envelope(dat):
    """Replace ``dat.data`` by its envelope (reflection strength) ``hypot(x, q)``, trace by trace.  Shape and dtype stay
    (integer data becomes float64); a resident radargram stays in HBM.  A trace with a sample that is not finite becomes
    NaN throughout.  ``flags`` are left alone: the reference's flag struct has no slot for the step."""
    _in_place(dat, 'envelope')


def instantaneous_phase(dat):
    """Replace ``dat.data`` by the instantaneous phase ``atan2(q, x)`` in radians, in (-pi, pi]; otherwise as
    :func:`envelope`."""
    _in_place(dat, 'phase')


def instantaneous_frequency(dat, smooth=1):
    """Replace ``dat.data`` by the instantaneous frequency in Hz, ``arg(z[k + 1] conj z[k]) / (2 pi dat.dt)`` (the last
    sample repeats the one before it); ``smooth`` (odd, 1 .. 255): the mean over so many samples weighted by the squared
    envelope, which keeps the value of a reflection and not of the noise between two.  Otherwise as :func:`envelope`."""
    _in_place(dat, 'frequency', smooth)


def analytic_signal(dat):
    """``x + 1j q`` on the host, complex64 for float32 data and complex128 otherwise; its real part is the data bit for
    bit.  The data are untouched."""
    q = complex_attribute(dat, 'quadrature')
    dev = getattr(dat, '_dev', None)
    x = dev.to_host() if dev is not None else np.asarray(dat.data)
    z = np.empty(q.shape, dtype=np.complex64 if q.dtype == np.float32 else np.complex128)
    z.real = x
    z.imag = q
    return z
