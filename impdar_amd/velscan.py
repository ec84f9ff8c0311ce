"""Stolt velocity scan: how well does the f-k migration focus at each of a batch of velocities?

``stolt_velocity_scan(dat, vels)`` migrates ``dat`` with ``migrationStolt`` at every velocity of ``vels`` without
touching ``dat``: the taper and the forward transforms run once on the GPU, the stretch and the inverse transforms in
batches of velocities, and no image leaves the device -- each is reduced there to three sums per output row,
``sum |x|``, ``sum x^2`` and ``sum x^4`` over a window of traces (``csrc/stolt.hip``: ``impdar_stolt_scan``).  The
:class:`VelocityScan` that comes back turns them into the varimax ``n sum x^4 / (sum x^2)^2`` of any range of samples or
of depth gates; a diffraction collapses, and the varimax peaks, at the velocity of the medium.

``scan_host`` and ``scan_dev`` are the only functions here that reach the library.
"""
import ctypes as C

import numpy as np

from . import _hip


def scan_host(data, kx, ws, vels, htaper, vtaper, t0, t1, keep=-1, max_batch=0):
    """``impdar_stolt_scan`` on a host array (float32 / float64, (snum, tnum)): ``(sums, image)`` with ``sums`` of
    shape ``(nv, 2 * (snum // 2), 3)`` float64 and ``image`` the Stolt image of ``vels[keep]`` (None for keep < 0)."""
    data = np.ascontiguousarray(data)
    snum, tnum = data.shape
    nout = 2 * (snum // 2)
    vels = np.ascontiguousarray(vels, dtype=np.float64)
    sums = np.empty((len(vels), nout, 3), dtype=np.float64)
    image = np.empty((nout, tnum), dtype=data.dtype) if keep >= 0 else None
    rc = _hip.load().impdar_stolt_scan(_hip.context(), data.ctypes.data_as(C.c_void_p), _hip.dtype_code(data.dtype), snum, tnum,
                                       _hip.as_dp(kx)[1], _hip.as_dp(ws)[1], _hip.as_dp(vels)[1], len(vels), float(htaper),
                                       float(vtaper), int(t0), int(t1), int(max_batch), _hip.as_dp(sums)[1], int(keep),
                                       image.ctypes.data_as(C.c_void_p) if image is not None else None)
    _hip.check(rc, 'impdar_stolt_scan')
    return sums, image


def scan_dev(dev, kx, ws, vels, htaper, vtaper, t0, t1, keep=-1, max_batch=0):
    """``impdar_stolt_scan_dev`` on a resident :class:`_hip.DeviceArray`; the kept image is a new ``DeviceArray``."""
    snum, tnum = dev.shape
    nout = 2 * (snum // 2)
    vels = np.ascontiguousarray(vels, dtype=np.float64)
    sums = np.empty((len(vels), nout, 3), dtype=np.float64)
    image = _hip.DeviceArray(dev.ctx, (nout, tnum), dev.dtype) if keep >= 0 else None
    rc = _hip.load().impdar_stolt_scan_dev(dev.ctx, dev.ptr, _hip.dtype_code(dev.dtype), snum, tnum, _hip.as_dp(kx)[1],
                                           _hip.as_dp(ws)[1], _hip.as_dp(vels)[1], len(vels), float(htaper), float(vtaper),
                                           int(t0), int(t1), int(max_batch), _hip.as_dp(sums)[1], int(keep),
                                           image.ptr if image is not None else None)
    if rc and image is not None:
        image.free()
    _hip.check(rc, 'impdar_stolt_scan')
    return sums, image


class VelocityScan(object):
    """Focus sums of a Stolt velocity scan.

    ``vels`` (nv,); ``l1``, ``l2``, ``l4`` (nv, nout) float64: per velocity and output row, the sums of ``|x|``,
    ``x^2`` and ``x^4`` over the traces ``traces = (t0, t1)``; ``image``: the migrated image of the velocity asked for
    with ``keep`` (a host array, or a ``DeviceArray`` when the radargram was resident), else None."""

    def __init__(self, vels, sums, traces, image=None):
        self.vels = np.array(vels, dtype=np.float64)
        sums = np.asarray(sums, dtype=np.float64)
        self.l1 = np.ascontiguousarray(sums[:, :, 0])
        self.l2 = np.ascontiguousarray(sums[:, :, 1])
        self.l4 = np.ascontiguousarray(sums[:, :, 2])
        self.traces = (int(traces[0]), int(traces[1]))
        self.image = image

    def _regions(self, samples, gates):
        nout = self.l2.shape[1]
        s0, s1 = (0, nout) if samples is None else (int(samples[0]), int(samples[1]))
        if not 0 <= s0 < s1 <= nout:
            raise ValueError('samples must satisfy 0 <= s0 < s1 <= %d, got (%d, %d)' % (nout, s0, s1))
        rows = np.arange(s0, s1)
        if gates is None:
            return [rows], False
        if int(gates) < 1 or int(gates) > len(rows):
            raise ValueError('gates must be between 1 and the number of samples, got %r' % (gates,))
        return np.array_split(rows, int(gates)), True

    def varimax(self, samples=None, gates=None):
        """``n sum x^4 / (sum x^2)^2`` over the rows ``samples = (s0, s1)`` (default: all) and the scan's traces, n the
        number of samples of the region: ``(nv,)``, or ``(nv, gates)`` with the sample range split into ``gates`` parts as
        ``numpy.array_split`` splits it.  The rows' sums are added in index order; a region without energy gives NaN."""
        regions, gated = self._regions(samples, gates)
        width = self.traces[1] - self.traces[0]
        out = np.empty((len(self.vels), len(regions)), dtype=np.float64)
        for g, rows in enumerate(regions):
            e2 = np.zeros(len(self.vels))
            e4 = np.zeros(len(self.vels))
            for k in rows:                                  # (index order: the same bits whatever NumPy's pairwise blocking)
                e2 = e2 + self.l2[:, k]
                e4 = e4 + self.l4[:, k]
            n = float(len(rows) * width)
            with np.errstate(divide='ignore', invalid='ignore'):
                v = n * e4 / (e2 * e2)
            v[e2 == 0] = np.nan
            out[:, g] = v
        return out if gated else out[:, 0]

    def best(self, samples=None, gates=None):
        """``(index, velocity)`` of the largest varimax (arrays of length ``gates`` with gates); NaNs are skipped, a
        region with nothing else raises ``ValueError('no finite focus value')``."""
        v = self.varimax(samples=samples, gates=gates)
        cols = v if v.ndim == 2 else v[:, None]
        if not np.isfinite(cols).any(axis=0).all():
            raise ValueError('no finite focus value')
        cols = np.where(np.isfinite(cols), cols, np.nan)
        idx = np.nanargmax(cols, axis=0)
        if v.ndim == 2:
            return idx, self.vels[idx]
        return int(idx[0]), float(self.vels[idx[0]])


def check_vels(vels):
    vels = np.asarray(vels, dtype=np.float64)
    if vels.ndim != 1:
        raise ValueError('vels must be a 1-D sequence of velocities')
    if vels.size == 0:
        raise ValueError('vels is empty')
    if not np.all(np.isfinite(vels)) or np.any(vels <= 0):
        raise ValueError('every velocity must be finite and greater than 0')
    return np.ascontiguousarray(vels)


def stolt_velocity_scan(dat, vels, htaper=100, vtaper=1000, traces=None, keep=None, max_batch=0):
    """Scan ``migrationStolt(dat, vel=v, htaper, vtaper)`` over ``vels`` and return a :class:`VelocityScan`.

    ``dat`` (a host radargram or one held on the device with ``to_device()``) is left as it is.  ``traces = (t0, t1)``
    is the window of traces the sums run over (default: all); ``keep`` the index into ``vels`` of an image to hand back
    as ``scan.image`` (on the device for a resident radargram).  Integer data is tapered and truncated on the host as
    ``migrationStolt`` does.  ``max_batch`` caps the velocities per batch (0: as many as fit the library's budget)."""
    from .lib.migrationlib.mig_hip import _check_data_shape, _device_data, _kx
    vels = check_vels(vels)
    dev = getattr(dat, '_dev', None)
    if dev is None:
        _check_data_shape(dat)
    elif dev.shape != (dat.snum, dat.tnum):
        raise ValueError('The input array must be of size (snum, tnum)')
    t0, t1 = (0, dat.tnum) if traces is None else (int(traces[0]), int(traces[1]))
    if not 0 <= t0 < t1 <= dat.tnum:
        raise ValueError('traces must satisfy 0 <= t0 < t1 <= tnum, got (%d, %d)' % (t0, t1))
    if keep is None:
        keep = -1
    elif not 0 <= int(keep) < len(vels):
        raise ValueError('keep must be an index into vels, got %r' % (keep,))
    ws = 2. * np.pi * np.fft.rfftfreq(dat.snum, d=dat.dt)
    kx = _kx(dat)
    if dev is not None:
        sums, image = scan_dev(dev, kx, ws, vels, htaper, vtaper, t0, t1, int(keep), max_batch)
        return VelocityScan(vels, sums, (t0, t1), image)
    src = np.asarray(dat.data)
    ht, vt = float(htaper), float(vtaper)
    if not np.issubdtype(src.dtype, np.floating):
        # integer dtypes: the taper product is truncated to the integer type before the transform (mig_python.py:157);
        # NaN taper lengths tell the device that the taper has been applied
        it = np.arange(dat.tnum)
        ks = np.arange(dat.snum)
        hh = np.minimum(it, it[::-1]) / htaper
        vv = np.minimum(ks, ks[::-1]) / vtaper
        hh[hh > 1.] = 1.
        vv[vv > 1.] = 1.
        src = (src * hh[None, :] * vv[:, None]).astype(src.dtype)
        ht = vt = float('nan')
    data, _ = _device_data(src)
    sums, image = scan_host(data, kx, ws, vels, ht, vt, t0, t1, int(keep), max_batch)
    return VelocityScan(vels, sums, (t0, t1), image)
