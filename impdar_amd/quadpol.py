"""Quad-polarised ApRES processing: the rotation of the scattering matrix through a set of azimuths, the hhvv
coherence image, its phase gradient along range, the cross-polarised extinction (cpe) axis and the fabric strength
along it.  The functions take any object with the attributes of the
reference's ``ApresQuadPol`` -- that object itself, or the :class:`QuadPol` holder below -- and leave the same
attributes and flags behind as NumPy arrays.  The O(n) and O(n_thetas) tables (azimuths and their cos^2, sin cos,
sin^2, window sizes, gradient coefficients, filter design) are NumPy / SciPy here; everything that touches an
(n, n_thetas) image runs in ``csrc/quadpol.hip`` through the C ABI, on host buffers or, in :func:`chain` and
:func:`quadpol_processing`, resident in HBM from the four measured vectors to the last product.  What is left on
the host is O(n): ``cpe = thetas[cpe_idxs]``, the product of :func:`phase_gradient_to_fabric`, and the column roll of
:func:`azimuthal_rotation`.

All data is complex128, as in the reference.  Loaders and containers are not here.

Reference: ``src/impdar/lib/ApresData/_QuadPolProcessing.py:37-389`` and the ``quadpol_processing`` flow of
``src/impdar/bin/apdar.py:357-363``; the native hook is
``src/impdar/lib/ApresData/coherence.h:13`` with its wrapper ``_coherence.pyx``.
"""
import ctypes as C

import numpy as np

from . import _hip
from .lib.ImpdarError import ImpdarError
from .lib.migrationlib.mig_hip import gradient_coefficients

# the reference's messages, continuation lines and all
_MSG_ROTATE_FIRST = 'Rotate the quad-pol acquisition before \
                          calling this function.'
_MSG_COHERENCE_FIRST = 'Calculate coherence before calling this function.'
_MSG_CROSS_POL = 'Cross-polarized terms are of the opposite sign, check and update.'
_MSG_FILTER = 'Filter: %s has \
                            not been implemented yet.'
_MSG_FABRIC = "Get the phase gradient along CPE axis \
                             before calling this function."


class QuadPolFlags(object):
    """The reference's ``QuadPolFlags`` defaults (``ApresFlags.py:153-170``)."""

    def __init__(self):
        self.rotation = np.zeros((2,))
        self.coherence = np.zeros((3,))
        self.phasegradient = False
        self.cpe = True
        self.attrs = ['rotation', 'coherence', 'phasegradient', 'cpe']
        self.attr_dims = [2, 3, None, None]


class QuadPol(object):
    """Bare holder of what the three steps read and write (every attribute None until it is set)."""

    def __init__(self):
        self.snum = None
        self.dt = None
        self.range = None
        self.shh = None
        self.shv = None
        self.svh = None
        self.svv = None
        self.thetas = None
        self.HH = None
        self.HV = None
        self.VH = None
        self.VV = None
        self.chhvv = None
        self.dphi_dz = None
        self.flags = QuadPolFlags()


def _c128(a):
    return np.ascontiguousarray(a, dtype=np.complex128)


def _cdp(a):
    """double* to the (re, im) pairs of a C-contiguous complex128 array."""
    return a.ctypes.data_as(C.POINTER(C.c_double))


# ------------------------------------------------------------------------------------------------ host tables
def rotation_tables(qp, theta_start, theta_end, n_thetas, cross_pol_exception, cross_pol_flip, flip_force):
    """The reference's sign check of the cross-polarised terms (:64-78, flipping ``qp.shv`` or ``qp.svh`` in place
    where it asks for that), then ``(vectors, thetas, cos2, sincos, sin2)``: the four measured vectors as
    complex128 and the float64 factors of every azimuth, formed as NumPy forms them."""
    if abs(np.sum(np.imag(qp.shv) + np.imag(qp.svh))) < abs(np.sum(np.imag(qp.shv) - np.imag(qp.svh))) or \
            abs(np.sum(np.real(qp.shv) + np.real(qp.svh))) < abs(np.sum(np.real(qp.shv) - np.real(qp.svh))) or \
            flip_force:
        if cross_pol_exception:
            pass
        elif cross_pol_flip == 'HV':
            qp.shv *= -1.
        elif cross_pol_flip == 'VH':
            qp.svh *= -1.
        else:
            raise ValueError(_MSG_CROSS_POL)
    thetas = np.linspace(theta_start, theta_end, n_thetas)
    n = len(qp.range)
    vectors = [_c128(v) for v in (qp.shh, qp.shv, qp.svh, qp.svv)]
    for v in vectors:
        if v.shape != (n,):
            raise ValueError('could not broadcast input array from shape %s into shape (%d,)' % (v.shape, n))
    if n < 1 or len(thetas) < 1:
        raise ValueError('nothing to rotate: %d range bins and %d azimuths' % (n, len(thetas)))
    cos2 = np.cos(thetas)**2.
    sincos = np.sin(thetas) * np.cos(thetas)
    sin2 = np.sin(thetas)**2
    return vectors, thetas, cos2, sincos, sin2


def coherence_windows(qp, delta_theta, delta_range):
    """``(nrange, ntheta)`` by the reference's float expressions (:124-125).  A window that is empty or wider than
    the circle is a ``ValueError`` here; the reference's slices degenerate silently."""
    if qp.flags.rotation[0] != 1:
        raise ImpdarError(_MSG_ROTATE_FIRST)
    nrange = int(delta_range // abs(qp.range[0] - qp.range[1]))
    ntheta = int(delta_theta // abs(qp.thetas[0] - qp.thetas[1]))
    n_thetas = np.shape(qp.HH)[1]
    if ntheta < 1:
        raise ValueError('delta_theta = %r gives ntheta = %d: an empty window along azimuth' % (delta_theta, ntheta))
    if ntheta > n_thetas:
        raise ValueError('delta_theta = %r gives ntheta = %d: a window wider than the %d azimuths it wraps around'
                         % (delta_theta, ntheta, n_thetas))
    if nrange < 1:
        raise ValueError('delta_range = %r gives nrange = %d: an empty window along range' % (delta_range, nrange))
    return nrange, ntheta


def lowpass_spec(Wn, fs, order=3):
    """``('iir', b, a, zi)`` of the reference's ``lowpass`` (:347), the form ``preproc.filter_dev`` takes."""
    from scipy import signal
    b, a = signal.butter(order, Wn, btype='low', fs=fs)
    zi = signal.lfilter_zi(b, a)
    return ('iir', np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(a, dtype=np.float64),
            np.ascontiguousarray(zi, dtype=np.float64))


def gradient_tables(qp, filt, Wn):
    """``(grad, spec)``: the coefficients of ``np.gradient(., qp.range, axis=0)`` and the filter, or None."""
    if qp.flags.coherence[0] != 1:
        raise ImpdarError(_MSG_COHERENCE_FIRST)
    spec = None
    if filt is not None:
        if filt == 'lowpass':
            spec = lowpass_spec(Wn, 1. / qp.dt)
        else:
            raise TypeError(_MSG_FILTER % filt)
    return gradient_coefficients(qp.range), spec


def refuse_nan_subset(chhvv):
    """The reference's ``lowpass`` filters only the rows between the leading NaN rows of column 1 and as many
    trailing ones (:340-353); that subset is not built."""
    for part in (np.real(chhvv), np.imag(chhvv)):
        nan_idx = next(k for k, value in enumerate(part[:, 1]) if ~np.isnan(value))
        if nan_idx != 0:
            raise NotImplementedError('the coherence starts with %d NaN rows: filtering the rows between the NaN '
                                      'edges is not supported by the MI355X engine' % nan_idx)


def cpe_tables(qp, Wn, rad_start, rad_end):
    """``(spec, idx_start, idx_stop)`` of the reference's ``find_cpe`` (:243-254): its error before a rotation, the
    low-pass design (SciPy's own errors for a bad ``Wn``), the window of columns nearest the two azimuths.  An empty
    window is the ``ValueError`` that ``np.argmin`` raises on an empty sequence."""
    if qp.flags.rotation[0] != 1:
        raise ImpdarError(_MSG_ROTATE_FIRST)
    spec = lowpass_spec(Wn, 1. / qp.dt)
    idx_start = int(np.argmin(abs(qp.thetas - rad_start)))
    idx_stop = int(np.argmin(abs(qp.thetas - rad_end)))
    if idx_stop <= idx_start:
        np.argmin(np.empty((0,)))
    return spec, idx_start, idx_stop


def refuse_nan_anomaly(anomaly_of_rows, n):
    """:func:`refuse_nan_subset` on the power anomaly, of which only the leading rows are formed: a row of the anomaly
    depends on that row of the image alone.  ``anomaly_of_rows(k)`` gives the first ``k`` rows as complex128."""
    k = 1
    while True:
        try:
            return refuse_nan_subset(anomaly_of_rows(k))
        except StopIteration:                                # every row so far starts with NaN: look further down
            if k >= n:
                raise
            k = min(n, 8 * k)


def _planes_to_complex(pa):
    """complex128 (n, m) of the kernels' (n, 2 m) layout: m real parts, then m imaginary parts per row."""
    m = pa.shape[1] // 2
    out = np.empty((pa.shape[0], m), dtype=np.complex128)
    out.real = pa[:, :m]
    out.imag = pa[:, m:]
    return out


def _check_idx(idx, n, m):
    idx = np.asarray(idx)
    if idx.shape != (n,):
        raise IndexError('shape mismatch: %d rows and indices of shape %s' % (n, idx.shape))
    if not np.issubdtype(idx.dtype, np.integer):
        raise IndexError('arrays used as indices must be of integer (or boolean) type')
    if n and (idx.min() < -m or idx.max() >= m):
        bad = idx[(idx < -m) | (idx >= m)][0]
        raise IndexError('index %d is out of bounds for axis 1 with size %d' % (bad, m))
    return np.ascontiguousarray(np.where(idx < 0, idx + m, idx), dtype=np.int32)


def _grad_args(grad):
    uniform, h, ga, gb, gc = grad
    return (1 if uniform else 0, float(h), _hip.as_dp(ga), _hip.as_dp(gb), _hip.as_dp(gc))


def _spec_args(spec):
    if spec is None:
        return (None, None, 0, None), ()
    _, b, a, zi = spec
    n = max(len(a), len(b))
    keep = (np.r_[b, np.zeros(n - len(b))], np.r_[a, np.zeros(n - len(a))], zi)
    return (_hip.as_dp(keep[0])[1], _hip.as_dp(keep[1])[1], n, _hip.as_dp(keep[2])[1]), keep


# ------------------------------------------------------------------------------------------------ host buffers
def rotate_host(vectors, cos2, sincos, sin2):
    """``(HH, HV, VH, VV)``, each (n, n_thetas) complex128, of four complex128 vectors."""
    n, nth = len(vectors[0]), len(cos2)
    out = [np.empty((n, nth), dtype=np.complex128) for _ in range(4)]
    rc = _hip.load().impdar_qp_rotate(_hip.context(), *[_cdp(v) for v in vectors], n, _hip.as_dp(cos2)[1],
                                     _hip.as_dp(sincos)[1], _hip.as_dp(sin2)[1], nth, *[_cdp(o) for o in out])
    _hip.check(rc, 'impdar_qp_rotate')
    return tuple(out)


def coherence_host(HH, VV, nrange, ntheta, wrap=True):
    """hhvv coherence of two (n, ncols) images: (n, ncols) with periodic columns, (n, ncols - 2 ntheta) of a
    padded pair with ``wrap=False``."""
    HH, VV = _c128(HH), _c128(VV)
    if HH.ndim != 2 or HH.shape != VV.shape:
        raise ValueError('HH and VV must be two (range_bins, azimuth_bins) arrays of one shape')
    n, ncols = HH.shape
    out = np.empty((n, ncols if wrap else max(ncols - 2 * ntheta, 0)), dtype=np.complex128)
    rc = _hip.load().impdar_qp_coherence(_hip.context(), _cdp(HH), _cdp(VV), n, ncols, int(nrange), int(ntheta),
                                        1 if wrap else 0, _cdp(out))
    _hip.check(rc, 'impdar_qp_coherence')
    return out


def phase_gradient_host(chhvv, grad, spec=None):
    """(n, m) float64 phase gradient of an (n, m) coherence image."""
    chhvv = _c128(chhvv)
    n, m = chhvv.shape
    out = np.empty((n, m), dtype=np.float64)
    uniform, h, ga, gb, gc = _grad_args(grad)
    filt, keep = _spec_args(spec)
    rc = _hip.load().impdar_qp_phase_gradient(_hip.context(), _cdp(chhvv), n, m, uniform, h, ga[1], gb[1], gc[1], *filt,
                                             _hip.as_dp(out)[1])
    _hip.check(rc, 'impdar_qp_phase_gradient')
    return out


def anomaly_host(HV):
    """Power anomaly of an (n, m) complex128 image in the kernels' (n, 2 m) float64 layout."""
    HV = _c128(HV)
    if HV.ndim != 2:
        raise ValueError('the image must be a (range_bins, azimuth_bins) array')
    n, m = HV.shape
    pa = np.empty((n, 2 * m), dtype=np.float64)
    rc = _hip.load().impdar_qp_power_anomaly(_hip.context(), _cdp(HV), n, m, _hip.as_dp(pa)[1])
    _hip.check(rc, 'impdar_qp_power_anomaly')
    return pa


def find_cpe_host(HV, spec, idx_start, idx_stop, filtered=False):
    """int32 column of the least low-passed power anomaly in ``[idx_start, idx_stop)`` per row of an (n, m)
    complex128 image; with ``filtered`` also that anomaly, (n, 2 m) float64."""
    HV = _c128(HV)
    n, m = HV.shape
    idxs = np.empty((n,), dtype=np.int32)
    pa = np.empty((n, 2 * m), dtype=np.float64) if filtered else None
    filt, keep = _spec_args(spec)
    rc = _hip.load().impdar_qp_find_cpe(_hip.context(), _cdp(HV), n, m, *filt, int(idx_start), int(idx_stop),
                                       idxs.ctypes.data_as(C.POINTER(C.c_int)), _hip.as_dp(pa)[1])
    _hip.check(rc, 'impdar_qp_find_cpe')
    return (idxs, pa) if filtered else idxs


def cpe_gather_host(image, idx):
    """``image[np.arange(n), idx]`` of an (n, m) complex128 or float64 image."""
    image = np.asarray(image)
    is_complex = np.iscomplexobj(image)
    image = np.ascontiguousarray(image, dtype=np.complex128 if is_complex else np.float64)
    n, m = image.shape
    idx = _check_idx(idx, n, m)
    out = np.empty((n,), dtype=image.dtype)
    ptr = _cdp if is_complex else (lambda a: _hip.as_dp(a)[1])
    rc = _hip.load().impdar_qp_cpe_gather(_hip.context(), ptr(image), 1 if is_complex else 0, n, m,
                                         idx.ctypes.data_as(C.POINTER(C.c_int)), ptr(out))
    _hip.check(rc, 'impdar_qp_cpe_gather')
    return out


# ------------------------------------------------------------------------------------------------ resident
def rotate_dev(d_vectors, cos2, sincos, sin2):
    """Four new resident (n, n_thetas) complex128 arrays from four resident complex128 vectors."""
    ctx, n, nth = d_vectors[0].ctx, d_vectors[0].shape[0], len(cos2)
    out = []
    try:
        for _ in range(4):
            out.append(_hip.DeviceArray(ctx, (n, nth), np.complex128))
        rc = _hip.load().impdar_qp_rotate_dev(ctx, *[d.ptr for d in d_vectors], n, _hip.as_dp(cos2)[1], _hip.as_dp(sincos)[1],
                                             _hip.as_dp(sin2)[1], nth, *[d.ptr for d in out])
        _hip.check(rc, 'impdar_qp_rotate')
    except Exception:
        for d in out:
            d.free()
        raise
    return tuple(out)


def coherence_dev(d_HH, d_VV, nrange, ntheta, wrap=True):
    """New resident coherence image of two resident (n, ncols) images."""
    n, ncols = d_HH.shape
    with _hip.new_device_array(d_HH.ctx, (n, ncols if wrap else max(ncols - 2 * ntheta, 0)), np.complex128) as d_out:
        rc = _hip.load().impdar_qp_coherence_dev(d_HH.ctx, d_HH.ptr, d_VV.ptr, n, ncols, int(nrange), int(ntheta),
                                                1 if wrap else 0, d_out.ptr)
        _hip.check(rc, 'impdar_qp_coherence')
    return d_out


def phase_gradient_dev(d_chhvv, grad, spec=None):
    """New resident (n, m) float64 phase gradient of a resident coherence image."""
    n, m = d_chhvv.shape
    uniform, h, ga, gb, gc = _grad_args(grad)
    filt, keep = _spec_args(spec)
    with _hip.new_device_array(d_chhvv.ctx, (n, m), np.float64) as d_out:
        rc = _hip.load().impdar_qp_phase_gradient_dev(d_chhvv.ctx, d_chhvv.ptr, n, m, uniform, h, ga[1], gb[1], gc[1], *filt,
                                                     d_out.ptr)
        _hip.check(rc, 'impdar_qp_phase_gradient')
    return d_out


def anomaly_dev(d_HV, rows=None):
    """New resident (rows, 2 m) float64 power anomaly of the first ``rows`` rows (all of them by default) of a
    resident (n, m) complex128 image."""
    n, m = d_HV.shape
    rows = n if rows is None else int(rows)
    with _hip.new_device_array(d_HV.ctx, (rows, 2 * m), np.float64) as d_pa:
        rc = _hip.load().impdar_qp_power_anomaly_dev(d_HV.ctx, d_HV.ptr, rows, m, d_pa.ptr)
        _hip.check(rc, 'impdar_qp_power_anomaly')
    return d_pa


def find_cpe_dev(d_HV, spec, idx_start, idx_stop, filtered=False):
    """New resident int32 indices of a resident (n, m) complex128 image; with ``filtered`` also the resident
    (n, 2 m) float64 low-passed anomaly."""
    n, m = d_HV.shape
    filt, keep = _spec_args(spec)
    out = []
    try:
        out.append(_hip.DeviceArray(d_HV.ctx, (n,), np.int32))
        if filtered:
            out.append(_hip.DeviceArray(d_HV.ctx, (n, 2 * m), np.float64))
        rc = _hip.load().impdar_qp_find_cpe_dev(d_HV.ctx, d_HV.ptr, n, m, *filt, int(idx_start), int(idx_stop), out[0].ptr,
                                               out[1].ptr if filtered else None)
        _hip.check(rc, 'impdar_qp_find_cpe')
    except Exception:
        for d in out:
            d.free()
        raise
    return tuple(out) if filtered else out[0]


def find_cpe_last_ms(ctx=None):
    """Device milliseconds ``(anomaly, filter, argmin)`` of the last ``find_cpe``."""
    ms = [C.c_float(), C.c_float(), C.c_float()]
    rc = _hip.load().impdar_qp_find_cpe_last_ms(ctx or _hip.context(), *[C.byref(m) for m in ms])
    _hip.check(rc, 'impdar_qp_find_cpe_last_ms')
    return tuple(m.value for m in ms)


def cpe_gather_dev(d_image, d_idx):
    """New resident ``image[np.arange(n), idx]`` of a resident (n, m) image and resident int32 indices."""
    n, m = d_image.shape
    with _hip.new_device_array(d_image.ctx, (n,), d_image.dtype) as d_out:
        rc = _hip.load().impdar_qp_cpe_gather_dev(d_image.ctx, d_image.ptr, 1 if d_image.dtype == np.complex128 else 0, n, m,
                                                 d_idx.ptr, d_out.ptr)
        _hip.check(rc, 'impdar_qp_cpe_gather')
    return d_out


# ------------------------------------------------------------------------------------------------ bookkeeping
def _set_rotation(qp, thetas, images, n_thetas):
    qp.thetas = thetas
    qp.HH, qp.HV, qp.VH, qp.VV = images
    qp.flags.rotation = np.array([1, n_thetas])


def _set_coherence(qp, chhvv, delta_theta, delta_range):
    qp.chhvv = chhvv
    # if the cpe axis has already been identified, the coherence along it (:173-174)
    if qp.flags.cpe is True:
        qp.chhvv_cpe = qp.chhvv[np.arange(qp.snum), qp.cpe_idxs]
    qp.flags.coherence = np.array([1, delta_theta, delta_range])


def _set_gradient(qp, dphi_dz):
    qp.dphi_dz = dphi_dz
    if qp.flags.cpe is True:
        qp.dphi_dz_cpe = qp.dphi_dz[np.arange(qp.snum), qp.cpe_idxs]
    qp.flags.phasegradient = True


def _set_cpe(qp, idxs, chhvv_cpe=None, dphi_dz_cpe=None):
    """What ``find_cpe`` leaves (:260-272).  The two gathers are taken from the host images unless the caller has
    made them already from resident ones."""
    qp.cpe_idxs = np.asarray(idxs).astype(int)
    qp.cpe = np.array([qp.thetas[i] for i in qp.cpe_idxs]).astype(float)
    if qp.flags.coherence[0] == 1.:
        qp.chhvv_cpe = qp.chhvv[np.arange(qp.snum), qp.cpe_idxs] if chhvv_cpe is None else chhvv_cpe
    if qp.flags.phasegradient:
        qp.dphi_dz_cpe = qp.dphi_dz[np.arange(qp.snum), qp.cpe_idxs] if dphi_dz_cpe is None else dphi_dz_cpe
    qp.flags.cpe = True


# ------------------------------------------------------------------------------------------------ the steps
def rotational_transform(qp, theta_start=0, theta_end=np.pi, n_thetas=100, cross_pol_exception=False,
                         cross_pol_flip=False, flip_force=False):
    """Azimuthal rotation of the scattering matrix (reference :37-101): leaves ``thetas``, ``HH``, ``HV``, ``VH``,
    ``VV`` and ``flags.rotation``."""
    vectors, thetas, cos2, sincos, sin2 = rotation_tables(qp, theta_start, theta_end, n_thetas, cross_pol_exception,
                                                          cross_pol_flip, flip_force)
    _set_rotation(qp, thetas, rotate_host(vectors, cos2, sincos, sin2), n_thetas)


def coherence2d(qp, delta_theta=20.0 * np.pi / 180., delta_range=100.):
    """hhvv coherence over a moving (range, azimuth) window, periodic in azimuth (reference :104-176): leaves
    ``chhvv`` and ``flags.coherence``."""
    nrange, ntheta = coherence_windows(qp, delta_theta, delta_range)
    _set_coherence(qp, coherence_host(qp.HH, qp.VV, nrange, ntheta, wrap=True), delta_theta, delta_range)


def phase_gradient2d(qp, filt=None, Wn=0):
    """Depth gradient of the phase of the coherence image (reference :180-222): leaves ``dphi_dz`` and
    ``flags.phasegradient``."""
    grad, spec = gradient_tables(qp, filt, Wn)
    if spec is not None:
        refuse_nan_subset(qp.chhvv)
    _set_gradient(qp, phase_gradient_host(qp.chhvv, grad, spec))


def power_anomaly(data):
    """Power anomaly from the row mean of an (n, m) image (reference :303-319): complex128, computed on the GPU."""
    return _planes_to_complex(anomaly_host(data))


def find_cpe(qp, Wn=50, rad_start=np.pi / 4., rad_end=3. * np.pi / 4.):
    """The cross-polarised extinction axis (reference :225-272): leaves ``cpe_idxs``, ``cpe``, ``flags.cpe`` and,
    where the coherence or the phase gradient is there already, ``chhvv_cpe`` / ``dphi_dz_cpe``."""
    spec, idx_start, idx_stop = cpe_tables(qp, Wn, rad_start, rad_end)
    HV = _c128(qp.HV)
    refuse_nan_anomaly(lambda k: _planes_to_complex(anomaly_host(HV[:k])), HV.shape[0])
    _set_cpe(qp, find_cpe_host(HV, spec, idx_start, idx_stop))


def phase_gradient_to_fabric(qp, c=300e6, fc=300e6, delta_eps=0.035, eps=3.12):
    """Fabric strength from the phase gradient along the cpe axis (reference :276-299): leaves ``e2e1``."""
    if not hasattr(qp, 'dphi_dz_cpe'):
        raise AttributeError(_MSG_FABRIC)
    qp.e2e1 = (c / (4. * np.pi * fc)) * (2. * np.sqrt(eps) / delta_eps) * qp.dphi_dz_cpe


def azimuthal_rotation(data, thetas, azi):
    """Roll the columns of an image to a known antenna orientation (reference :359-389); ``thetas`` is shifted and
    shifted back in place, as there."""
    thetas += azi
    if azi < 0:
        clip = np.argwhere(thetas > 0)[0][0]
        data = np.append(data[:, clip:], data[:, :clip], axis=1)
    elif azi > 0:
        clip = np.argwhere(thetas > np.pi)[0][0]
        data = np.append(data[:, clip:], data[:, :clip], axis=1)
    thetas -= azi
    return data


def chain(qp, theta_start=0, theta_end=np.pi, n_thetas=100, cross_pol_exception=False, cross_pol_flip=False,
          flip_force=False, delta_theta=20.0 * np.pi / 180., delta_range=100., filt=None, Wn=0):
    """The three steps with the images resident in HBM in between: the four vectors go up once, every product comes
    down once.  Leaves what the three calls leave, bit for bit."""
    vectors, thetas, cos2, sincos, sin2 = rotation_tables(qp, theta_start, theta_end, n_thetas, cross_pol_exception,
                                                          cross_pol_flip, flip_force)
    ctx = _hip.context()
    held = []
    try:
        for v in vectors:
            held.append(_hip.DeviceArray.from_host(ctx, v))
        images = rotate_dev(held[:4], cos2, sincos, sin2)
        held.extend(images)
        _set_rotation(qp, thetas, tuple(d.to_host() for d in images), n_thetas)
        nrange, ntheta = coherence_windows(qp, delta_theta, delta_range)
        d_chhvv = coherence_dev(images[0], images[3], nrange, ntheta, wrap=True)
        held.append(d_chhvv)
        _set_coherence(qp, d_chhvv.to_host(), delta_theta, delta_range)
        grad, spec = gradient_tables(qp, filt, Wn)
        if spec is not None:
            refuse_nan_subset(qp.chhvv)
        d_dphi = phase_gradient_dev(d_chhvv, grad, spec)
        held.append(d_dphi)
        _set_gradient(qp, d_dphi.to_host())
    finally:
        for d in held:
            d.free()


def quadpol_processing(qp, nthetas=100, dtheta=20.0 * np.pi / 180., drange=100., Wn=50, cross_pol_flip=False,
                       gradient=False, filt=None, Wn_gradient=0):
    """The reference's full flow (``apdar.py:357-363``) -- rotation, cpe axis, coherence -- and with ``gradient`` the
    phase gradient, its values along the cpe axis and the fabric strength, with every image resident in HBM in
    between: the four vectors go up once, every product comes down once.  Leaves what the separate calls leave, bit
    for bit."""
    vectors, thetas, cos2, sincos, sin2 = rotation_tables(qp, 0, np.pi, nthetas, False, cross_pol_flip, False)
    ctx = _hip.context()
    held = []
    try:
        for v in vectors:
            held.append(_hip.DeviceArray.from_host(ctx, v))
        images = rotate_dev(held[:4], cos2, sincos, sin2)
        held.extend(images)
        _set_rotation(qp, thetas, tuple(d.to_host() for d in images), nthetas)
        # the cpe axis of the resident HV
        spec, idx_start, idx_stop = cpe_tables(qp, Wn, np.pi / 4., 3. * np.pi / 4.)

        def lead(k):
            d_pa = anomaly_dev(images[1], k)
            try:
                return _planes_to_complex(d_pa.to_host())
            finally:
                d_pa.free()
        refuse_nan_anomaly(lead, images[1].shape[0])
        d_idx = find_cpe_dev(images[1], spec, idx_start, idx_stop)
        held.append(d_idx)
        # (a coherence or a gradient left by an earlier call is gathered from its host image, as find_cpe does)
        _set_cpe(qp, d_idx.to_host())
        nrange, ntheta = coherence_windows(qp, dtheta, drange)
        d_chhvv = coherence_dev(images[0], images[3], nrange, ntheta, wrap=True)
        held.append(d_chhvv)
        held.append(cpe_gather_dev(d_chhvv, d_idx))
        qp.chhvv = d_chhvv.to_host()
        qp.chhvv_cpe = held[-1].to_host()
        qp.flags.coherence = np.array([1, dtheta, drange])
        if gradient:
            grad, gspec = gradient_tables(qp, filt, Wn_gradient)
            if gspec is not None:
                refuse_nan_subset(qp.chhvv)
            d_dphi = phase_gradient_dev(d_chhvv, grad, gspec)
            held.append(d_dphi)
            held.append(cpe_gather_dev(d_dphi, d_idx))
            qp.dphi_dz = d_dphi.to_host()
            qp.dphi_dz_cpe = held[-1].to_host()
            qp.flags.phasegradient = True
            phase_gradient_to_fabric(qp)
    finally:
        for d in held:
            d.free()


# ------------------------------------------------------------------------------------------------ native hook
def coherence2d_loop(chhvv, HH, VV, nrange, ntheta, range_bins, azimuth_bins):
    """The reference's Cython wrapper (``_coherence.pyx:23-40``) over this library's ``coherence2d`` symbol: the
    padded images of ``_QuadPolProcessing.py:127-136`` in, columns ``ntheta ... azimuth_bins - ntheta - 1`` of
    ``chhvv`` written in place, ``chhvv.copy()`` returned.  Anything but 2-D C-contiguous complex128 is refused, as
    the wrapper's typed arguments refuse it."""
    for name, a in (('chhvv', chhvv), ('HH', HH), ('VV', VV)):
        if not isinstance(a, np.ndarray):
            raise TypeError("Argument '%s' has incorrect type (expected numpy.ndarray, got %s)" % (name, type(a).__name__))
        if a.dtype != np.complex128:
            raise ValueError("Buffer dtype mismatch, expected 'double complex' but got %s for '%s'" % (a.dtype, name))
        if a.ndim != 2:
            raise ValueError('Buffer has wrong number of dimensions (expected 2, got %d)' % a.ndim)
        if not a.flags.c_contiguous:
            raise ValueError('ndarray is not C-contiguous')
        if a.size < int(range_bins) * int(azimuth_bins):
            raise ValueError("'%s' holds %d values, fewer than range_bins x azimuth_bins = %d x %d"
                             % (name, a.size, range_bins, azimuth_bins))
    _hip.load().coherence2d(_cdp(chhvv), _cdp(HH), _cdp(VV), int(nrange), int(ntheta), int(range_bins), int(azimuth_bins))
    return chhvv.copy()
