"""ApRES range conversion, stacking and phase difference: from raw FMCW voltages to the complex range profile that
``quadpol.py`` consumes, and to the coherence between two acquisitions.  The functions take any object with the
attributes of the reference's ``ApresData`` / ``ApresTimeDiff`` -- those objects themselves, or the :class:`Apres` and
:class:`TimeDiff` holders below -- and leave the same attributes and flags behind as NumPy arrays.  The O(n) tables
(window, ``tau``, ``Rcoarse``, ``phiref``, the reference phasor, the fine-range denominator, the crop) are NumPy
here, by the reference's own expressions in its order; everything that touches a (chirps, samples) array runs in
``csrc/apres.hip`` through the C ABI, on host buffers or, in :func:`chain`, resident in HBM from the raw chirps to
the stacked profile.

All data is float64 / complex128, as in the reference.  ``phase_uncertainty``, ``phase_unwrap``, ``range_diff``,
``strain_rate``, ``bed_pick``, loaders and savers are not here.

Reference: ``src/impdar/lib/ApresData/_ApresDataProcessing.py:24-123`` and ``:156-222``,
``src/impdar/lib/ApresData/_TimeDiffProcessing.py:57-93``.
"""
import ctypes as C
import operator

import numpy as np

from . import _hip

_MSG_RANGE_DONE = 'The range filter has already been done on these data.'
_MSG_WINDOW = 'Window must be in: blackman, bartlett, hamming, hanning, kaiser'
_WINDOWS = ['blackman', 'bartlett', 'hamming', 'hanning', 'kaiser']


class ApresFlags(object):
    """The reference's ``ApresFlags`` defaults (``ApresFlags.py:39-45``)."""

    def __init__(self):
        self.file_read_code = None
        self.range = 0
        self.stack = 0
        self.uncertainty = False
        self.attrs = ['file_read_code', 'range', 'stack', 'uncertainty']
        self.attr_dims = [None, None, None, None]


class TimeDiffFlags(object):
    """The reference's ``TimeDiffFlags`` defaults (``ApresFlags.py:104-111``)."""

    def __init__(self):
        self.file_read_code = None
        self.phase_diff = False
        self.unwrap = False
        self.strain = np.zeros((2,))
        self.bed_pick = False
        self.attrs = ['file_read_code', 'phase_diff', 'unwrap', 'strain', 'bed_pick']
        self.attr_dims = [None, None, None, 2, None]


class ApresHeader(object):
    """What the steps read of the reference's ``ApresHeader`` (``ApresHeader.py:35-66``), with its defaults."""

    def __init__(self):
        self.fsysclk = 1e9
        self.fs = 4e4
        self.snum = None
        self.chirp_length = None
        self.chirp_grad = None
        self.bandwidth = None
        self.fc = None
        self.er = None
        self.ci = None
        self.lambdac = None


class Apres(object):
    """Bare holder of what range conversion and stacking read and write (every attribute None until it is set)."""

    def __init__(self):
        self.snum = None
        self.cnum = None
        self.bnum = None
        self.data = None
        self.dt = None
        self.data_dtype = None
        self.spec = None
        self.Rcoarse = None
        self.Rfine = None
        self.phiref = None
        self.flags = ApresFlags()
        self.header = ApresHeader()


class TimeDiff(object):
    """Bare holder of what the phase difference reads and writes."""

    def __init__(self):
        self.snum = None
        self.data = None
        self.data2 = None
        self.dt = None
        self.range = None
        self.ds = None
        self.co = None
        self.w = None
        self.data_dtype = None
        self.flags = TimeDiffFlags()
        self.header = ApresHeader()


def _c128(a):
    return np.ascontiguousarray(a, dtype=np.complex128)


def _cdp(a):
    """double* to the (re, im) pairs of a C-contiguous complex128 array."""
    return a.ctypes.data_as(C.POINTER(C.c_double))


# ------------------------------------------------------------------------------------------------ host tables
def phase2range(dat, phi, lambdac=None, rc=None, K=None, ci=None):
    """Phase to range for an FMCW radar (reference :156-188): first order without ``K``, ``ci`` or ``rc``."""
    if lambdac is None:
        lambdac = dat.header.lambdac
    if not all([K, ci]) or rc is None:
        r = lambdac * phi / (4. * np.pi)
    else:
        r = phi / ((4. * np.pi / lambdac) - (4. * rc * K / ci**2.))
    return r


def window(winfun, snum):
    """NumPy's own window of ``snum`` points; the reference's errors for a name it does not know and for 'kaiser'."""
    if winfun not in _WINDOWS:
        raise TypeError(_MSG_WINDOW)
    elif winfun == 'blackman':
        win = np.blackman(snum)
    elif winfun == 'bartlett':
        win = np.bartlett(snum)
    elif winfun == 'hamming':
        win = np.hamming(snum)
    elif winfun == 'hanning':
        win = np.hanning(snum)
    elif winfun == 'kaiser':
        win = np.kaiser(snum)          # (no beta: a TypeError, as in the reference)
    return win


class RangeTables(object):
    """Everything of a range conversion that does not depend on the chirps."""


def range_tables(dat, p, max_range=4000, winfun='blackman'):
    """The reference's tables (:55-82, :98-103, :111-116) in its order: ``nf``, ``win``, ``tau``, ``Rcoarse``,
    ``phiref``, ``comp = exp(-1j phiref)``, the two scale factors, ``den`` and ``first_order`` of
    :func:`phase2range` and the number ``n`` of bins within ``max_range``."""
    if dat.flags.range != 0:
        raise TypeError(_MSG_RANGE_DONE)
    t = RangeTables()
    t.p, t.snum = p, int(dat.snum)
    t.nf = int(np.floor(p * dat.snum / 2))
    t.win = window(winfun, dat.snum)
    t.tau = np.arange(t.nf) / (dat.header.bandwidth * p)
    t.Rcoarse = t.tau * dat.header.ci / 2.
    t.phiref = 2. * np.pi * dat.header.fc * t.tau - (dat.header.chirp_grad * t.tau**2.) / 2
    t.scale_mul = np.sqrt(2. * p) / dat.snum
    t.scale_div = np.sqrt(np.mean(t.win**2.))
    t.comp = np.exp(-1j * (t.phiref))
    t.lambdac = dat.header.lambdac
    K, ci = dat.header.chirp_grad, dat.header.ci
    t.first_order = not all([K, ci])
    if t.first_order:
        t.den = np.full(t.nf, 4. * np.pi)
    else:
        t.den = (4. * np.pi / t.lambdac) - (4. * t.Rcoarse * K / ci**2.)
    t.n = int(np.argmin(t.Rcoarse <= max_range)) if t.nf else 0
    t.max_range = max_range
    return t


def raw_rows(dat):
    """The chirps as a C-contiguous (bnum cnum, snum) float64 array (any real dtype widened, as ``chirp -
    np.mean(chirp)`` would)."""
    data = np.asarray(dat.data)
    if np.iscomplexobj(data):
        raise TypeError('range conversion takes raw (real) chirps, got %s' % data.dtype)
    shape = (int(dat.bnum), int(dat.cnum), int(dat.snum))
    if data.shape != shape:
        raise ValueError('data is %s, not (bnum, cnum, snum) = %s' % (data.shape, shape))
    return np.ascontiguousarray(data, dtype=np.float64).reshape(shape[0] * shape[1], shape[2])


def _range_args(t, chunk):
    keep = (_hip.as_dp(t.win)[0], _c128(t.comp), _hip.as_dp(t.den)[0])
    args = (int(t.p), int(t.n), _hip.as_dp(keep[0])[1], _cdp(keep[1]), _hip.as_dp(keep[2])[1], float(t.scale_mul),
            float(t.scale_div), 1 if t.first_order else 0, float(t.lambdac) if t.first_order else 0., int(chunk))
    return args, keep


def stack_plan(bnum, cnum, num_chirps):
    """``(num_chirps, groups, m, per_burst)`` of the reference's two branches (:204-220)."""
    if num_chirps == None:                                   # noqa: E711  (the reference's comparison)
        num_chirps = cnum * bnum
    num_chirps = int(num_chirps)
    if num_chirps < 1:
        raise ValueError('num_chirps = %d: nothing to stack' % num_chirps)
    if num_chirps == cnum:
        return num_chirps, bnum, cnum, True
    return num_chirps, 1, min(num_chirps, bnum * cnum), False


# ------------------------------------------------------------------------------------------------ host buffers
def range_host(raw, t, chunk=0):
    """``(spec, data, Rfine)`` of (rows, snum) float64 chirps: (rows, n), (rows, n) complex128 and (rows, nf)
    float64.  ``chunk`` chirps are transformed at a time, 0 for the library's choice."""
    rows, snum = raw.shape
    spec = np.empty((rows, t.n), dtype=np.complex128)
    data = np.empty((rows, t.n), dtype=np.complex128)
    rfine = np.empty((rows, t.nf), dtype=np.float64)
    args, keep = _range_args(t, chunk)
    rc = _hip.load().impdar_apres_range(_hip.context(), _hip.as_dp(raw)[1], rows, snum, *args, _cdp(spec), _cdp(data),
                                       _hip.as_dp(rfine)[1])
    _hip.check(rc, 'impdar_apres_range')
    return spec, data, rfine


def stack_host(data, groups, m):
    """(groups, snum) means over runs of ``m`` rows of a (rows, snum) float64 or complex128 array."""
    rows, snum = data.shape
    out = np.empty((groups, snum), dtype=data.dtype)
    if snum == 0:
        return out
    ptr = _cdp if data.dtype == np.complex128 else (lambda a: _hip.as_dp(a)[1])
    rc = _hip.load().impdar_apres_stack(_hip.context(), ptr(data), 1 if data.dtype == np.complex128 else 0, rows, snum,
                                       int(groups), int(m), ptr(out))
    _hip.check(rc, 'impdar_apres_stack')
    return out


def phase_diff_windows(length, win, step):
    """The reference's window centres (:75)."""
    return np.arange(win // 2, length - win // 2, step).astype(int)


def phase_diff_host(s1, s2, win, step):
    """Complex coherence of two complex128 vectors in every window of :func:`phase_diff_windows`."""
    s1, s2 = _c128(s1), _c128(s2)
    if s1.ndim != 1 or s1.shape != s2.shape:
        raise ValueError('the two acquisitions must be vectors of one length, got %s and %s' % (s1.shape, s2.shape))
    co = np.empty(len(phase_diff_windows(len(s1), win, step)), dtype=np.complex128)
    rc = _hip.load().impdar_apres_phase_diff(_hip.context(), _cdp(s1), _cdp(s2), len(s1), int(win), int(step), _cdp(co))
    _hip.check(rc, 'impdar_apres_phase_diff')
    return co


# ------------------------------------------------------------------------------------------------ resident
def range_dev(d_raw, t, chunk=0):
    """Three new resident arrays ``(spec, data, Rfine)`` of resident (rows, snum) float64 chirps."""
    ctx, (rows, snum) = d_raw.ctx, d_raw.shape
    out = []
    args, keep = _range_args(t, chunk)
    try:
        for shape, dtype in (((rows, t.n), np.complex128), ((rows, t.n), np.complex128), ((rows, t.nf), np.float64)):
            out.append(_hip.DeviceArray(ctx, shape, dtype))
        rc = _hip.load().impdar_apres_range_dev(ctx, d_raw.ptr, rows, snum, *args, *[d.ptr for d in out])
        _hip.check(rc, 'impdar_apres_range')
    except Exception:
        for d in out:
            d.free()
        raise
    return tuple(out)


def range_last_ms(ctx=None):
    """Device milliseconds ``(prep, transform, post)`` of the last range conversion, summed over its chunks."""
    ms = [C.c_float(), C.c_float(), C.c_float()]
    rc = _hip.load().impdar_apres_range_last_ms(ctx or _hip.context(), *[C.byref(m) for m in ms])
    _hip.check(rc, 'impdar_apres_range_last_ms')
    return tuple(m.value for m in ms)


def stack_dev(d_data, groups, m):
    """New resident (groups, snum) means over runs of ``m`` rows of a resident (rows, snum) array."""
    rows, snum = d_data.shape
    with _hip.new_device_array(d_data.ctx, (groups, snum), d_data.dtype) as d_out:
        if snum:
            rc = _hip.load().impdar_apres_stack_dev(d_data.ctx, d_data.ptr, 1 if d_data.dtype == np.complex128 else 0, rows,
                                                   snum, int(groups), int(m), d_out.ptr)
            _hip.check(rc, 'impdar_apres_stack')
    return d_out


def phase_diff_dev(d_s1, d_s2, win, step):
    """New resident coherence vector of two resident complex128 vectors."""
    length = d_s1.shape[0]
    nwin = len(phase_diff_windows(length, win, step))
    with _hip.new_device_array(d_s1.ctx, (nwin,), np.complex128) as d_co:
        rc = _hip.load().impdar_apres_phase_diff_dev(d_s1.ctx, d_s1.ptr, d_s2.ptr, length, int(win), int(step), d_co.ptr)
        _hip.check(rc, 'impdar_apres_phase_diff')
    return d_co


def _to_host(d):
    return d.to_host() if d.nbytes else np.empty(d.shape, dtype=d.dtype)


# ------------------------------------------------------------------------------------------------ bookkeeping
def _set_range(dat, t, spec, data, rfine):
    bnum, cnum = int(dat.bnum), int(dat.cnum)
    dat.phiref = t.phiref
    dat.data = data.reshape(bnum, cnum, t.n)
    dat.spec = spec.reshape(bnum, cnum, t.n)
    dat.data_dtype = dat.data.dtype
    # the reference crops Rfine on its first axis (:118): bursts, not range bins
    dat.Rfine = rfine.reshape(bnum, cnum, t.nf)[:t.n]
    dat.Rcoarse = t.Rcoarse[:t.n]
    dat.snum = t.n
    dat.flags.range = t.max_range


def _stack_rows(dat):
    data = np.asarray(dat.data)
    dtype = np.complex128 if np.iscomplexobj(data) else np.float64
    shape = (int(dat.bnum), int(dat.cnum), int(dat.snum))
    if data.shape != shape:
        raise ValueError('data is %s, not (bnum, cnum, snum) = %s' % (data.shape, shape))
    return np.ascontiguousarray(data, dtype=dtype).reshape(shape[0] * shape[1], shape[2])


def _set_stack(dat, mean, num_chirps, per_burst):
    if per_burst:
        dat.data = mean.reshape(int(dat.bnum), 1, mean.shape[1])
        dat.cnum = 1
    else:
        dat.data = mean.reshape(1, 1, mean.shape[1])
        dat.bnum = 1
        dat.cnum = 1
    dat.flags.stack = num_chirps


# ------------------------------------------------------------------------------------------------ the steps
def apres_range(dat, p, max_range=4000, winfun='blackman'):
    """Range conversion (reference :24-123): leaves ``data``, ``spec``, ``Rcoarse``, ``Rfine``, ``phiref``, ``snum``,
    ``data_dtype`` and ``flags.range``."""
    t = range_tables(dat, p, max_range, winfun)
    _set_range(dat, t, *range_host(raw_rows(dat), t))


def stacking(dat, num_chirps=None):
    """Mean over chirps, per burst when ``num_chirps == cnum``, else over the first ``num_chirps`` chirps of all
    bursts in turn (reference :191-222): leaves ``data``, ``cnum``, ``bnum`` and ``flags.stack``."""
    num_chirps, groups, m, per_burst = stack_plan(int(dat.bnum), int(dat.cnum), num_chirps)
    _set_stack(dat, stack_host(_stack_rows(dat), groups, m), num_chirps, per_burst)


def phase_diff(diff, win, step, range_ext=None):
    """Coherence of two acquisitions in a moving window (reference :57-93): leaves ``ds``, ``co`` and
    ``flags.phase_diff``."""
    win, step = operator.index(win), operator.index(step)
    idxs = phase_diff_windows(len(diff.data), win, step)
    if range_ext is not None:
        ds = range_ext[idxs]
    else:
        ds = diff.range[idxs]
    co = phase_diff_host(diff.data, diff.data2, win, step)
    diff.ds = ds
    diff.co = co.reshape(np.shape(ds))
    diff.flags.phase_diff = np.array([win, step])


def chain(dat, p, max_range=4000, winfun='blackman', num_chirps=None):
    """Range conversion then stacking with the converted data resident in HBM in between: the raw chirps go up once.
    Leaves what the two calls leave, bit for bit."""
    t = range_tables(dat, p, max_range, winfun)
    raw = raw_rows(dat)
    ctx = _hip.context()
    held = []
    try:
        held.append(_hip.DeviceArray.from_host(ctx, raw))
        products = range_dev(held[0], t)
        held.extend(products)
        _set_range(dat, t, *[_to_host(d) for d in products])
        num_chirps, groups, m, per_burst = stack_plan(int(dat.bnum), int(dat.cnum), num_chirps)
        d_mean = stack_dev(products[1], groups, m)
        held.append(d_mean)
        _set_stack(dat, _to_host(d_mean), num_chirps, per_burst)
    finally:
        for d in held:
            d.free()
