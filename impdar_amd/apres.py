"""ApRES range conversion, stacking, phase uncertainty and the time-difference flow: from raw FMCW voltages to the
complex range profile that ``quadpol.py`` consumes, and from two such profiles to the vertical velocity, the strain
rate and the bed.  The functions take any object with the
attributes of the reference's ``ApresData`` / ``ApresTimeDiff`` -- those objects themselves, or the :class:`Apres` and
:class:`TimeDiff` holders below -- and leave the same attributes and flags behind as NumPy arrays.  The O(n) tables
(window, ``tau``, ``Rcoarse``, ``phiref``, the reference phasor, the fine-range denominator, the crop) are NumPy
here, by the reference's own expressions in its order; everything that touches a (chirps, samples) array runs in
``csrc/apres.hip`` through the C ABI, on host buffers or, in :func:`chain`, resident in HBM from the raw chirps to
the stacked profile.  What follows the phase difference -- :func:`phase_unwrap`, :func:`range_diff`,
:func:`strain_rate`, :func:`bed_pick` -- and :func:`phase_uncertainty` work on vectors of a few hundred to a few
thousand elements: they are NumPy / SciPy on the host, the reference's expressions in its order, with its messages,
exception types and quirks.  :func:`single_processing` and :func:`time_diff_processing` are the reference's two
full flows.

All data is float64 / complex128, as in the reference.  Loaders and savers are not here: they are
``impdar_amd/lib/ApresData``, whose raw acquisitions keep the instrument's counts so that :func:`chain` can upload
those (:func:`decode_dev`) instead of float64 chirps.

Reference: ``src/impdar/lib/ApresData/_ApresDataProcessing.py:24-222``,
``src/impdar/lib/ApresData/_TimeDiffProcessing.py:57-247``, ``src/impdar/bin/apdar.py:337-354``.
"""
import ctypes as C
import operator

import numpy as np

from . import _hip

_MSG_RANGE_DONE = 'The range filter has already been done on these data.'
_MSG_WINDOW = 'Window must be in: blackman, bartlett, hamming, hanning, kaiser'
_WINDOWS = ['blackman', 'bartlett', 'hamming', 'hanning', 'kaiser']
_MSG_RANGE_FIRST = ('The range filter has not been executed on this data class, do that before the uncertainty '
                    'calculation.')
_MSG_DIFF_FIRST = 'Need to do the phase difference calculation first.'
_MSG_UNWRAP_FIRST = 'Should unwrap the phase profile before converting to range'
_MSG_RANGE_DIFF_FIRST = "Get the vertical velocity profile first with 'range_diff()'."
_MSG_BED_APART = 'Bed pick from first and second acquisitions are too far apart.'
_MSG_BED_COHERENCE = 'Bed pick has too low coherence.'


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
        self.uncertainty = None
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
        self.unc1 = None
        self.unc2 = None
        self.phi = None
        self.w_err = None
        self.eps_zz = None
        self.w0 = None
        self.bed = None
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


# ------------------------------------------------------------------------------------------------ counts to volts
_COUNT_KINDS = {np.dtype('<u2'): 0, np.dtype('<u4'): 1}


def _counts(counts):
    """``(flat C-contiguous array, kind)`` of an instrument's counts: little-endian uint16 or uint32."""
    counts = np.asarray(counts)
    if counts.dtype not in _COUNT_KINDS:
        raise TypeError('counts are little-endian uint16 or uint32, got %s' % counts.dtype)
    return np.ascontiguousarray(counts).reshape(-1), _COUNT_KINDS[counts.dtype]


def decode_host(counts, divisor=1.):
    """``counts.astype(float) * 2.5 / 2**16.`` (``/ divisor`` unless that is 1) of uint16 or uint32 counts, computed
    on the device from the counts as they are (reference ``load_apres.py:391-395``): float64 of the counts' shape,
    bit for bit NumPy's."""
    flat, kind = _counts(counts)
    out = np.empty(flat.shape, dtype=np.float64)
    rc = _hip.load().impdar_apres_decode(_hip.context(), flat.ctypes.data_as(C.c_void_p), kind, flat.size, float(divisor),
                                        _hip.as_dp(out)[1])
    _hip.check(rc, 'impdar_apres_decode')
    return out.reshape(np.shape(counts))


def decode_dev(counts, divisor=1., shape=None, ctx=None, piece=0):
    """New resident float64 array of ``shape`` (default: ``(1, counts.size)`` for flat counts, else the counts' shape
    folded to two axes) with the volts of host ``counts``: what :func:`range_dev` reads, without the float64 chirps
    ever existing on the host.  ``piece`` counts go up at a time (0: the library's choice, 8 MiB of them); the result
    does not depend on it."""
    flat, kind = _counts(counts)
    if shape is None:
        last = np.shape(counts)[-1] if np.ndim(counts) else 1
        shape = (flat.size // last if last else 0, last)
    if int(np.prod(shape)) != flat.size:
        raise ValueError('%d counts do not fill %s' % (flat.size, (shape,)))
    with _hip.new_device_array(ctx or _hip.context(), shape, np.float64) as d_out:
        rc = _hip.load().impdar_apres_decode_pieces_dev(d_out.ctx, flat.ctypes.data_as(C.c_void_p), kind, flat.size,
                                                       float(divisor), d_out.ptr, int(piece))
        _hip.check(rc, 'impdar_apres_decode')
    return d_out


def raw_counts(dat):
    """``(counts, divisor)`` of an acquisition that still holds the instrument's counts in place of float64 chirps
    (``lib.ApresData.ApresData`` after ``load_apres`` of ``.DAT`` files), shaped (bnum, cnum, snum); else None."""
    get = getattr(dat, 'raw_counts', None)
    held = get() if callable(get) else None
    if held is not None:
        shape = (int(dat.bnum), int(dat.cnum), int(dat.snum))
        if held[0].shape != shape:
            raise ValueError('counts are %s, not (bnum, cnum, snum) = %s' % (held[0].shape, shape))
    return held


def range_counts(counts, divisor, t, chunk=0):
    """:func:`range_host` of the chirps that ``counts`` decode to: the counts go up and are widened in HBM."""
    held = [decode_dev(counts, divisor, shape=(counts.size // t.snum, t.snum))]
    try:
        held.extend(range_dev(held[0], t, chunk))
        return tuple(_to_host(d) for d in held[1:])
    finally:
        for d in held:
            d.free()


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
    held = raw_counts(dat)
    if held is not None:
        _set_range(dat, t, *range_counts(held[0], held[1], t))
    else:
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


def phase_uncertainty(dat, bed_range, noise_phase=None):
    """Phase uncertainty from a noise phasor of random phase and the median magnitude below the bed (reference
    :126-153, Kingslake et al. 2014): leaves ``uncertainty`` and ``flags.uncertainty``.  The phase is drawn from
    NumPy's global generator by the reference's own call unless ``noise_phase`` (an array of the data's squeezed
    shape) is given."""
    if dat.flags.range == 0:
        raise TypeError(_MSG_RANGE_FIRST)
    meas = np.squeeze(dat.data)
    # (the first axis of the squeezed data, whatever it is: a per-burst stack is NumPy's IndexError, as in the reference)
    below = np.argwhere(dat.Rcoarse > bed_range)
    median_mag = np.nanmedian(abs(meas[below]))
    if noise_phase is None:
        noise_phase = np.random.uniform(-np.pi, np.pi, np.shape(meas))
    noise = median_mag * (np.cos(noise_phase) + 1j * np.sin(noise_phase))
    noise_orth = median_mag * np.sin(np.angle(meas) - np.angle(noise))
    dat.uncertainty = np.abs(np.arcsin(noise_orth / np.abs(meas)))
    dat.flags.uncertainty = True


def phase_unwrap(diff, win=10, thresh=0.9):
    """Unwrap the phase of ``co`` wherever the coherence around a sample is not all below ``thresh`` (reference
    :96-123): leaves ``phi``.  For ``idx < win`` the slice starts at a negative index and is empty, so nothing is
    unwrapped there -- the reference's behaviour."""
    if diff.flags.phase_diff is None:
        raise ValueError(_MSG_DIFF_FIRST)
    diff.phi = np.angle(diff.co).astype(float)
    for idx in range(1, len(diff.co)):
        if np.all(abs(diff.co[idx - win:idx + win]) < thresh):
            continue
        if diff.phi[idx] - diff.phi[idx - 1] > np.pi:
            diff.phi[idx:] -= 2. * np.pi
        elif diff.phi[idx] - diff.phi[idx - 1] < -np.pi:
            diff.phi[idx:] += 2. * np.pi


def range_diff(diff, uncertainty='noise_phasor'):
    """Phase profile to range offset (reference :126-170): leaves ``w`` and, when ``unc1`` is there, ``w_err`` by the
    Cramer-Rao bound ('CR') or the noise phasor."""
    if not hasattr(diff, 'phi'):
        raise ValueError(_MSG_UNWRAP_FIRST)
    win, step = diff.flags.phase_diff
    h = diff.header
    diff.w = phase2range(diff, diff.phi, h.lambdac, diff.ds, h.chirp_grad, h.ci)
    if diff.unc1 is not None:
        if uncertainty == 'CR':
            sigma = (1. / abs(diff.co)) * np.sqrt((1. - abs(diff.co)**2.) / (2. * win))
            diff.w_err = phase2range(diff, sigma, h.lambdac, diff.ds, h.chirp_grad, h.ci)
        elif uncertainty == 'noise_phasor':
            r_unc = phase2range(diff, diff.unc1, h.lambdac) + phase2range(diff, diff.unc2, h.lambdac)
            idxs = np.arange(win // 2, len(diff.data) - win // 2, step)
            diff.w_err = np.array([np.nanmean(r_unc[i - win // 2:i + win // 2]) for i in idxs])


def strain_rate(diff, strain_window=(200, 1200), w_surf=0.):
    """Mean vertical strain rate over ``strain_window`` by linear regression of ``w`` on ``ds`` (reference :173-200):
    leaves ``eps_zz``, ``w0`` and shifts ``w`` by ``w_surf - w0``."""
    from scipy.stats import linregress
    if not hasattr(diff, 'w'):
        raise ValueError(_MSG_RANGE_DIFF_FIRST)
    print('Calculating vertical strain rate over range from %s to %s meters.' % strain_window)
    idx = np.logical_and(diff.ds > strain_window[0], diff.ds < strain_window[1])
    slope, intercept, r_value, p_value, std_err = linregress(diff.ds[idx], diff.w[idx])
    diff.eps_zz = slope
    diff.w0 = intercept
    print('Vertical strain rate (yr-1):', diff.eps_zz)
    print('r_squared:', r_value**2.)
    diff.w += w_surf - diff.w0


def bed_pick(diff, sample_threshold=50, coherence_threshold=0.9, filt_kernel=201, prominence=10, peak_width=300):
    """The ice-bed interface as the deepest wide, prominent peak of the median-filtered power of both acquisitions
    (reference :203-247): leaves ``bed = [sample, range, coherence, power]``."""
    from scipy.signal import find_peaks, medfilt
    picks, power = [], []
    for acq in (diff.data, diff.data2):
        P = 10. * np.log10(acq**2.)
        mfilt = medfilt(P.real, filt_kernel)
        peaks = find_peaks(mfilt, prominence=prominence, width=peak_width)[0]
        picks.append(max(peaks))
        power.append(mfilt[picks[-1]])
    if not abs(picks[0] - picks[1]) < sample_threshold:
        raise ValueError(_MSG_BED_APART)
    bed_samp = (picks[0] + picks[1]) // 2
    bed_power = (power[0] + power[1]) / 2.
    bed_range = diff.range[bed_samp]
    diff_idx = np.argmin(abs(diff.ds - bed_range))
    bed_coherence = np.median(abs(diff.co[diff_idx - 10:diff_idx + 10]))
    if not bed_coherence > coherence_threshold:
        raise ValueError(_MSG_BED_COHERENCE)
    diff.bed = np.array([bed_samp, bed_range, bed_coherence, bed_power])


def chain(dat, p, max_range=4000, winfun='blackman', num_chirps=None, d_raw=None):
    """Range conversion then stacking with the converted data resident in HBM in between: the raw chirps go up once.
    Leaves what the two calls leave, bit for bit.  With ``d_raw``, a resident (bnum cnum, snum) float64 array of the
    chirps (:func:`decode_dev`), nothing is uploaded and ``dat.data`` is not read; the array stays the caller's."""
    t = range_tables(dat, p, max_range, winfun)
    ctx = _hip.context()
    held = []
    try:
        if d_raw is None:
            counts = raw_counts(dat)
            if counts is not None:
                held.append(decode_dev(counts[0], counts[1], shape=(int(dat.bnum) * int(dat.cnum), int(dat.snum)), ctx=ctx))
            else:
                held.append(_hip.DeviceArray.from_host(ctx, raw_rows(dat)))
            d_raw = held[0]
        elif d_raw.dtype != np.float64 or d_raw.shape != (int(dat.bnum) * int(dat.cnum), int(dat.snum)):
            raise ValueError('d_raw is %s %s, not float64 (bnum cnum, snum) = %s'
                             % (d_raw.dtype, d_raw.shape, (int(dat.bnum) * int(dat.cnum), int(dat.snum))))
        products = range_dev(d_raw, t)
        held.extend(products)
        _set_range(dat, t, *[_to_host(d) for d in products])
        num_chirps, groups, m, per_burst = stack_plan(int(dat.bnum), int(dat.cnum), num_chirps)
        d_mean = stack_dev(products[1], groups, m)
        held.append(d_mean)
        _set_stack(dat, _to_host(d_mean), num_chirps, per_burst)
    finally:
        for d in held:
            d.free()


def single_processing(dat, p=2, max_range=4000., num_chirps=0., noise_bed_range=3000.):
    """The reference's full flow for one acquisition (``apdar.py:337-345``): :func:`chain`, then
    :func:`phase_uncertainty`.  ``num_chirps = 0`` stacks everything."""
    if num_chirps == 0.:
        chain(dat, p, max_range)
    else:
        chain(dat, p, max_range, num_chirps=num_chirps)
    phase_uncertainty(dat, noise_bed_range)


def time_diff_processing(diff, win=20, step=20, thresh=0.95, strain_window=(200, 1000), w_surf=-0.15):
    """The reference's full flow for a pair of acquisitions (``apdar.py:348-354``): the phase difference on the GPU,
    then unwrapping, range difference, strain rate and bed pick on the host."""
    phase_diff(diff, win, step)
    phase_unwrap(diff, win, thresh)
    range_diff(diff)
    strain_rate(diff, strain_window=strain_window, w_surf=w_surf)
    bed_pick(diff)
