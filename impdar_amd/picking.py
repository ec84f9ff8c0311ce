"""Host side of layer picking: ``auto_pick``, the guided ``pick`` and the continuity index.  The seed checks, the
midpoints of a guided line and the slice bounds of the continuity windows -- O(seeds) and O(tnum) work -- are NumPy
here; everything that reads the (snum, tnum) radargram runs in ``csrc/pick.hip`` through the C ABI, on host buffers
or on an array that is already resident in HBM.  Only the picks (``nseeds * 5 * tnum`` doubles) or the index
(``tnum`` doubles) come back.

A pick that the reference refuses is refused here with the reference's error: the C calls report, per seed or per
line, the outcome and trace of the first pick that failed in the reference's order, and ``raise_outcome`` turns it
into the ``ValueError`` the reference would have raised there.

Reference: ``src/impdar/lib/picklib.py:16-199``, ``src/impdar/lib/analysis/continuity_index.py:27-81``.
"""
import ctypes as C

import numpy as np

from . import _hip

_IP = C.POINTER(C.c_int)

OK, SHORT, EMPTY_ARGMAX, EMPTY_ARGMIN = 0, 1, 2, 3
# picklib.py:165-166: a string continued over a line break keeps the indentation of its second line
SHORT_MESSAGE = 'Your choice of frequency is too high, ' + ' ' * 25 + 'making the pick window sub-pixel in size'
MESSAGES = {SHORT: SHORT_MESSAGE,
            EMPTY_ARGMAX: 'attempt to get argmax of an empty sequence',
            EMPTY_ARGMIN: 'attempt to get argmin of an empty sequence'}


def raise_outcome(code):
    """The reference's ``ValueError`` for a pick that failed (``packet_pick``'s own, or NumPy's for an empty slice)."""
    if code != OK:
        raise ValueError(MESSAGES[int(code)])


def params(pickparams):
    """``(plength, FWW, scst, pol)`` of a ``PickParameters`` as the ints the kernels take."""
    pol = int(pickparams.pol)
    if pol not in (1, -1):
        raise ValueError('pol must be 1 or -1, got %r' % (pickparams.pol,))
    return int(pickparams.plength), int(pickparams.FWW), int(pickparams.scst), pol


def _whole(values, what):
    a = np.asarray(values, dtype=np.float64).reshape(-1)
    if a.size and (not np.all(np.isfinite(a)) or np.any(a != np.floor(a)) or np.any(np.abs(a) > 2**31 - 1)):
        raise ValueError('%s must be whole numbers' % what)
    return a.astype(np.int32)


def check_seeds(snums, tnums, tnum):
    """int32 seed rows and traces.  Lengths that differ are the reference's ``ValueError``, a seed trace beyond the
    data its ``IndexError``; a negative seed trace or sample is refused (the reference re-picks one trace ``tnum``
    times there: a documented divergence)."""
    if len(snums) != len(tnums):
        raise ValueError('Snum and tnum must be of equal length')
    s, t = _whole(snums, 'seed samples'), _whole(tnums, 'seed traces')
    if s.size == 0:
        return s, t
    if np.any(t >= tnum):
        raise IndexError('index %d is out of bounds for axis 1 with size %d' % (int(t[t >= tnum][0]), tnum))
    if np.any(t < 0) or np.any(s < 0):
        raise ValueError('seed traces and samples must not be negative')
    return s, t


def _finish_auto(rc, out, status):
    _hip.check(rc, 'impdar_auto_pick')
    for code, _ in status:          # the lowest-numbered seed that failed is the one the reference reaches first
        raise_outcome(code)
    return out


def _auto_pick(fn, ctx, ptr, dtype, shape, snums, tnums, plength, FWW, scst, pol):
    snum, tnum = shape
    s, t = check_seeds(snums, tnums, tnum)
    out = np.empty((len(s), 5, tnum), dtype=np.float64)
    if len(s) == 0:
        return out
    status = np.zeros((len(s), 2), dtype=np.int32)
    rc = fn(ctx, ptr, _hip.dtype_code(dtype), snum, tnum, len(s), s.ctypes.data_as(_IP), t.ctypes.data_as(_IP), int(plength),
            int(FWW), int(scst), int(pol), _hip.as_dp(out)[1], status.ctypes.data_as(_IP))
    return _finish_auto(rc, out, status)


def auto_pick_host(data, snums, tnums, plength, FWW, scst, pol):
    """``picklib.auto_pick`` of a host radargram: (nseeds, 5, tnum) float64 (integers widened first)."""
    work = _hip.work_array(data, 'picks in complex data are', copy=False)
    return _auto_pick(_hip.load().impdar_auto_pick, _hip.context(), work.ctypes.data_as(C.c_void_p), work.dtype, work.shape,
                      snums, tnums, plength, FWW, scst, pol)


def auto_pick_dev(d_arr, snums, tnums, plength, FWW, scst, pol):
    """The same of a resident :class:`impdar_amd._hip.DeviceArray` (float32 / float64), which stays where it is."""
    return _auto_pick(_hip.load().impdar_auto_pick_dev, d_arr.ctx, d_arr.ptr, d_arr.dtype, d_arr.shape, snums, tnums,
                      plength, FWW, scst, pol)


# ------------------------------------------------------------------------------------------------ guided pick
def midpoints(n, snum_start, snum_end):
    """The reference's ``_midpoint``: the rows of a straight line over ``n`` traces; a start of -9999 makes it flat."""
    if snum_start == -9999:
        snum_start = snum_end
    return np.round(np.arange(n) * (snum_end - snum_start) / n) + snum_start


def _pick(fn, ctx, ptr, dtype, shape, t0, mid, plength, FWW, scst, pol):
    snum, tnum = shape
    mid = _whole(mid, 'midpoints')
    n = len(mid)
    out = np.full((5, n), np.nan, dtype=np.float64)
    if n == 0:
        return out
    status = np.zeros((2,), dtype=np.int32)
    rc = fn(ctx, ptr, _hip.dtype_code(dtype), snum, tnum, int(t0), n, mid.ctypes.data_as(_IP), int(plength), int(FWW),
            int(scst), int(pol), _hip.as_dp(out)[1], status.ctypes.data_as(_IP))
    _hip.check(rc, 'impdar_pick_guided')
    raise_outcome(status[0])
    return out


def pick_host(data, t0, mid, plength, FWW, scst, pol):
    """``packet_pick`` of traces ``t0 ... t0 + len(mid) - 1`` of a host radargram around the rows ``mid``: (5, n)."""
    work = _hip.work_array(data, 'picks in complex data are', copy=False)
    return _pick(_hip.load().impdar_pick_guided, _hip.context(), work.ctypes.data_as(C.c_void_p), work.dtype, work.shape, t0,
                 mid, plength, FWW, scst, pol)


def pick_dev(d_arr, t0, mid, plength, FWW, scst, pol):
    """The same of a resident :class:`impdar_amd._hip.DeviceArray`."""
    return _pick(_hip.load().impdar_pick_guided_dev, d_arr.ctx, d_arr.ptr, d_arr.dtype, d_arr.shape, t0, mid, plength, FWW,
                 scst, pol)


# ------------------------------------------------------------------------------------------------ continuity index
def continuity_bounds(spick, bpick, snum):
    """int32 ``(s, b)`` per trace: the bounds of ``slice(int(spick), int(bpick)).indices(snum)`` -- Python's slice
    semantics, as the reference's ``P[s:b, tr]`` -- and -1 in both where either pick is NaN."""
    spick, bpick = np.asarray(spick, dtype=np.float64), np.asarray(bpick, dtype=np.float64)
    s = np.full(spick.shape, -1, dtype=np.int32)
    b = np.full(spick.shape, -1, dtype=np.int32)
    for j in range(len(s)):
        if not (np.isnan(spick[j]) or np.isnan(bpick[j])):
            s[j], b[j], _ = slice(int(spick[j]), int(bpick[j])).indices(snum)
    return s, b


def _continuity(fn, ctx, ptr, dtype, shape, s, b, cutoff_ratio):
    snum, tnum = shape
    s, b = np.ascontiguousarray(s, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32)
    if s.shape != (tnum,) or b.shape != (tnum,):
        raise ValueError('the picks need length tnum %d' % tnum)
    out = np.empty((tnum,), dtype=np.float64)
    rc = fn(ctx, ptr, _hip.dtype_code(dtype), snum, tnum, s.ctypes.data_as(_IP), b.ctypes.data_as(_IP),
            0 if cutoff_ratio is None else 1, 0.0 if cutoff_ratio is None else float(cutoff_ratio), _hip.as_dp(out)[1])
    _hip.check(rc, 'impdar_continuity')
    return out


def continuity_host(data, s, b, cutoff_ratio=None):
    """Continuity index of every trace of a host radargram between the slice bounds ``s`` and ``b``."""
    work = _hip.work_array(data, 'a continuity index of complex data is', copy=False)
    return _continuity(_hip.load().impdar_continuity, _hip.context(), work.ctypes.data_as(C.c_void_p), work.dtype, work.shape,
                       s, b, cutoff_ratio)


def continuity_dev(d_arr, s, b, cutoff_ratio=None):
    """The same of a resident :class:`impdar_amd._hip.DeviceArray`."""
    return _continuity(_hip.load().impdar_continuity_dev, d_arr.ctx, d_arr.ptr, d_arr.dtype, d_arr.shape, s, b, cutoff_ratio)
