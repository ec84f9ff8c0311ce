"""Host side of the steps that change the trace axis of a radargram: ``reverse``, ``hcrop`` and ``restack``.  The
index rules and the per-trace attribute vectors are NumPy here, as in the reference; what touches the (snum, tnum)
radargram runs in ``csrc/taxis.hip`` through the C ABI.  On a host array ``reverse`` and ``hcrop`` are a view and a
slice, as a scalar ``crop`` is; on an array resident in HBM they are a row-reversal kernel and a strided copy.

Reference: ``src/impdar/lib/RadarData/_RadarDataProcessing.py:20-47, 340-453``.
"""
import ctypes as C

import numpy as np

from . import _hip

# the per-trace vectors each step touches, in the reference's order
REVERSED_ATTRS = ['x_coord', 'y_coord', 'decday', 'lat', 'long', 'elev']
HCROPPED_ATTRS = ['lat', 'long', 'pressure', 'trace_int', 'trig', 'elev', 'x_coord', 'y_coord', 'decday']
RESTACKED_ATTRS = ['dist', 'pressure', 'lat', 'long', 'x_coord', 'y_coord', 'elev', 'decday', 'trig']


# ------------------------------------------------------------------------------------------------ reverse
def reverse_dev(d_arr):
    """In place on a resident :class:`impdar_amd._hip.DeviceArray` (float32 / float64)."""
    snum, tnum = d_arr.shape
    if d_arr.nbytes:
        rc = _hip.load().impdar_reverse_dev(d_arr.ctx, d_arr.ptr, _hip.dtype_code(d_arr.dtype), snum, tnum)
        _hip.check(rc, 'impdar_reverse')


# ------------------------------------------------------------------------------------------------ hcrop
def hcrop_lims(lim, left_or_right, dimension, dist, tnum):
    """The trace range ``[lo, hi)`` that ``hcrop`` keeps, as Python slice bounds (a negative ``lim`` gives a
    negative bound): the reference's checks, messages and index rules (:361-384).  ``tnum`` is 1-indexed; ``dist``
    cuts at the first trace at or past ``lim``."""
    if left_or_right not in ['left', 'right']:
        raise ValueError('left_or_right must be left or right, not {:s}'.format(left_or_right))
    if dimension not in ['tnum', 'dist']:
        raise ValueError('Dimension must be in ["tnum", "dist"]')
    if dimension == 'dist':
        if lim > np.max(dist):
            raise ValueError('lim is larger than largest distance')
        if lim <= 0:
            raise ValueError('Distance should be strictly positive')
        ind = int(np.min(np.argwhere(dist >= lim)))
    else:
        if int(lim) in (0, 1):
            raise ValueError('lim should be at least two to preserve some data')
        if lim > tnum:
            raise ValueError('lim should be less than tnum+1 {:d} in order to do anything'.format(tnum + 1))
        if lim == -1 or lim < -int(tnum):
            raise ValueError('If negative, lim should be in [-self.tnum; -1)')
        ind = int(lim) - 1
    return [ind, tnum] if left_or_right == 'left' else [0, ind]


def col_range_dev(d_arr, lo, hi):
    """New resident array of the array's own dtype holding its traces ``[lo:hi]`` (Python slice bounds); the
    caller frees the old one."""
    snum, tnum = d_arr.shape
    lo, hi, _ = slice(lo, hi).indices(tnum)
    hi = max(hi, lo)
    with _hip.new_device_array(d_arr.ctx, (snum, hi - lo), d_arr.dtype) as d_out:
        if d_out.nbytes:
            rc = _hip.load().impdar_hcrop_dev(d_arr.ctx, d_arr.ptr, _hip.dtype_code(d_arr.dtype), snum, tnum, lo, hi,
                                             d_out.ptr)
            _hip.check(rc, 'impdar_hcrop')
    return d_out


# ------------------------------------------------------------------------------------------------ restack
def restack_count(traces, tnum):
    """``(traces, tnum_new)``: the odd number of traces per stack (an even request is bumped, with the reference's
    message) and the number of whole stacks."""
    traces = int(traces)
    if traces % 2 == 0:
        print('Only will stack odd numbers of traces. Using {:d}'.format(int(traces + 1)))
        traces = traces + 1
    return traces, int(np.floor(tnum / traces))


def block_means(val, traces, tnum_new):
    """float64 means of the first ``tnum_new`` blocks of ``traces`` entries of a per-trace vector."""
    return np.array([np.mean(val[j * traces:(j + 1) * traces]) for j in range(tnum_new)], dtype=np.float64).reshape((tnum_new,))


def restack_host(data, traces):
    """float64 (snum, tnum // traces) block means of a host radargram (integers widened to float64 first)."""
    work = _hip.work_array(data, 'restacking complex data is', copy=False)
    snum, tnum = work.shape
    out = np.empty((snum, tnum // traces), dtype=np.float64)
    if out.size == 0:
        return out
    rc = _hip.load().impdar_restack(_hip.context(), work.ctypes.data_as(C.c_void_p), _hip.dtype_code(work.dtype), snum,
                                   tnum, int(traces), out.ctypes.data_as(C.c_void_p))
    _hip.check(rc, 'impdar_restack')
    return out


def restack_dev(d_arr, traces):
    """New resident float64 (snum, tnum // traces) array; the caller frees the old one."""
    snum, tnum = d_arr.shape
    with _hip.new_device_array(d_arr.ctx, (snum, tnum // traces), np.float64) as d_out:
        if d_out.nbytes:
            rc = _hip.load().impdar_restack_dev(d_arr.ctx, d_arr.ptr, _hip.dtype_code(d_arr.dtype), snum, tnum,
                                               int(traces), d_out.ptr)
            _hip.check(rc, 'impdar_restack')
    return d_out
