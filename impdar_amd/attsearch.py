"""The growing-window search of the attenuation methods 3 and 6b on the MI355X (``csrc/attsearch.hip``), its NumPy
restatement for a machine without a GPU, and what turns the per-centre outcomes into the reference's arrays or
exceptions."""
import ctypes as C
import warnings

import numpy as np

from . import _hip

INDEX, DEPTH = 0, 1                                   # method 3 (index windows), method 6b (depth windows)
VALUE, NOT_ENTERED, TIE, NONFINITE = 0, 1, 2, 3       # what a centre ended as (csrc/att_route.h)
MAX_WINDOWS = 1 << 20                                 # csrc/att_route.h: ATT_MAX_WINDOWS
MAX_PROBE_ROWS = 1 << 16                              # the probe's table is rows x len(Ns) doubles on the host


def zero_rate(ns):
    """The index of the rate 0 in ``ns``.  The reference compares ``C[Ns == 0]`` with ``Cw``: no such entry, or several,
    has no truth value there (``ValueError``)."""
    at = np.flatnonzero(np.asarray(ns) == 0)
    if at.size != 1:
        raise ValueError('Ns must hold the rate 0 exactly once (it holds it %d times): C[Ns == 0] > Cw has no truth value' % at.size)
    return int(at[0])


def check_walk(flavour, z, win_init, win_step):
    """The widths a search accepts, with or without a device (``csrc/att_route.h``: ``att_route``, ``att_depth_walk_bad``):
    ``ValueError`` for an index width below 2 (its first window would be empty) or a fraction, and for a step with which a
    walk could not end, or only after more than ``MAX_WINDOWS`` steps across the depth range."""
    if flavour == INDEX:
        if not (2 <= win_init < 2 ** 62 and win_init == int(win_init)):
            raise ValueError('win_init must be an integer >= 2, not %r' % (win_init,))
        if not (1 <= win_step < 2 ** 62 and win_step == int(win_step)):
            raise ValueError('win_step must be an integer >= 1, not %r: the window would never grow' % (win_step,))
        return
    if not (0. < win_init <= 1.7e308 and 0. < win_step <= 1.7e308):
        raise ValueError('win_init and win_step must be positive and finite, not %r and %r' % (win_init, win_step))
    if len(z) == 0:
        return
    z0, zn = float(z[0]), float(z[-1])
    span = zn - z0
    if not (np.isfinite(z0) and np.isfinite(zn) and 2. * span <= 1.7e308):
        raise ValueError('the pick depths are not finite')
    if np.float64(2. * span) + np.float64(win_step) / 2. == 2. * span:
        raise ValueError('win_step %r does not advance a window as wide as the depth range %r: the search would not end' % (win_step, span))
    if not span / win_step <= MAX_WINDOWS:
        raise ValueError('win_step %r is more than 2^20 steps across the depth range %r' % (win_step, span))


def probe_rows_bound(flavour, z, win_init, win_step):
    """No centre visits more windows than this (``ValueError`` where a probe's table would not be one to hold)."""
    if flavour == INDEX:
        rows = max(1, (len(z) - int(win_init)) // int(win_step) + 2)
    else:
        rows = max(1, int(min(max(2. * ((z[-1] - z[0]) - win_init) / win_step, 0.0), 4. * MAX_WINDOWS)) + 3)
    if rows > MAX_PROBE_ROWS:
        raise ValueError('a probed centre could visit %d windows: its table is limited to %d rows' % (rows, MAX_PROBE_ROWS))
    return rows


def search_dev(flavour, z, pc, ns, cw, nh_target, win_init, win_step, centres=None, first=0, ncent=None, probe=None):
    """``impdar_att_search`` (``include/impdar_hip.h``): ``(idx, win, code)`` per centre -- the rate index at the minimum of
    the last window visited, the width after the last increment, the outcome code -- and with ``probe`` a centre's number
    also the ``C`` rows of the windows it visited.  ``z``, ``pc``: the NaN-free pairs, sorted by ``z`` for ``DEPTH``."""
    lib = _hip.load()
    ctx = _hip.context()
    z, p_z = _hip.as_dp(z)
    pc, p_pc = _hip.as_dp(pc)
    ns, p_ns = _hip.as_dp(ns)
    if not (z.ndim == pc.ndim == ns.ndim == 1 and z.size == pc.size):
        raise ValueError('search_dev takes one-dimensional z, pc of one length and one-dimensional rates')
    j0 = zero_rate(ns)
    centres, p_c = _hip.as_dp(centres)
    if flavour == DEPTH:
        if centres is None or centres.ndim != 1:
            raise ValueError('the depth form takes a one-dimensional array of centres')
        ncent = centres.size
    ncent = int(ncent)
    idx = np.empty(max(ncent, 0), dtype=np.int64)
    win = np.empty(max(ncent, 0), dtype=np.float64)
    code = np.empty(max(ncent, 0), dtype=np.int32)
    outs = (idx.ctypes.data_as(C.POINTER(C.c_longlong)), win.ctypes.data_as(_hip._dp), code.ctypes.data_as(_hip._ip))
    head = (ctx, int(flavour), p_z, p_pc, z.size, p_ns, ns.size, j0, p_c, int(first), ncent, float(win_init), float(win_step),
            float(cw), float(nh_target)) + outs
    if probe is None:
        _hip.check(lib.impdar_att_search(*(head + (-1, None, 0, None))), 'impdar_att_search')
        return idx, win, code
    cap = probe_rows_bound(flavour, z, win_init, win_step) if z.size and win_step > 0 and win_init > 0 else 1
    table = np.full((cap, ns.size), np.nan)
    rows = C.c_longlong(0)
    _hip.check(lib.impdar_att_search(*(head + (int(probe), table.ctypes.data_as(_hip._dp), cap, C.byref(rows)))), 'impdar_att_search')
    if rows.value > cap:
        raise RuntimeError('impdar_att_search: the probed centre visited %d windows, more than the bound %d' % (rows.value, cap))
    return idx, win, code, table[:rows.value]


def centre_host(flavour, z, pc, ns, cw, nh_target, win_init, win_step, centre, table=None):
    """One centre's walk with NumPy, comparisons and non-finite values as NumPy has them: ``(code, idx, win)`` with code
    ``VALUE``, ``NOT_ENTERED`` or ``TIE`` (no rate, or several, at the minimum of the last window).  ``centre``: the trace
    (``INDEX``) or the depth (``DEPTH``).  ``table``: a list that takes the ``C`` row of every window visited."""
    n, win, nh, found = len(z), win_init, nh_target + 1., None
    zero = ns == 0
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        while True:
            if flavour == INDEX:
                if not (nh > nh_target and win // 2 <= centre and win // 2 <= n - centre):
                    break
                sel = slice(centre - win // 2, centre + win // 2)
            else:
                if not (nh > nh_target and centre - win / 2 >= z[0] and centre + win / 2 <= z[-1]):
                    break
                sel = abs(z - centre) < win / 2
            zw, pw = z[sel], pc[sel]
            dz = zw - (np.mean(zw) if zw.size else np.nan)
            pa = pw[None, :] + 2. * zw[None, :] * ns[:, None]
            dpa = pa - (np.mean(pa, axis=1)[:, None] if zw.size else np.nan)
            s1, s2, s3 = np.sum(dz[None, :] * dpa, axis=1), np.sqrt(np.sum(dz ** 2.)), np.sqrt(np.sum(dpa ** 2., axis=1))
            cs = np.abs(s1 / (s2 * s3))
            if table is not None:
                table.append(cs)
            cm = np.min(cs) if flavour == INDEX else np.nanmin(cs)
            found = np.flatnonzero(cs == cm)
            below = ns[cs < cw]
            if cm < cw and cs[zero] > cw:
                nh = np.max(below) - np.min(below) if flavour == INDEX else (np.max(below) - np.min(below)) / 2.
            win += win_step
    if found is None:
        return NOT_ENTERED, -1, win
    return (VALUE, int(found[0]), win) if found.size == 1 else (TIE, -1, win)


def search_host(flavour, z, pc, ns, cw, nh_target, win_init, win_step, centres):
    """``search_dev`` without a device."""
    zero_rate(ns)
    out = [centre_host(flavour, z, pc, ns, cw, nh_target, win_init, win_step, c) for c in centres]
    return (np.array([o[1] for o in out], dtype=np.int64), np.array([o[2] for o in out], dtype=np.float64),
            np.array([o[0] for o in out], dtype=np.int32))


def search(flavour, z, pc, ns, cw, nh_target, win_init, win_step, centres):
    """Every centre's ``(idx, win, code)``: on the device where there is one, else with NumPy; a centre whose windows held a
    non-finite ``C`` is walked again with NumPy, whose comparison rules then decide as they do in the reference.  Widths
    with which a walk could not end are a ``ValueError`` on either path (``check_walk``)."""
    ns = np.ascontiguousarray(ns, dtype=np.float64)
    zero_rate(ns)
    check_walk(flavour, z, win_init, win_step)
    if len(centres) == 0:
        return np.empty(0, dtype=np.int64), np.empty(0), np.empty(0, dtype=np.int32)
    if len(z) == 0:
        return (np.full(len(centres), -1, dtype=np.int64), np.full(len(centres), float(win_init)),
                np.full(len(centres), NOT_ENTERED, dtype=np.int32))
    if _hip.device_count() <= 0:
        return search_host(flavour, z, pc, ns, cw, nh_target, win_init, win_step, centres)
    if flavour == INDEX:
        idx, win, code = search_dev(flavour, z, pc, ns, cw, nh_target, win_init, win_step, first=centres[0], ncent=len(centres))
    else:
        idx, win, code = search_dev(flavour, z, pc, ns, cw, nh_target, win_init, win_step, centres=centres)
    for b in np.flatnonzero(code == NONFINITE):
        code[b], idx[b], win[b] = centre_host(flavour, z, pc, ns, cw, nh_target, win_init, win_step, centres[b])
    return idx, win, code


def settle(ns, idx, win, code):
    """The reference's loop over the centres, given their outcomes: the rate of a centre that visited no window is the one
    left over from the centre before (``UnboundLocalError`` where there is none yet), a minimum that is no single rate is
    the ``ValueError`` of the reference's assignment.  Returns ``(rates, widths)``, one per centre."""
    rates, left = np.empty(len(code)), None
    for b in range(len(code)):
        if code[b] == VALUE:
            left = ns[idx[b]]
        elif code[b] == TIE:
            raise ValueError('centre %d: the smallest correlation of the last window belongs to no single rate of Ns' % b)
        elif left is None:
            raise UnboundLocalError("cannot access local variable 'Nm' where it is not associated with a value")
        rates[b] = left
    return rates, np.asarray(win, dtype=np.float64)
