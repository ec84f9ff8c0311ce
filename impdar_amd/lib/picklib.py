"""The mechanics of picking with the reference's names, signatures and return shapes
(``src/impdar/lib/picklib.py:16-199``), run on the MI355X: everything that reads the radargram goes through
``impdar_amd.picking`` and ``csrc/pick.hip``.  ``get_intersection``, O(picks) host work on what these write, is not
part of this engine.
"""
import numpy as np

from .. import picking


def _params(pickparams):
    return picking.params(pickparams)


def auto_pick(dat, snums, tnums):
    """Pick a reflector from every seed ``(snums[i], tnums[i])`` over all traces: (len(snums), 5, tnum), rows top,
    centre, bottom of the packet, NaN and power.  Reads the resident array when the radargram is on the device."""
    prm = _params(dat.picks.pickparams)
    dev = getattr(dat, '_dev', None)
    if dev is not None:
        return picking.auto_pick_dev(dev, snums, tnums, *prm)
    return picking.auto_pick_host(dat.data, snums, tnums, *prm)


def pick(traces, snum_start, snum_end, pickparams):
    """Pick in every trace of ``traces`` (snum, n) along the line from row ``snum_start`` to ``snum_end``: (5, n)."""
    traces = np.asarray(traces)
    return picking.pick_host(traces, 0, _midpoint(traces.shape[1], snum_start, snum_end), *_params(pickparams))


def _midpoint(len_tnums, snum_start, snum_end):
    return picking.midpoints(len_tnums, snum_start, snum_end)


def packet_power(trace, plength, midpoint):
    """The packet of ``plength`` samples around ``midpoint`` (a view of the trace) and the row of its first sample."""
    if len(trace.shape) > 1:
        raise ValueError('Need a single, flat trace')
    topsnum = int(midpoint - plength / 2.)
    return trace[topsnum:int(midpoint + plength / 2.)], topsnum


def packet_pick(trace, pickparams, midpoint):
    """One pick: [top, centre, bottom, NaN, power] of the packet around ``midpoint``."""
    trace = np.asarray(trace)
    if trace.ndim > 1:
        raise ValueError('Need a single, flat trace')
    out = picking.pick_host(trace[:, None], 0, [midpoint], *_params(pickparams))[:, 0]
    return [int(out[0]), int(out[1]), int(out[2]), np.nan, out[4]]
