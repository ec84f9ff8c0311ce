"""Picking as the last step of a chain: ``pick_layers`` (the reference's ``picklib.auto_pick`` with the bookkeeping
its GUI does around it, ``Picks.add_pick`` and ``update_pick``) and ``continuity_index``
(``src/impdar/lib/analysis/continuity_index.py:27-81``), both on the radargram where it is -- resident or on the
host.  Only the picks or the index come back from the device.
"""
import numpy as np

from ... import picking
from .. import picklib
from ..Picks import Picks


def pick_layers(self, snums, tnums, picknums=None, freq=None, pol=None):
    """Pick one layer per seed ``(snums[i], tnums[i])`` and store them in ``self.picks`` (built from the loaded
    ``picks`` struct when there is one, else blank).  ``freq`` and ``pol`` update the pick parameters first;
    ``picknums`` default to the numbers after the largest present.  If any pick fails the reference's error is raised
    and ``self.picks`` is left as it was."""
    if len(snums) != len(tnums):
        raise ValueError('Snum and tnum must be of equal length')
    had = self.picks
    picks = had if had is not None else Picks(self, self._picks_struct)
    params = picks.pickparams
    before = (params.freq, params.plength, params.FWW, params.scst, params.pol)
    try:
        if freq is not None:
            params.freq_update(freq)
        if pol is not None:
            params.pol = pol
        present = [] if picks.picknums is None else [int(p) for p in np.asarray(picks.picknums).reshape(-1)]
        if picknums is None:
            first = max(present) + 1 if present else 1
            picknums = list(range(first, first + len(snums)))
        if len(picknums) != len(snums):
            raise ValueError('picknums and snums must be of equal length')
        if len(set(picknums)) != len(picknums) or set(picknums) & set(present):
            raise ValueError('We already have that pick')
        self.picks = picks          # auto_pick reads dat.picks.pickparams, as the reference's does
        out = picklib.auto_pick(self, snums, tnums)
    except Exception:
        params.freq, params.plength, params.FWW, params.scst, params.pol = before
        self.picks = had
        raise
    for k, num in enumerate(picknums):
        picks.add_pick(num)
        picks.update_pick(num, out[k])
    return out


def continuity_index(self, b_ind, s_ind=None, cutoff_ratio=None):
    """Karlsson et al. (2012) continuity index of every trace between pick ``s_ind`` (default: the first sample) and
    pick ``b_ind`` (rows of ``picks.samp1``), into ``self.continuity_index_`` -- the reference assigns
    ``dat.continuity_index``, which would replace this method."""
    bpick = np.asarray(self.picks.samp1[b_ind], dtype=np.float64)
    spick = np.zeros_like(bpick) if s_ind is None else np.asarray(self.picks.samp1[s_ind], dtype=np.float64)
    dev = getattr(self, '_dev', None)
    snum = dev.shape[0] if dev is not None else np.shape(self.data)[0]
    s, b = picking.continuity_bounds(spick, bpick, snum)
    if dev is not None:
        self.continuity_index_ = picking.continuity_dev(dev, s, b, cutoff_ratio)
    else:
        self.continuity_index_ = picking.continuity_host(self.data, s, b, cutoff_ratio)
    return self.continuity_index_
