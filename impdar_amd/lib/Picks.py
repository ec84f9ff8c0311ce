"""The picks of a radargram: per pick and trace the rows of the packet's top, centre and bottom and its power, and
the parameters they were picked with.  Restates the reference's ``src/impdar/lib/Picks.py:19-218, 344-363``
(construction from a ``.mat`` struct or blank, ``add_pick``, ``update_pick``, ``to_struct``, ``__str__``) in this
project's own text.

Picking is the last step of a chain here: the reference's methods that move picks with the data (``reverse``,
``hcrop``, ``crop``, ``restack``) and ``smooth`` are not part of this class, and the ``RadarData`` steps that would
call them refuse an object that carries picks.
"""
import numpy as np

from .LastTrace import LastTrace
from .LeaderTrailer import LeaderTrailer
from .PickParameters import PickParameters


class Picks(object):
    """``samp1`` / ``samp2`` / ``samp3`` / ``time`` / ``power``: (npicks, tnum) arrays (top, centre, bottom row of every
    pick, the deprecated time, the power); ``picknums``: the number of each pick; ``lasttrace``, ``lt``,
    ``pickparams``: the records saved with them."""

    attrs = ['samp1', 'samp2', 'samp3', 'time', 'power', 'picknums']
    flatten = [False, False, False, False, False, True]
    spec_attrs = ['lasttrace', 'lt', 'pickparams']
    _rows = ['samp1', 'samp2', 'samp3', 'time', 'power']

    def __init__(self, radardata, pick_struct=None):
        if pick_struct is not None:
            for attr, flat in zip(self.attrs, self.flatten):
                val = pick_struct[attr][0][0]
                if flat:
                    val = val.flatten()
                if val.shape == (1, 1) and val[0][0] == 0:    # matlab's stand-in for None
                    val = None
                setattr(self, attr, val)
            self.lasttrace = LastTrace(pick_struct['lasttrace'])
            self.lt = LeaderTrailer(radardata, pick_struct['lt'])
            self.pickparams = PickParameters(radardata, pick_struct['pickparams'])
            self.picknums = self.picknums.tolist()
        else:
            for attr in self.attrs:
                setattr(self, attr, None)
            self.lasttrace = LastTrace()
            self.lt = LeaderTrailer(radardata)
            self.pickparams = PickParameters(radardata)
        self.radardata = radardata
        self.lines = []

    def __str__(self):
        try:
            if self.samp1 is None:
                return 'Empty pick object'
            rows = np.nanmean(self.samp1, axis=1).astype(int)
            rows[rows < 0] = 0      # an all-NaN pick
            twtt = self.radardata.travel_time[rows]
            if self.radardata.nmo_depth is not None:
                note, depth = '', self.radardata.nmo_depth[rows]
            else:
                note, depth = ' assuming 1.68e8 m/s vel', twtt / 2.0 * 1.68e3
            string = 'Pick object with {:d} picks:'.format(len(self.picknums))
            for i, num in enumerate(self.picknums):
                if rows[i] != 0:
                    string += '\n    pick {:d} at ~{:4.2f} us (~{:4.2f} m{:s})'.format(int(num), twtt[i], depth[i], note)
                else:
                    string += '\n    empty pick {:d}'.format(int(num))
            return string
        except (ValueError, TypeError, IndexError):
            return 'Picks Object'

    def _blank_row(self):
        return np.full((1, self.radardata.tnum), np.nan)

    def add_pick(self, picknum=0):
        """A new, all-NaN pick called ``picknum``; returns the number of picks.  The first pick creates the arrays; a
        last pick that is still blank is re-used under the new number; a number that exists is a ``ValueError``."""
        if self.samp1 is None:
            for attr in self._rows:
                setattr(self, attr, self._blank_row())
            self.picknums = [picknum]
            self.lasttrace.add_pick(-9999, 0)
        elif np.all(np.isnan(self.samp1[-1, :])):
            for attr in self._rows:
                getattr(self, attr)[-1, :] = np.nan
            self.picknums[-1] = picknum
        else:
            if isinstance(self.picknums, np.ndarray):
                self.picknums = self.picknums.flatten().tolist()
            if picknum in self.picknums:
                raise ValueError('We already have that pick')
            for attr in self._rows:
                setattr(self, attr, np.vstack((getattr(self, attr), self._blank_row())))
            self.lasttrace.add_pick(-9999, 0)
            self.picknums.append(picknum)
        return self.samp1.shape[0]

    def update_pick(self, picknum, pick_info):
        """Store the (5, tnum) rows top, centre, bottom, time and power of pick ``picknum``."""
        try:
            ind = self.picknums.index(picknum)
        except ValueError:
            raise ValueError('picknum provided is not a pick; you must use a picknum not an index')
        if pick_info.shape != (5, self.radardata.tnum):
            raise ValueError('pick_info must be a 5xtnum array')
        for k, attr in enumerate(self._rows):
            getattr(self, attr)[ind, :] = pick_info[k, :]

    def to_struct(self):
        """Attributes as a dict for ``scipy.io.savemat`` (0 stands for None)."""
        mat = {attr: (getattr(self, attr) if getattr(self, attr) is not None else 0) for attr in self.attrs}
        for attr in self.spec_attrs:
            mat[attr] = getattr(self, attr).to_struct() if getattr(self, attr) is not None else 0
        return mat
