"""Where each pick was last touched: a StoDeep legacy that picked files carry.  Restates the reference's
``src/impdar/lib/LastTrace.py:13-115`` in this project's own text."""
import numpy as np


class LastTrace(object):
    """``snum`` and ``tnum``: per pick, the sample and trace last picked (None until there is a pick)."""

    attrs = ['snum', 'tnum']

    def __init__(self, lasttrace_struct=None):
        self.snum = None
        self.tnum = None
        if lasttrace_struct is not None:
            for attr in self.attrs:
                val = lasttrace_struct[0][0][attr][0][0].flatten()
                setattr(self, attr, None if (len(val) == 1 and val[0] == -9999) else val)

    def add_pick(self, snum, tnum):
        """Append the entry of a new pick."""
        if self.snum is None:
            self.snum = [snum]
            self.tnum = [tnum]
            return
        for attr in self.attrs:     # loaded as arrays, appended to as lists
            if isinstance(getattr(self, attr), np.ndarray):
                setattr(self, attr, getattr(self, attr).flatten().tolist())
        self.snum.append(int(snum))
        self.tnum.append(int(tnum))

    def mod_line(self, ind, snum, tnum):
        """Overwrite the entry of pick ``ind``."""
        if self.snum is None or self.tnum is None:
            raise AttributeError('need snum and tnum defined')
        if len(self.snum) <= ind or len(self.tnum) <= ind:
            raise ValueError('Index is too large for snum/tnum')
        self.snum[ind] = snum
        self.tnum[ind] = tnum

    def to_struct(self):
        """Attributes as a dict for ``scipy.io.savemat`` (-9999 stands for None)."""
        return {attr: (getattr(self, attr) if getattr(self, attr) is not None else -9999) for attr in self.attrs}
