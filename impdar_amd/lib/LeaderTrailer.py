"""StoInterpret's ``lt`` structure, kept so that picked files round-trip.  Restates the reference's
``src/impdar/lib/LeaderTrailer.py:13-52`` and the ``Crop`` record it embeds (``src/impdar/lib/Crop.py:13-53``) in
this project's own text."""
import numpy as np


class Crop(object):
    """The extent of the data the picks were made on: ``tnum``, ``maxsnum`` and the travel-time range."""

    attrs = ['tnum', 'maxsnum', 'mintt', 'maxtt']

    def __init__(self, radardata):
        self.tnum = radardata.tnum
        self.maxsnum = radardata.snum
        self.mintt = np.min(radardata.travel_time)
        self.maxtt = np.max(radardata.travel_time)

    def to_struct(self):
        return {attr: getattr(self, attr) for attr in self.attrs}


class LeaderTrailer(object):
    """``llength``, ``tlength`` and ``ltmatrix`` (all 0 unless loaded) and the crop record of the radargram."""

    attrs = ['llength', 'tlength', 'ltmatrix']

    def __init__(self, radardata, lt_struct=None):
        for attr in self.attrs:
            setattr(self, attr, lt_struct[0][0][attr] if lt_struct is not None else 0)
        self.crop = Crop(radardata)

    def to_struct(self):
        """Attributes as a dict for ``scipy.io.savemat`` (0 stands for None)."""
        mat = {attr: (getattr(self, attr) if getattr(self, attr) is not None else 0) for attr in self.attrs}
        mat['crop'] = self.crop.to_struct()
        return mat
