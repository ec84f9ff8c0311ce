"""The parameters of a picking session: the frequency of the layers looked for and the window sizes that follow
from it.  Restates the reference's ``src/impdar/lib/PickParameters.py:11-116`` (names, defaults, the ``.mat``
struct) in this project's own text."""


class PickParameters(object):
    """``freq`` (MHz, default 4), ``dt``, and what ``freq_update`` derives: ``plength`` (samples of the packet that is
    searched), ``FWW`` (samples of its centre portion) and ``scst`` (offset of that portion); ``pol`` (1 or -1, the
    polarity of the centre peak); ``apickthresh``, ``apickflag`` and ``addpicktype`` are StoDeep's and unused."""

    attrs = ['apickthresh', 'freq', 'dt', 'plength', 'FWW', 'scst', 'pol', 'apickflag', 'addpicktype']

    def __init__(self, radardata, pickparams_struct=None):
        if pickparams_struct is not None:
            for attr in self.attrs:
                setattr(self, attr, pickparams_struct[0][0][attr][0][0][0][0])
        else:
            self.freq = 4
            self.apickthresh = 10
            self.dt = radardata.dt
            self.pol = 1
            self.apickflag = 1
            self.addpicktype = 'zero'
        self.radardata = radardata
        self.freq_update(self.freq)

    def freq_update(self, freq):
        """Set the frequency and the window sizes with it: ``plength`` is one sample short of two periods (3 at
        the least), ``FWW`` two thirds of a period made odd, ``scst`` what centres the one in the other.  A packet
        longer than the trace is clamped to it, ``FWW`` to half of it; ``scst`` stays as computed."""
        self.freq = freq
        period = 1. / (self.freq * 1.0e6 * self.radardata.dt)
        self.plength = 2 * int(round(period)) - 1
        if self.plength < 3:
            print('Warning: high freq compared to sampling rate. Forcing a minimum plength')
            self.plength = 3
        self.FWW = int(round(2. / 3. * period))
        if self.FWW % 2 == 0:
            self.FWW += 1
        self.scst = (self.plength - self.FWW) // 2
        if self.plength > self.radardata.snum and self.radardata.snum >= 3:
            self.plength = self.radardata.snum
            self.FWW = self.radardata.snum // 2
            if self.FWW % 2 == 0:
                self.FWW += 1

    def to_struct(self):
        """Attributes as a dict for ``scipy.io.savemat`` (0 stands for None)."""
        return {attr: (getattr(self, attr) if getattr(self, attr) is not None else 0) for attr in self.attrs}
