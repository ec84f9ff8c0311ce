"""The parameters of an ApRES acquisition as the instrument's burst header gives them, with the reference's
attribute names and ``.mat`` layout (``src/impdar/lib/ApresData/ApresHeader.py``).

Quirks of the reference that decide a value are kept and named where they act."""
import re

import numpy as np

from ..ImpdarError import ImpdarError
from .ApresFlags import read_h5_attrs, struct_to_attrs, write_h5_attrs

#: the reference collects header fields in ``np.empty(n).astype(str)``, a '<U32' array: a field keeps 32 characters
FIELD_CHARS = 32


def header_field(header_string, key):
    """The text after the first ``key`` up to the next backslash, or None without the key.  The header is searched
    in its ``str(bytes)`` form, where the carriage return that ends a line reads ``\\r``: a field ends at that
    backslash (reference :198-201; without one ``find`` gives -1 and the slice ends one character early, as there)."""
    if key not in header_string:
        return None
    start = header_string.find(key)
    end = header_string[start:].find('\\')
    return header_string[start + len(key):end + start][:FIELD_CHARS]


def _tuning_word(word, fsysclk):
    """A 32-bit frequency tuning word of the synthesiser in hertz."""
    return word * fsysclk / (2**32)


def _rate_word(word, fsysclk):
    """A 16-bit ramp-rate word in seconds: that many periods of a quarter of the system clock."""
    return word * 4 / fsysclk


# register -> (attribute of its leading digits, attribute of the rest, number of leading digits, word to value):
# 0x0B the ramp's limits (upper, lower), 0x0C its step sizes (decrement, increment), 0x0D its rates (negative, positive)
_RAMP_REGISTERS = {'Reg0B': ('f_stop', 'f0', 8, _tuning_word), 'Reg0C': ('ramp_down_step', 'ramp_up_step', 8, _tuning_word),
                   'Reg0D': ('tstep_down', 'tstep_up', 4, _rate_word)}


class ApresHeader(object):
    """Every attribute of the reference's header (:35-77)."""

    def __init__(self):
        names = ['fsysclk', 'fs', 'fn', 'header_string', 'file_format', 'noDwellHigh', 'noDwellLow',
                 'f0', 'f_stop', 'ramp_up_step', 'ramp_down_step', 'tstep_up', 'tstep_down', 'snum', 'nsteps_DDS',
                 'chirp_length', 'chirp_grad', 'nchirp_samples', 'ramp_dir', 'f1', 'bandwidth', 'fc', 'er', 'ci',
                 'lambdac', 'n_attenuators', 'attenuator1', 'attenuator2', 'tx_ant', 'rx_ant']
        for name in names:          # (in this order, then the two lists: the order of the saved struct's fields)
            setattr(self, name, None)
        self.fsysclk = 1e9          # system clock of the synthesiser
        self.fs = 4e4               # sampling frequency
        self.attrs = names
        self.attr_dims = ['none'] * len(names)

    def read_header(self, fn_apres, max_header_len=2000, offset=0):
        """Keep the first ``max_header_len`` bytes of the file (from ``offset``, the start of a later burst) as
        ``header_string``, in their ``str(bytes)`` form (reference :81-95)."""
        self.fn = fn_apres
        with open(fn_apres, 'rb') as fid:
            fid.seek(offset)
            self.header_string = str(fid.read(max_header_len))

    def get_file_format(self):
        """The format of the file by the keywords of its header (reference :97-117): 5 RMB2 from October 2014 on,
        4 from October 2013, 3 from January 2013, 2 the prototype of November 2012."""
        if 'SW_Issue=' in self.header_string:
            self.file_format = 5
        elif 'SubBursts in burst:' in self.header_string:
            self.file_format = 4
        elif '*** Burst Header ***' in self.header_string:
            self.file_format = 3
        elif 'RADAR TIME' in self.header_string:
            self.file_format = 2
        else:
            raise ImpdarError('Unknown file format - check file')

    def _register(self, k, loc2):
        """The quoted hex digits that follow the k-th ``="``."""
        start = loc2[k] + 2
        return self.header_string[start:start + self.header_string[start:].find('"')]

    def update_parameters(self, fn_apres=None):
        """The chirp's parameters from the DDS registers and the sampling keys of the header (reference :119-228)."""
        if self.header_string is None:
            if fn_apres is None:
                raise TypeError('Must input file name if the header has not been read yet.')
            self.read_header(fn_apres)
        if self.file_format is None:
            self.get_file_format()

        # the k-th 'Reg0' is paired with the k-th '="' of the whole header, whatever key that belongs to (:147-151)
        loc1 = [m.start() for m in re.finditer('Reg0', self.header_string)]
        loc2 = [m.start() for m in re.finditer('="', self.header_string)]
        for k in range(len(loc1)):
            case = self.header_string[loc1[k]:loc2[k]]
            if case == 'Reg01':
                # control function register 2, least significant bit first: bit 18 no-dwell high, bit 17 no-dwell low
                bits = bin(int(self._register(k, loc2), 16))[::-1]
                self.noDwellHigh, self.noDwellLow = int(bits[18]), int(bits[17])
            elif case in _RAMP_REGISTERS:
                first, rest, digits, scale = _RAMP_REGISTERS[case]
                val = self._register(k, loc2)
                setattr(self, rest, scale(int(val[digits:], 16), self.fsysclk))
                setattr(self, first, scale(int(val[:digits], 16), self.fsysclk))

        # The reference compares the field, a string, with the integer 1 (:203-207): never equal, so 80 kHz is never
        # selected and SamplingFreqMode=1 leaves 40 kHz.
        self.fs = header_field(self.header_string, 'SamplingFreqMode=')
        if self.fs == 1:
            self.fs = 8e4
        else:
            self.fs = 4e4

        snum = header_field(self.header_string, 'N_ADC_SAMPLES=')
        self.snum = int('' if snum is None else snum)

        self.nsteps_DDS = round(abs((self.f_stop - self.f0) / self.ramp_up_step))   # abs: the ramp may go down
        self.chirp_length = int(self.nsteps_DDS * self.tstep_up)
        self.nchirp_samples = round(self.chirp_length * self.fs)
        # fewer samples recorded than the chirp has: the chirp is as long as the record
        if self.nchirp_samples > self.snum:
            self.chirp_length = self.snum / self.fs

        self.chirp_grad = 2. * np.pi * (self.ramp_up_step / self.tstep_up)   # rad / s^2
        if self.f_stop > 400e6:
            self.ramp_dir = 'down'
        else:
            self.ramp_dir = 'up'
        if self.noDwellHigh and self.noDwellLow:
            self.ramp_dir = 'upDown'
            self.nchirpsPerPeriod = np.nan

    def write_h5(self, grp):
        """Write every attribute into the subgroup ``ApresHeader`` of an open hdf5 group."""
        write_h5_attrs(grp, 'ApresHeader', self, list(vars(self)), none_as_dataset=False)

    def read_h5(self, grp):
        read_h5_attrs(grp, 'ApresHeader', self)

    def to_matlab(self):
        """Every attribute (``attrs`` and ``attr_dims`` among them, as in the reference :257-261) as a dictionary for
        :func:`scipy.io.savemat`: NaN where one is None."""
        return {att: (getattr(self, att) if getattr(self, att) is not None else np.nan) for att in vars(self)}

    def from_matlab(self, matlab_struct):
        """Take the attributes of ``attrs`` from the struct :func:`scipy.io.loadmat` returns."""
        struct_to_attrs(self, matlab_struct, lambda dim: None if dim == 'none' else dim)
