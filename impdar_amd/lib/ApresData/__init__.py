"""The ApRES containers with the reference's names, attribute lists, messages and file formats
(``src/impdar/lib/ApresData/__init__.py``): :class:`ApresData` for one acquisition, :class:`ApresTimeDiff` for a pair,
:class:`ApresQuadPol` for a quad-polarized set.  Their processing methods are the functions of ``impdar_amd.apres`` and
``impdar_amd.quadpol``; ``save`` is ``_ApresDataSaving.save``; the loaders are ``load_apres``, ``load_time_diff`` and
``load_quadpol`` beside this file.

A raw acquisition read from the instrument's ``.DAT`` files keeps the counts as they were read (2 bytes a sample)
beside the scale that makes volts of them.  ``ApresData.data`` is then produced on first read by the reference's NumPy
expression and cached; range conversion on such an object uploads the counts and widens them in HBM
(``apres.decode_dev``), which leaves the same bits.  Assigning ``data`` drops the counts.

hdf5 files need ``h5py``, netCDF files ``netCDF4``: an ``ImportError`` says so where they are missing."""
import datetime
import os

import numpy as np
from scipy.io import loadmat

from ... import apres as _apres
from ... import quadpol as _quadpol
from ..ImpdarError import ImpdarError
from .ApresFlags import ApresFlags, QuadPolFlags, TimeDiffFlags, _h5py
from .ApresHeader import ApresHeader
from ._ApresDataSaving import save as _save

FILETYPE_OPTIONS = ['DAT', 'dat', 'mat', 'h5', 'nc']

# the reference's messages carry the indentation of their continuation lines (:182-183 and the like)
_ILL = '{:s} is {:s}. ' + ' ' * 20 + 'It appears that this is an ill-defined {:s} object'
_MSG_TIMEDIFF_FILE = 'ApresTimeDiff() is looking for an .h5 or .mat file ' + ' ' * 30 + 'saved as an Apdar object.'


def counts_to_volts(counts, divisor=1.):
    """The reference's decode of an instrument's counts (``load_apres.py:392-395``)."""
    volts = counts.astype(float) * 2.5 / 2**16.
    if divisor != 1:
        volts /= divisor
    return volts


def _from_mat(self, mat, flatten_data):
    """The reference's scalar / flatten rules for what ``loadmat`` returns (:141-159): (1, 1) to a scalar, a row or a
    column to a vector (``data`` of an acquisition keeps its shape), an optional attribute that is absent to None."""
    def take(attr, flatten):
        if mat[attr].shape == (1, 1):
            setattr(self, attr, mat[attr][0][0])
        elif (mat[attr].shape[0] == 1 or mat[attr].shape[1] == 1) and flatten:
            setattr(self, attr, mat[attr].flatten())
        else:
            setattr(self, attr, mat[attr])
    for attr in self.attrs_guaranteed:
        take(attr, flatten_data or attr != 'data')
    for attr in self.attrs_optional:
        if attr in mat:
            take(attr, True)
        else:
            setattr(self, attr, None)


def _from_h5(self, fn, flag_class, groups, with_header=True):
    h5py = _h5py()
    with h5py.File(fn, 'r') as fin:
        grp = fin['dat']
        for attr in grp.keys():
            if attr in groups:
                continue
            val = grp[attr][:]
            setattr(self, attr, None if isinstance(val, h5py.Empty) else val)
        for attr in grp.attrs.keys():
            val = grp.attrs[attr]
            setattr(self, attr, None if isinstance(val, h5py.Empty) else val)
        self.flags = flag_class()
        self.flags.read_h5(grp)
        if with_header:
            self.header = ApresHeader()
            self.header.read_h5(grp)


def _check(self, kind, optional):
    for attr in self.attrs_guaranteed:
        if not hasattr(self, attr):
            raise ImpdarError(_ILL.format(attr, 'missing', kind))
        if getattr(self, attr) is None:
            raise ImpdarError(_ILL.format(attr, 'None', kind))
    if optional:
        for attr in self.attrs_optional:
            if not hasattr(self, attr):
                raise ImpdarError(_ILL.format(attr, 'missing', kind))


def _datetime(self):
    return np.array([datetime.datetime.fromordinal(int(dd)) + datetime.timedelta(days=dd % 1) - datetime.timedelta(days=366)
                     for dd in self.decday], dtype=np.datetime64)


class ApresData(object):
    """One ApRES acquisition: ``data`` is (bnum, cnum, snum), bursts by chirps by samples; per-burst records
    (``decday``, ``lat``, ``temperature1`` ...) have one entry per burst; what belongs to the instrument's settings is
    in ``header``, what has been done to the data in ``flags``."""
    #: Attributes that every ApresData object has, none of them None.
    attrs_guaranteed = ['data', 'decday', 'dt', 'snum', 'cnum', 'bnum', 'chirp_num', 'chirp_att', 'chirp_time',
                        'travel_time', 'frequencies']
    #: Attributes that may be None.
    attrs_optional = ['lat', 'long', 'x_coord', 'y_coord', 'elev', 'temperature1', 'temperature2', 'battery_voltage',
                      'Rcoarse', 'uncertainty']

    apres_range = _apres.apres_range
    stacking = _apres.stacking
    phase_uncertainty = _apres.phase_uncertainty
    single_processing = _apres.single_processing
    save = _save

    def __init__(self, fn):
        if fn is None:
            # the documented empty object: data (bnum, cnum, snum); decday, lat, long, the temperatures and the battery
            # voltage per burst; chirp_num, chirp_att, chirp_time (bnum, cnum); travel_time (microseconds), frequencies
            # and, after range conversion, Rcoarse per sample; dt in seconds
            for name in self.attrs_guaranteed + self.attrs_optional + ['data_dtype']:
                setattr(self, name, None)
            self.flags = ApresFlags()
            self.header = ApresHeader()
            return

        if os.path.splitext(fn)[1] == '.h5':
            _from_h5(self, fn, ApresFlags, ['ApresFlags', 'ApresHeader'])
        else:
            mat = loadmat(fn)
            _from_mat(self, mat, flatten_data=False)
            self.data_dtype = self.data.dtype
            self.flags = ApresFlags()
            self.flags.from_matlab(mat['flags'])
            self.header = ApresHeader()
            self.header.from_matlab(mat['header'])
        self.fn = fn
        self.check_attrs()

    # ---- data: an array, or the instrument's counts with their scale until somebody reads the volts
    @property
    def data(self):
        if '_data' not in self.__dict__:
            raise AttributeError("'ApresData' object has no attribute 'data'")
        held = self.__dict__['_data']
        counts = self.__dict__.get('_counts')
        if held is None and counts is not None:
            held = self.__dict__['_data'] = counts_to_volts(counts, self.__dict__['_counts_divisor'])
        return held

    @data.setter
    def data(self, value):
        self.__dict__['_data'] = value
        self.__dict__['_counts'] = None
        self.__dict__['_counts_divisor'] = 1.

    @data.deleter
    def data(self):
        for k in ('_data', '_counts', '_counts_divisor'):
            self.__dict__.pop(k, None)

    def set_counts(self, counts, divisor=1.):
        """Hold ``counts`` (little-endian uint16 or uint32 of the data's shape) in place of the data: the volts are
        ``counts_to_volts(counts, divisor)``, made when ``data`` is first read."""
        self.data = None
        self.__dict__['_counts'] = counts
        self.__dict__['_counts_divisor'] = float(divisor)

    def raw_counts(self):
        """``(counts, divisor)`` while the counts are held, else None (read by ``apres.apres_range`` and
        ``apres.chain``)."""
        counts = self.__dict__.get('_counts')
        return None if counts is None else (counts, self.__dict__['_counts_divisor'])

    def check_attrs(self):
        """Raise ``ImpdarError`` if a guaranteed attribute is missing or None or an optional one is missing."""
        _check(self, 'ApresData', optional=True)
        if not hasattr(self, 'data_dtype') or self.data_dtype is None:
            self.data_dtype = np.dtype(float) if self.raw_counts() is not None else self.data.dtype

    @property
    def datetime(self):
        """The time of each burst as ``numpy.datetime64``."""
        return _datetime(self)


class ApresTimeDiff(object):
    """Two acquisitions of one site, stacked and converted to range, for differencing in time."""
    attrs_guaranteed = ['data', 'data2', 'decday', 'decday2', 'dt', 'snum', 'range', 'fn1', 'fn2', 'fn']
    attrs_optional = ['lat', 'lat2', 'long', 'long2', 'x_coord', 'x_coord2', 'y_coord', 'y_coord2', 'elev', 'elev2',
                      'unc1', 'unc2', 'ds', 'co', 'phi', 'w', 'w_err', 'w_0', 'eps_zz', 'bed']

    phase_diff = _apres.phase_diff
    phase_unwrap = _apres.phase_unwrap
    range_diff = _apres.range_diff
    strain_rate = _apres.strain_rate
    bed_pick = _apres.bed_pick
    save = _save

    def __init__(self, fn):
        if fn is None:
            # the documented empty object: the two profiles data and data2 (snum,) on one range axis, what belongs to
            # the second acquisition under the first's name with a 2, the products ds, co, w of the differencing
            for name in ('snum', 'data', 'data2', 'dt', 'decday', 'decday2', 'lat', 'lat2', 'long', 'long2', 'range', 'x_coord',
                         'x_coord2', 'y_coord', 'y_coord2', 'elev', 'elev2', 'ds', 'co', 'w', 'data_dtype'):
                setattr(self, name, None)
            self.flags = TimeDiffFlags()
            self.header = ApresHeader()
            return

        if os.path.splitext(fn)[1] == '.h5':
            _from_h5(self, fn, TimeDiffFlags, ['TimeDiffFlags', 'ApresHeader'])
        elif os.path.splitext(fn)[1] == '.mat':
            mat = loadmat(fn)
            _from_mat(self, mat, flatten_data=True)
            self.data_dtype = self.data.dtype
            self.flags = TimeDiffFlags()
            self.flags.from_matlab(mat['flags'])
            self.header = ApresHeader()
            self.header.from_matlab(mat['header'])
        else:
            raise ImportError(_MSG_TIMEDIFF_FILE)
        self.fn = fn
        self.check_attrs()

    def check_attrs(self):
        """Raise ``ImpdarError`` if a guaranteed attribute is missing or None."""
        _check(self, 'ApresTimeDiff', optional=False)
        if not hasattr(self, 'data_dtype') or self.data_dtype is None:
            self.data_dtype = self.data.dtype


class ApresQuadPol(object):
    """A quad-polarized acquisition: the four stacked complex profiles ``shh``, ``shv``, ``svh``, ``svv`` on one
    ``range`` axis (``data`` is a copy of ``shh``, so that ``save`` finds one)."""
    attrs_guaranteed = ['data', 'shh', 'shv', 'svh', 'svv', 'range', 'decday', 'dt', 'snum', 'travel_time']
    attrs_optional = ['lat', 'long', 'x_coord', 'y_coord', 'elev', 'ant_sep', 'ant_azi', 'thetas', 'HH', 'HV', 'VH',
                      'VV', 'chhvv', 'dphi_dz', 'cpe', 'cpe_idxs', 'chhvv_cpe', 'dphi_dz_cpe', 'phi']

    rotational_transform = _quadpol.rotational_transform
    coherence2d = _quadpol.coherence2d
    phase_gradient2d = _quadpol.phase_gradient2d
    find_cpe = _quadpol.find_cpe
    phase_gradient_to_fabric = _quadpol.phase_gradient_to_fabric
    save = _save

    def __init__(self, fn):
        if fn is None:
            # the documented empty object (no header until a loader gives it one)
            for name in ('data', 'snum', 'dt', 'shh', 'shv', 'svh', 'svv', 'travel_time', 'decday', 'lat', 'long', 'x_coord',
                         'y_coord', 'elev', 'data_dtype'):
                setattr(self, name, None)
            self.flags = QuadPolFlags()
            return

        if os.path.splitext(fn)[1] == '.h5':
            _from_h5(self, fn, QuadPolFlags, ['QuadPolFlags'], with_header=False)
        else:
            mat = loadmat(fn)
            _from_mat(self, mat, flatten_data=True)
            self.data_dtype = self.shh.dtype
            self.flags = QuadPolFlags()
            self.flags.from_matlab(mat['flags'])
            self.header = ApresHeader()
            self.header.from_matlab(mat['header'])
        self.fn = fn
        self.check_attrs()

    def check_attrs(self):
        """Raise ``ImpdarError`` if a guaranteed attribute is missing or None."""
        _check(self, 'ApresQuadPol', optional=False)
        if not hasattr(self, 'data_dtype') or self.data_dtype is None:
            self.data_dtype = self.shh.dtype

    @property
    def datetime(self):
        """The time of the acquisition as ``numpy.datetime64``."""
        return _datetime(self)


from . import load_apres, load_quadpol, load_time_diff   # noqa: E402,F401  (the loaders import the classes above)
