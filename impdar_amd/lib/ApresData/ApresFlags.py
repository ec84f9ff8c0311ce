"""Flags that record which processing steps an ApRES object has been through, with the reference's names,
defaults and ``.mat`` layout (``src/impdar/lib/ApresData/ApresFlags.py``): :class:`ApresFlags` for one acquisition,
:class:`TimeDiffFlags` for a pair, :class:`QuadPolFlags` for a quad-polarized set.  The processing functions of
``impdar_amd.apres`` and ``impdar_amd.quadpol`` read and write their attributes only."""
import numpy as np


def _h5py():
    try:
        import h5py
    except ImportError:
        raise ImportError('Need the h5py library to read and write h5 files.')
    return h5py


def write_h5_attrs(grp, name, obj, attrs, none_as_dataset):
    """The attributes ``attrs`` of ``obj`` as hdf5 attributes of a new subgroup ``name``: arrays as float32, None as an
    empty float32 (a dataset of that name for the flags, an attribute for the header, as the reference writes them)."""
    h5py = _h5py()
    subgrp = grp.create_group(name)
    for attr in attrs:
        val = getattr(obj, attr)
        if val is None:
            (subgrp if none_as_dataset else subgrp.attrs)[attr] = h5py.Empty('f')
        else:
            subgrp.attrs[attr] = val.astype('f') if hasattr(val, 'dtype') else val


def read_h5_attrs(grp, name, obj):
    """Every hdf5 attribute of subgroup ``name`` onto ``obj``, an empty one as None."""
    h5py = _h5py()
    for attr, val in grp[name].attrs.items():
        setattr(obj, attr, None if isinstance(val, h5py.Empty) else val)


def struct_to_attrs(obj, matlab_struct, vector_or_none):
    """The fields ``obj.attrs`` of a struct from :func:`scipy.io.loadmat` onto ``obj``.  A field that should be a vector
    (``vector_or_none`` gives its length) and comes back with one element -- a scalar that was padded lazily --
    becomes the preallocated zeros."""
    for attr, dim in zip(obj.attrs, obj.attr_dims):
        val = matlab_struct[attr][0][0][0]
        length = vector_or_none(dim)
        setattr(obj, attr, np.zeros((length, )) if length is not None and val.shape[0] == 1 else val)


class _Flags(object):
    """What the three classes share: ``attrs`` names what is saved, ``attr_dims`` the length of those that are
    vectors (None for scalars)."""
    h5_group = 'ApresFlags'

    def write_h5(self, grp):
        """Write the flags into a subgroup of an open hdf5 group."""
        write_h5_attrs(grp, self.h5_group, self, self.attrs, none_as_dataset=True)

    def read_h5(self, grp):
        read_h5_attrs(grp, self.h5_group, self)

    def to_matlab(self):
        """The flags as a dictionary for :func:`scipy.io.savemat`: NaN where a flag is None."""
        return {att: (getattr(self, att) if getattr(self, att) is not None else np.nan) for att in self.attrs}

    def from_matlab(self, matlab_struct):
        """Take the flags from the struct :func:`scipy.io.loadmat` returns."""
        struct_to_attrs(self, matlab_struct, lambda dim: dim)


class ApresFlags(_Flags):
    """``file_read_code``, ``range`` (the maximum range of the conversion, 0 before it), ``stack`` (chirps stacked)
    and ``uncertainty`` (reference :30-36)."""

    def __init__(self):
        self.file_read_code = None
        self.range = 0
        self.stack = 0
        self.uncertainty = False
        self.attrs = ['file_read_code', 'range', 'stack', 'uncertainty']
        self.attr_dims = [None, None, None, None]


class TimeDiffFlags(_Flags):
    """``file_read_code``, ``phase_diff``, ``unwrap``, ``strain`` and ``bed_pick`` (reference :98-105)."""

    def __init__(self):
        self.file_read_code = None
        self.phase_diff = False
        self.unwrap = False
        self.strain = np.zeros((2,))
        self.bed_pick = False
        self.attrs = ['file_read_code', 'phase_diff', 'unwrap', 'strain', 'bed_pick']
        self.attr_dims = [None, None, None, 2, None]


class QuadPolFlags(_Flags):
    """``rotation``, ``coherence``, ``phasegradient`` and ``cpe`` (reference :164-170; ``cpe`` starts True there)."""
    h5_group = 'QuadPolFlags'

    def __init__(self):
        self.rotation = np.zeros((2,))
        self.coherence = np.zeros((3,))
        self.phasegradient = False
        self.cpe = True
        self.attrs = ['rotation', 'coherence', 'phasegradient', 'cpe']
        self.attr_dims = [2, 3, None, None]

    def to_matlab(self):
        """No flag of this class is ever None: the values as they are (reference :198-202)."""
        return {att: getattr(self, att) for att in self.attrs}
