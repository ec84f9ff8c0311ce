"""Saving of the ApRES containers: the ``.mat`` layout that the reference reads and writes, or hdf5 where ``h5py`` is
installed (behaviour of ``src/impdar/lib/ApresData/_ApresDataSaving.py``)."""
import os

import numpy as np
from scipy.io import savemat

from .ApresFlags import ApresFlags, _h5py
from .ApresHeader import ApresHeader

# Data that came in as integers and holds NaNs now cannot go back to its dtype: the float type written instead
_NAN_FALLBACK = ((np.float16, (int, np.int8, np.int16)), (np.float32, (np.int32,)), (np.float64, (np.int64,)))


def save(self, fn):
    """Write the object to ``fn``: ``.mat``, or ``.h5`` / ``.hdf5``; another extension is a ``ValueError``."""
    writers = {'.mat': save_mat, '.h5': save_h5, '.hdf5': save_h5}
    ext = os.path.splitext(fn)[1]
    if ext not in writers:
        raise ValueError('File extension choices are .h5 and .mat (legacy)')
    return writers[ext](self, fn)


def _stored_dtype(data, wanted):
    """The dtype ``data`` is written in when the object remembers ``wanted`` as the dtype it was loaded with."""
    if np.any(np.isnan(data)):
        for fallback, integers in _NAN_FALLBACK:
            if wanted in integers:
                print('Warning: new file is %s rather than ' % np.dtype(fallback).name, wanted, ' since we now have NaNs')
                return fallback
    return wanted


def save_mat(self, fn):
    """One variable per guaranteed attribute (0 where it is None, so that Matlab finds every name), one per optional
    attribute that is set, and the structs ``flags`` and ``header`` (defaults where the object's are None).  An object
    with a header has its ``data`` cast back to ``data_dtype`` where that differs."""
    present = [a for a in self.attrs_optional if getattr(self, a, None) is not None]
    mat = {a: getattr(self, a) for a in present}
    mat.update((a, 0 if getattr(self, a) is None else getattr(self, a)) for a in self.attrs_guaranteed)
    mat['flags'] = (self.flags if self.flags is not None else ApresFlags()).to_matlab()
    if 'header' in vars(self):
        mat['header'] = (self.header if self.header is not None else ApresHeader()).to_matlab()
        wanted = getattr(self, 'data_dtype', None)
        if wanted is not None and wanted != mat['data'].dtype:
            mat['data'] = mat['data'].astype(_stored_dtype(mat['data'], wanted))
    savemat(fn, mat)


def save_h5(self, fn, groupname='dat'):
    """Write the object as the group ``groupname`` of a new hdf5 file."""
    with _h5py().File(fn, 'w') as f:
        save_as_h5_group(self, f, groupname=groupname)


def save_as_h5_group(self, h5_file_descriptor, groupname='dat'):
    """Into a new group of an open hdf5 file or group: arrays of more than one element as datasets (object arrays in
    ``data_dtype``, float32 without one), everything else as attributes, an empty float32 attribute for None; string
    values of guaranteed attributes are left out; flags and header as subgroups."""
    h5py = _h5py()
    grp = h5_file_descriptor.create_group(groupname)
    empty = h5py.Empty(dtype=np.dtype('f'))
    fallback = getattr(self, 'data_dtype', None) or np.dtype('f')
    for attr in list(self.attrs_guaranteed) + list(self.attrs_optional):
        val = getattr(self, attr, None)
        if val is None:
            grp.attrs.create(attr, empty)
        elif type(val) is str and attr in self.attrs_guaranteed:
            continue
        elif hasattr(val, 'shape') and any(s != 1 for s in val.shape):
            grp.create_dataset(attr, data=val, dtype=fallback if val.dtype == 'O' else val.dtype)
        else:
            grp.attrs.create(attr, val)
    (self.flags if self.flags is not None else ApresFlags()).write_h5(grp)
    header = getattr(self, 'header', None)
    (header if header is not None else ApresHeader()).write_h5(grp)
