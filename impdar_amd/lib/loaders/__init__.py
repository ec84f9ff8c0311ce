"""Instrument files in (reference ``src/impdar/lib/load/__init__.py``): ``load(filetype, fns_in)`` for GSSI ``.DZT``,
pulseEKKO ``.DT1``, RAMAC ``.rd3`` and Tek ``.DAT`` files besides ImpDAR ``.mat``, and ``load_and_exit``, which writes
each as ``*_raw.mat`` -- what ``impdar load`` runs and ``impproc`` then reads.

``resident=None`` decodes on the host: ``dat.data`` is the reference's array, in its dtype, and no GPU is needed.
``resident='float32' | 'float64'`` sends the file's bytes up as they are and decodes them in HBM (``impdar_amd.rawload``):
``dat._dev`` holds the radargram, ``dat.data`` is None and ``dat.data_dtype`` the reference's dtype, as if ``to_device()``
had been called on the widened array.

The reference's other readers need h5py, segyio or netCDF4, or have no sample files to hold this package to; they are
named in ``NOT_PROVIDED`` and raise ``NotImplementedError``.  ``t_srs`` / ``s_srs`` are accepted and, as in the reference
without GDAL, have no effect.
"""
import os

from ..RadarData import RadarData
from . import _decode, load_gssi, load_pulse_ekko, load_ramac, load_tek

FILETYPE_OPTIONS = ['mat', 'pe', 'gssi', 'ramac', 'tek']

NOT_PROVIDED = {'gprMax': 'needs h5py', 'bsi': 'needs h5py', 'UoA_mat': 'needs h5py', 'UoA_h5': 'needs h5py',
                'segy': 'needs segyio', 'mcords_nc': 'needs netCDF4', 'mcords_mat': 'not provided',
                'stomat': 'not provided', 'gecko': 'not provided', 'delores': 'not provided', 'osu': 'not provided',
                'apres': 'not provided (ApRES files: impdar_amd.lib.ApresData, apdar)'}


def load(filetype, fns_in, channel=1, t_srs=None, s_srs=None, resident=None, *args, **kwargs):
    """A list of RadarData, one per file of ``fns_in``."""
    if not isinstance(fns_in, (list, tuple)):
        fns_in = [fns_in]
    if filetype == 'gssi':
        return [load_gssi._read(fn, resident=resident) for fn in fns_in]
    if filetype == 'pe':
        dat = []
        for fn in fns_in:
            if os.path.splitext(fn)[-1] == '.GPZ':
                raise NotImplementedError('pulseEKKO project files (.GPZ) are not provided; unpack the .HD and .DT1 files')
            try:
                dat.append(load_pulse_ekko._read(fn, resident=resident))
            except IOError:
                print('Could not load ', fn, 'as a Pulse Ekko file.')
        return dat
    if filetype == 'ramac':
        return [load_ramac._read(fn, resident=resident) for fn in fns_in]
    if filetype == 'tek':
        return [load_tek._read(fn, resident=resident) for fn in fns_in]
    if filetype == 'mat':
        dat = [RadarData(fn) for fn in fns_in]
        if resident is not None:
            for d in dat:
                d.data = d.data.astype(_decode.RESIDENT_DTYPES[resident])
                d.to_device()
        return dat
    if filetype in NOT_PROVIDED:
        raise NotImplementedError('filetype %s is not read by this package: %s' % (filetype, NOT_PROVIDED[filetype]))
    raise ValueError('Unrecognized filetype')


def load_and_exit(filetype, fns_in, channel=1, t_srs=None, s_srs=None, o=None, *args, **kwargs):
    """Load the files and write each as a StoDeep/ImpDAR ``.mat``: to ``o`` (one file), into the folder ``o``, or beside
    the input as ``<name>_raw.mat``."""
    if not isinstance(fns_in, (list, tuple)):
        fns_in = [fns_in]
    kwargs.pop('resident', None)          # what is written is the host array in the file's own dtype
    if (len(fns_in) > 1) and (o is not None) and (not os.path.isdir(o)):
        raise FileNotFoundError('The output directory does not exist')
    for fn in fns_in:
        _save(load(filetype, fn, channel=channel, t_srs=t_srs, s_srs=s_srs, **kwargs), outpath=o)


def _raw_name(rd):
    return os.path.splitext(rd.fn)[0] + '_raw.mat'


def _save(rd_list, outpath=None):
    if outpath is None:
        for rd in rd_list:
            rd.save(_raw_name(rd))
    elif len(rd_list) > 1:
        for rd in rd_list:
            rd.save(os.path.join(outpath, os.path.split(_raw_name(rd))[-1]))
    elif os.path.isdir(outpath):
        rd_list[0].save(outpath + _raw_name(rd_list[0]))      # (the reference joins the two without a separator)
    else:
        rd_list[0].save(outpath)
