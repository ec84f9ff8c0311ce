"""The band-pass / re-spacing / migration chain of ImpDAR's multi-step driver.

Mirrors the part of the reference's ``src/impdar/lib/process.py`` that leads up to a migration, in the
reference's order (``:72-197``): ``vbp=(low, high)`` -> ``dat.vertical_band_pass`` (``:151-154``),
``interp=(spacing, gps_fn)`` -> ``gpslib.interp`` = ``dat.constant_space`` when no GPS file is given
(``:178-180``), ``migrate=X`` -> ``dat.migrate(mtype='stolt')`` whatever ``X`` is (``:190-193`` -- the string
given on the command line is ignored by the reference, and so it is here), and ``ahfilt=W`` ->
``dat.hfilt(ftype='adaptive', window_size=W)`` after the band pass (``:160-162``), and ``denoise=(V, H)`` ->
``dat.denoise(V, H)`` (Wiener) after the horizontal filter and before the re-spacing (``:121-126``, ``:175-178``).
When more than one of the steps is requested on a float radargram it is uploaded once and stays in HBM until the
last step is done.
``process_and_exit`` loads, processes and saves with the reference's file naming (``:30-70``, ``:274-295``).
The other steps of that driver (crop, nmo, the ``hfilt=(first, last)`` mean-trace filter, restack, reverse)
are rejected here.  ``RadarData.hfilt(ftype='hfilt')``, ``RadarData.crop``, ``RadarData.nmo``, ``RadarData.hcrop``,
``RadarData.restack`` and ``RadarData.reverse`` exist and run on their own (``impproc hfilt / crop / nmo / hcrop /
restack / rev``, or ``dat.to_device()`` and the methods for a resident chain), but
accepting them here would change what ``process`` has always answered to them.
"""
import os

import numpy as np

from .load import load

_OUT_OF_SCOPE = ('rev', 'hfilt', 'nmo', 'crop', 'hcrop', 'restack')


def _window(ahfilt):
    """``-ahfilt W`` arrives from argparse as a 1-element list (``nargs=1``); the reference hands that list on
    to ``window_size // 2`` and fails.  An int or a 1-element list is accepted here."""
    if isinstance(ahfilt, (list, tuple, np.ndarray)):
        if len(ahfilt) != 1:
            raise ValueError('ahfilt must be one window size (number of traces)')
        ahfilt = ahfilt[0]
    if isinstance(ahfilt, (bool, np.bool_)) or int(ahfilt) != ahfilt:
        raise TypeError('ahfilt must be an integer number of traces')
    return int(ahfilt)


def process(RadarDataList, interp=None, vbp=None, ahfilt=None, denoise=None, migrate=None, **kwargs):
    """Returns True if something was done (reference ``process.py:72-197``).  ``hfilt=(first, last)`` stays
    rejected (run ``RadarData.hfilt`` or ``impproc hfilt`` for it)."""
    for name in _OUT_OF_SCOPE:
        if kwargs.get(name) not in (None, False):
            raise NotImplementedError('processing step %r is not part of the MI355X migration engine; '
                                      'run it with the reference ImpDAR first' % name)
    if denoise is not None:
        try:
            ok = type(denoise[0]) is int and type(denoise[1]) is int     # the reference's check (:121-126)
        except (TypeError, IndexError):
            ok = False
        if not ok:
            raise ValueError('Denoise must be two integers giving vertical and horizontal window sizes')
    if vbp is not None:
        if not hasattr(vbp, '__iter__'):
            raise TypeError('vbp must be a tuple with first two elements [low] [high] MHz')
    if interp is not None:
        try:
            float(interp[0])
            interp[1]
        except (ValueError, TypeError, IndexError):
            raise ValueError('interp must be a target spacing (float) then a gps filename')
        if interp[1] is not None:
            raise NotImplementedError('process() does not take a gps filename for interp: attach the track with '
                                      'gpslib.interp / `impproc geolocate` first')
    if ahfilt is False or (isinstance(ahfilt, (int, np.integer)) and ahfilt == 0):
        ahfilt = None                 # the reference's `if ahfilt:`
    if ahfilt is not None:
        ahfilt = _window(ahfilt)
    steps = sum(x is not None for x in (vbp, ahfilt, denoise, interp, migrate))
    if steps == 0:
        return False
    for dat in RadarDataList:
        resident = steps > 1 and np.asarray(dat.data).dtype in (np.float32, np.float64)
        if resident:
            dat.to_device()
        try:
            if vbp is not None:
                dat.vertical_band_pass(*vbp)
            if ahfilt is not None:
                dat.hfilt(ftype='adaptive', window_size=ahfilt)
            if denoise is not None:
                dat.denoise(*denoise)
            if interp is not None:
                dat.constant_space(float(interp[0]))
            if migrate is not None:
                dat.migrate(mtype='stolt')
        finally:
            if resident:
                dat.from_device()
    return True


def _save(rd_list, outpath=None, cat=False):
    if outpath is not None:
        if len(rd_list) > 1:
            for rd in rd_list:
                bn = os.path.split(os.path.splitext(rd.fn)[0])[1]
                if bn[-4:] == '_raw':
                    bn = bn[:-4]
                rd.save(os.path.join(outpath, bn + '_proc.mat'))
        else:
            rd_list[0].save(outpath)
    else:
        for rd in rd_list:
            bn = os.path.splitext(rd.fn)[0]
            if bn[-4:] == '_raw':
                bn = bn[:-4]
            rd.save(bn + ('.mat' if cat else '_proc.mat'))


def process_and_exit(fn, cat=False, filetype='mat', o=None, **kwargs):
    if cat:
        raise NotImplementedError('concatenation is not part of the MI355X migration engine')
    radar_data = load(filetype, fn)
    processed = process(radar_data, **kwargs)
    if not processed:
        print('No processing steps performed. Not saving!')
    else:
        _save(radar_data, outpath=o, cat=cat)
