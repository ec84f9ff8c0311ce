"""RAMAC / Mala: ``.rd3`` samples, ``.rad`` text header, optional ``.cor`` positions (reference
``src/impdar/lib/load/load_ramac.py``).  The ``.rd3`` file is ``snum`` int16 per trace and nothing else."""
import datetime
import os
import struct

import numpy as np
from scipy.interpolate import interp1d

from ... import rawload
from ..RadarData import RadarData
from ..gpslib import conversions_enabled, nmea_info
from . import _decode

_COR_FIELDS = [('trace_num', int), ('date', 'S10'), ('time', 'S8'), ('lat', float), ('north', 'S1'), ('lon', float),
               ('east', 'S1'), ('elev', float), ('el_unit', 'S1'), ('pdop', float)]


def _file_names(ramac_fn):
    """A base name, the ``.rad`` header or the ``.rd3`` data file -> (header, data, positions)."""
    if len(ramac_fn) > 4 and ramac_fn[-4:] in ('.rd3', '.rad'):
        stem = ramac_fn[:-4]
    else:
        stem = ramac_fn
    return stem + '.rad', stem + '.rd3', stem + '.cor'


def _value(line, skip):
    return line.rstrip('\n')[skip:]


def _positions(dat, gps_fn):
    """Per-trace time, latitude, longitude and elevation from the sparse fixes of a ``.cor`` file."""
    cor = np.genfromtxt(gps_fn, dtype=_COR_FIELDS)
    stamps = np.array([d + b'T' + t for d, t in zip(cor['date'], cor['time'])], dtype=np.datetime64)
    since = stamps - np.array(datetime.datetime(1, 1, 1, 0, 0, 0), dtype=np.datetime64)
    south, west = cor['north'] != b'N', cor['east'] != b'E'
    cor['lat'][south] = -1 * cor['lat'][south]
    cor['lon'][west] = -1 * cor['lon'][west]

    def onto_traces(values):
        return interp1d(cor['trace_num'], values, fill_value='extrapolate')(dat.trace_num)

    dat.decday = onto_traces(since) / (24. * 60. * 60.)
    dat.lat = onto_traces(cor['lat'])
    dat.long = onto_traces(cor['lon'])
    dat.elev = onto_traces(cor['elev'])
    info = nmea_info()
    info.time = dat.decday
    info.lat = dat.lat
    info.lon = dat.long
    info.elev = dat.elev
    if conversions_enabled:
        info.get_utm()
        info.get_dist()
        dat.x_coord, dat.y_coord, dat.dist = info.x, info.y, info.dist
    else:
        dat.x_coord = dat.long
        dat.y_coord = dat.lat
        dat.dist = np.sqrt(dat.x_coord ** 2.0 + dat.y_coord ** 2.0) / 1000.0


def _read(ramac_fn, resident=None):
    dat = RadarData(None)
    header_fn, data_fn, gps_fn = _file_names(ramac_fn)
    dat.fn = data_fn
    with open(header_fn) as f:
        header = f.readlines()
    dat.chan = ramac_fn[-5]
    snum = int(_value(header[0], 8))                     # SAMPLES:
    dat.dt = (1. / float(_value(header[1], 10))) * 1.0e-6      # FREQUENCY: in MHz
    dat.travel_time = dat.dt * np.arange(snum) * 1.0e6
    tnum = int(_value(header[22], 11))                   # LAST TRACE:
    dat.trace_num = np.arange(tnum) + 1
    dat.trace_int = float(_value(header[9], 14)) * np.ones((tnum,))   # TIME INTERVAL:
    dat.trig = np.ones((tnum,)) * 36
    dat.trig_level = 0
    if os.path.exists(gps_fn):
        dat.snum, dat.tnum = snum, tnum
        _positions(dat, gps_fn)
    else:
        for attr in ('decday', 'lat', 'long', 'dist', 'elev'):
            setattr(dat, attr, np.arange(tnum))
    dat.pressure = np.zeros_like(dat.dist)
    with open(data_fn, 'rb') as f:
        raw = f.read()
    if len(raw) != 2 * snum * tnum:
        raise struct.error('unpack requires a buffer of %d bytes' % (2 * snum * tnum))
    _decode.install(dat, raw, rawload.ramac_layout(snum, tnum), resident)
    dat.check_attrs()
    return dat


def load_ramac(ramac_fn):
    """A RadarData from a RAMAC file; ``ramac_fn`` may be the base name, the ``.rad`` or the ``.rd3``."""
    return _read(ramac_fn)
