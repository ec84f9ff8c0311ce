"""GSSI SIR controllers: ``.DZT`` with an optional ``.DZG`` of NMEA fixes (reference
``src/impdar/lib/load/load_gssi.py``).  The ``.DZT`` is a file header of ``32768 * bits / 8`` bytes, then ``snum`` unsigned
counts of 16 or 32 bits per trace with no trace header; the counts are kept as the same bits signed, and the two top rows,
which hold the instrument's marks, take the third row's values."""
import codecs
import datetime
import os
import struct

import numpy as np

from ... import rawload
from ..RadarData import RadarData
from ..RadarFlags import RadarFlags
from ..gpslib import RadarGPS
from . import _decode


class GSSITime(object):
    """The 32-bit date of a GSSI header, low bit first: 5 bits of seconds / 2, 6 of minutes, 5 of hours, 5 of day, 4 of
    month, 7 of years since 1980."""
    _FIELDS = (('sec2', 5), ('minute', 6), ('hour', 5), ('day', 5), ('month', 4), ('year', 7))

    def __init__(self, binary_data, le=True):
        word = int.from_bytes(bytes(binary_data[:4]), 'little')
        for name, width in self._FIELDS:
            setattr(self, name, word & ((1 << width) - 1))
            word >>= width

    def to_datetime(self):
        if self.year > 0:
            return datetime.datetime(self.year + 1980, self.month, self.day, self.hour, self.minute, self.sec2)
        return datetime.datetime(2000, 1, 1, 1, 1, 1)


def _first_field(line):
    return line.split(',')[0]


def _get_dzg_data(fn_dzg, trace_nums):
    """GPS of a ``.DZG``: every $GPGGA sentence is matched with the last $GSSIS (scan number) line between it and the GGA
    before it, pairs whose order is broken are dropped, and the fixes are carried onto ``trace_nums``."""
    with codecs.open(fn_dzg, 'r', encoding='utf-8', errors='ignore') as f:
        lines = f.readlines()
    gga_all = [i for i, line in enumerate(lines) if _first_field(line) == '$GPGGA']
    scan_all = np.array([i for i, line in enumerate(lines) if _first_field(line) == '$GSSIS'])
    scan_inds, gga_inds = [], []
    for k, at in enumerate(gga_all):
        after = gga_all[k - 1] if k > 0 else 0
        between = scan_all[np.logical_and(scan_all < at, scan_all > after)]
        if len(between) == 0:
            continue
        try:
            if float(lines[np.max(between)].split(',')[1]).is_integer():     # a scan line can be corrupted too
                scan_inds.append(np.max(between))
                gga_inds.append(at)
        except ValueError:
            continue
    # a scan line counts when its GGA lies before the next scan line
    keep, shift = [], 0
    for k, at in enumerate(scan_inds[:-1]):
        if at < gga_inds[k + shift] < scan_inds[k + 1]:
            keep.append(at)
        else:
            shift -= 1
    if gga_inds[-1] > scan_inds[-1]:
        keep.append(scan_inds[-1])
    keep = set(keep)
    scans = np.array([int(line.split(',')[1]) for i, line in enumerate(lines) if i in keep])
    chosen = set(gga_inds)
    return RadarGPS([line for i, line in enumerate(lines) if i in chosen], scans, trace_nums)


def _read(fn_dzt, resident=None):
    dat = RadarData(None)
    dat.fn = fn_dzt
    with open(fn_dzt, 'rb') as f:
        raw = f.read()
    snum, bits, trig = struct.unpack('<HHh', raw[4:10])
    if bits not in (16, 32):
        raise ValueError('GSSI samples are 16 or 32 bits, got %d' % bits)
    el = bits // 8
    dat.range = struct.unpack('<f', raw[26:30])[0]
    dat.create = GSSITime(raw[32:36]).to_datetime()
    dat.chan = struct.unpack('<H', raw[52:54])[0]
    counts = (len(raw) - rawload.GSSI_HEADER_WORDS * el) // el
    if counts < 0:
        raise struct.error('the file ends inside its %d-byte header' % (rawload.GSSI_HEADER_WORDS * el))
    if snum == 0 or counts % snum:
        raise ValueError('cannot reshape array of size %d into shape (%d,newaxis)' % (counts, snum))
    if snum < 3:
        raise IndexError('index 2 is out of bounds for axis 0 with size %d' % snum)
    _decode.install(dat, raw, rawload.gssi_layout(snum, counts // snum, bits), resident)
    tnum = dat.tnum
    dat.trace_num = np.arange(tnum) + 1
    dat.trig_level = 0.
    dat.trig = trig * np.ones(tnum)
    dat.pressure = np.zeros((tnum, ))
    dat.flags = RadarFlags()
    dat.dt = dat.range / dat.snum * 1.0e-9
    dat.travel_time = np.atleast_2d(np.arange(0, dat.range / 1.0e3, dat.dt * 1.0e6)).transpose()
    dat.travel_time += dat.dt * 1.0e6

    fn_dzg = os.path.splitext(fn_dzt)[0] + '.DZG'
    if os.path.exists(fn_dzg):
        gps = dat.gps_data = _get_dzg_data(fn_dzg, dat.trace_num)
        dat.lat, dat.long = gps.lat, gps.lon
        dat.x_coord, dat.y_coord = gps.x, gps.y
        dat.dist = gps.dist.flatten()
        dat.elev = gps.z
        days = (dat.create - datetime.datetime(1, 1, 1, 0, 0, 0)).days
        tmin = days + np.min(gps.dectime) + 377.         # Matlab's day numbers
        tmax = days + np.max(gps.dectime) + 377.
        dat.decday = np.linspace(tmin, tmax, tnum)
        dat.trace_int = np.hstack((np.array(np.nanmean(np.diff(dat.dist))), np.diff(dat.dist)))
    else:
        for attr in ('lat', 'long', 'x_coord', 'y_coord', 'dist', 'elev'):
            setattr(dat, attr, np.zeros((tnum,)))
        dat.decday = np.arange(tnum)
        dat.trace_int = np.ones((tnum,))
    dat.check_attrs()
    return dat


def load_gssi(fn_dzt, *args, **kwargs):
    """A RadarData from a GSSI ``.DZT`` file (and the ``.DZG`` beside it, if there is one)."""
    return _read(fn_dzt)
