"""Sensors & Software pulseEKKO: ``.DT1`` records, ``.HD`` text header, optional ``.GPS`` (reference
``src/impdar/lib/load/load_pulse_ekko.py``; the ``.GPZ`` project partitioning is not part of this package).  Every
``.DT1`` record is a 128-byte trace header (25 float32 and 28 characters) and ``snum`` samples: int16 under the first
header generation (no ``pulseEKKO`` string in the ``.HD``: version 1.0), float32 after it.  Each trace has the mean of its
first 100 samples (NaN left out) taken off, in float64, and is stored back in the file's type."""
import datetime
import io
import os.path
import struct

import numpy as np

from ... import rawload
from ..RadarData import RadarData
from ..RadarFlags import RadarFlags
from ..gpslib import RadarGPS
from . import _decode

# float32 slot of the trace header -> (attribute, row of it)
_HEADER_SLOTS = {0: ('trace_numbers', 0), 1: ('positions', 0), 2: ('points_per_trace', 0), 3: ('topography', 0),
                 5: ('bytes_per_point', 0), 7: ('n_stacks', 0), 8: ('time_window', 0), 9: ('pos', 0), 11: ('pos', 1),
                 13: ('pos', 2), 14: ('receive', 0), 15: ('receive', 1), 16: ('receive', 2), 17: ('transmit', 0),
                 18: ('transmit', 1), 19: ('transmit', 2), 20: ('tz_adjustment', 0), 21: ('zero_flag', 0),
                 23: ('time_of_day', 0), 24: ('comment_flag', 0)}


class TraceHeaders(object):
    """The trace headers of a ``.DT1`` file, one column per trace."""

    def __init__(self, tnum):
        self.header_index = 0
        for name, rows in (('trace_numbers', 1), ('positions', 1), ('points_per_trace', 1), ('topography', 1),
                           ('bytes_per_point', 1), ('n_stacks', 1), ('time_window', 1), ('pos', 3), ('receive', 3),
                           ('transmit', 3), ('tz_adjustment', 1), ('zero_flag', 1), ('time_of_day', 1),
                           ('comment_flag', 1)):
            setattr(self, name, np.zeros((rows, tnum)))
        self.comment = ['' for _ in range(tnum)]

    def fill(self, raw, stride):
        """All headers of the file at once: record t starts at byte ``t * stride``."""
        tnum = len(self.comment)
        table = np.frombuffer(raw, dtype=np.dtype({'names': ['f', 'c'], 'formats': [('<f4', (25,)), 'S1'],
                                                   'offsets': [0, 100], 'itemsize': stride}), count=tnum)
        for slot, (name, row) in _HEADER_SLOTS.items():
            getattr(self, name)[row, :] = table['f'][:, slot]
        # the reference keeps the text of the first comment character's bytes object
        self.comment = [str(raw[t * stride + 100:t * stride + 101]) for t in range(tnum)]
        self.header_index = tnum


def _last_token(line):
    return line.rstrip('\n\r ').split(' ')[-1]


def _date(line, slices):
    return datetime.datetime(*[int(line[a:b]) for a, b in slices], 0, 0, 0)


def _parse_header(dat, hdname):
    """tnum, snum, the time window (ns), the trigger sample and the day of the survey from the ``.HD`` text.  Three
    generations: no ``pulseEKKO`` string (version 1.0, the date on line 4), version <= 1.5 (the date on line 2), version
    > 1.5 (line 2 as %Y-%b-%d)."""
    with open(hdname, 'r') as f:
        text = f.read()
    at = text.find('pulseEKKO')
    dat.version = '1.0' if at == -1 else text[at + 10:at + text[at:].find('\n')]
    window = day = None
    for i, line in enumerate(io.StringIO(text)):
        if 'TRACES' in line:
            dat.tnum = int(_last_token(line))
        if 'PTS' in line:
            dat.snum = int(_last_token(line))
        if ('WINDOW' in line and 'AMPLITUDE' not in line):
            window = float(_last_token(line))
        if 'TIMEZERO' in line:
            dat.trig = int(float(_last_token(line))) * np.ones((dat.tnum,))
        if i == 4 and dat.version == '1.0':
            try:
                day = _date(line, ((6, 10), (1, 2), (3, 5)))
            except ValueError:
                day = _date(line, ((0, 4), (5, 7), (8, 10)))
        elif i == 2 and float(dat.version) <= 1.5:
            try:
                day = _date(line, ((6, 10), (0, 2), (3, 5)))
            except ValueError:
                day = _date(line, ((28, 32), (34, 36), (36, 38)))
        elif i == 2:
            day = datetime.datetime.strptime(line + 'T00:00:00', '%Y-%b-%d\nT%H:%M:%S')
    return window, day


def _get_gps_data(fn_gps, trace_nums):
    """GPS of a ``.GPS`` file: 'Trace #n at position x' lines, each followed by its $GPGGA sentence."""
    with open(fn_gps) as f:
        lines = f.readlines()
    marks = [line for line in lines if line[:5] == 'Trace']
    gga = [line for line in lines if line[:6] == '$GPGGA']
    if len(gga) == 0:
        raise ValueError('I can only do gga sentences right now')
    scans = np.array([int(float(_last_token(line))) for line in marks])
    return RadarGPS(gga, scans, trace_nums)


def _read(fn_dt1, resident=None):
    dat = RadarData(None)
    dat.fn = fn_dt1
    stem = os.path.splitext(fn_dt1)[0]
    window, day = _parse_header(dat, stem + '.HD')
    first = dat.version == '1.0'
    with open(stem + '.DT1', 'rb') as f:
        raw = f.read()
    layout = rawload.pe_layout(dat.snum, dat.tnum, first)
    if len(raw) < layout.stride * layout.tnum:
        if first or len(raw) < layout.stride * (layout.tnum - 1) + rawload.PE_HEAD:
            raise struct.error('unpack requires a buffer of %d bytes' % (layout.stride * layout.tnum))
        raise ValueError('the last trace of %s is shorter than %d samples' % (fn_dt1, dat.snum))
    dat.traceheaders = TraceHeaders(dat.tnum)
    dat.traceheaders.fill(raw, layout.stride)
    _decode.install(dat, raw, layout, resident)
    tnum = dat.tnum

    dat.chan = 1
    dat.trace_num = np.arange(tnum) + 1
    dat.trig_level = 0.
    dat.pressure = np.zeros((tnum, ))
    dat.flags = RadarFlags()
    dat.dt = window / dat.snum * 1.0e-9
    dat.travel_time = np.atleast_2d(np.arange(0, window / 1.e3, dat.dt * 1.0e6)).transpose()
    dat.travel_time += dat.dt * 1.0e6

    gps_fn = stem + '.GPS'
    if os.path.exists(gps_fn):
        gps = dat.gps_data = _get_gps_data(gps_fn, dat.trace_num)
        dat.lat, dat.long = gps.lat, gps.lon
        dat.x_coord, dat.y_coord = gps.x, gps.y
        dat.dist = gps.dist.flatten()
        dat.elev = gps.z
        dat.trace_int = np.hstack((np.array(np.nanmean(np.diff(dat.dist))), np.diff(dat.dist)))
        tmin = day.toordinal() + np.min(gps.dectime) + 366.       # Matlab's day numbers
        tmax = day.toordinal() + np.max(gps.dectime) + 366.
        dat.decday = np.linspace(tmin, tmax, tnum)
    else:
        print('Warning: Cannot find gps file, %s.' % gps_fn)
        for attr in ('lat', 'long', 'x_coord', 'y_coord', 'dist', 'elev'):
            setattr(dat, attr, np.zeros((tnum,)))
        dat.trace_int = np.ones((tnum,))
        dat.decday = day.toordinal() + 366. + dat.traceheaders.time_of_day.flatten() / 60. / 60. / 24.
    dat.check_attrs()
    return dat


def load_pe(fn_dt1, *args, **kwargs):
    """A RadarData from a pulseEKKO ``.DT1`` file with its ``.HD`` (and ``.GPS``) beside it."""
    return _read(fn_dt1)
