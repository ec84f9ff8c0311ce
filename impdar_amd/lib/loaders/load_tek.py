"""Tektronix oscilloscope records (http://dx.doi.org/10.7265/N5736NTS; reference ``src/impdar/lib/load/load_tek.py``).
A ``.DAT`` file is records of a 20-byte header -- decimal day (f4), wheel count (u2), pressure (i2), y and x increment
(f4, f4), averages (u2), length (u2) -- and 1000 uint16 samples, which become int16 around zero (512 subtracted with
wrap-around)."""
import numpy as np

from ... import rawload
from ..RadarData import RadarData
from ..RadarFlags import RadarFlags
from . import _decode

_HEADER = np.dtype([('decday', '<f4'), ('wheel', '<u2'), ('pressure', '<i2'), ('yinc', '<f4'), ('xinc', '<f4'),
                    ('averages', '<u2'), ('length', '<u2')])
_RECORD = rawload.TEK_HEAD + 2 * rawload.TEK_SNUM


def _headers(raw):
    """The header fields the reference's field-by-field reader ends up with: one value per whole record, and one more of
    every field that is still complete in a file cut inside a record (its reader stops at the first short read)."""
    whole = 0
    while (whole + 1) * _RECORD <= len(raw) and \
            np.frombuffer(raw, dtype='<u2', count=1, offset=whole * _RECORD + 18)[0] == rawload.TEK_SNUM:
        whole += 1
    rest = len(raw) - whole * _RECORD
    table = np.frombuffer(raw, dtype=np.dtype({'names': _HEADER.names, 'formats': [_HEADER[n] for n in _HEADER.names],
                                               'offsets': [_HEADER.fields[n][1] for n in _HEADER.names],
                                               'itemsize': _RECORD}), count=whole)
    fields = {}
    for name in _HEADER.names:
        col = np.array(table[name])
        end = _HEADER.fields[name][1] + _HEADER[name].itemsize
        if rest >= end:
            col = np.append(col, np.frombuffer(raw, dtype=_HEADER[name], count=1, offset=whole * _RECORD + end - _HEADER[name].itemsize))
        fields[name] = col
    return whole, fields


def _read(fn_tek, magnets_per_wheel=1, wheel_diameter=0.5, trigger_level=0.1, trigger_sample=None, channel=1,
          resident=None):
    dat = RadarData(None)
    dat.fn = fn_tek
    with open(fn_tek, 'rb') as f:
        raw = f.read()
    tnum, fields = _headers(raw)
    dat.decday = fields['decday']
    dat.pressure = fields['pressure']
    if tnum == 0:
        raise ValueError('no whole record of %d samples in %s' % (rawload.TEK_SNUM, fn_tek))
    layout = rawload.tek_layout(tnum)
    _decode.install(dat, raw, layout, resident)
    dat.trace_num = np.arange(dat.tnum)

    # distance along the profile from the wheel count
    dat.dist = fields['wheel'].astype(np.float32)
    dat.dist *= np.pi * wheel_diameter / magnets_per_wheel
    dat.trace_int = np.gradient(dat.dist)
    dat.dt = np.median(fields['xinc'])

    # the trigger: the first sample where the mean trace's gradient exceeds trigger_level of its largest value
    dat.trig_level = trigger_level
    if trigger_sample is None:
        # the mean trace is O(file) host work on the 2-byte samples; the resident radargram is not read back for it
        host = dat.data if dat.data is not None else rawload.decode_host(raw, layout)
        avg_trace = np.mean(host, axis=1)
        exceeds = np.abs(np.gradient(avg_trace)) > dat.trig_level * np.max(np.abs(avg_trace))
        trigger_sample = next(i for i, hit in enumerate(exceeds) if hit > 0.7)
    dat.trig = trigger_sample * np.ones(dat.tnum)
    dat.travel_time = (-trigger_sample + np.arange(dat.snum)) * dat.dt * 1e6
    dat.pressure -= dat.pressure[0]          # differences from the first record
    dat.chan = channel
    dat.flags = RadarFlags()
    dat.check_attrs()
    return dat


def load_tek(fn_tek, magnets_per_wheel=1, wheel_diameter=0.5, trigger_level=0.1, trigger_sample=None,
             channel=1, *args, **kwargs):
    """A RadarData from a Tek ``.DAT`` file."""
    return _read(fn_tek, magnets_per_wheel, wheel_diameter, trigger_level, trigger_sample, channel)
