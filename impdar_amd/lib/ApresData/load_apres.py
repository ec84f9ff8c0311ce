"""Load ApRES acquisitions: the instrument's ``.DAT`` burst files (RMB2, format 5), this package's ``.mat`` / ``.h5``
files, the ``.mat`` that the British Antarctic Survey's Matlab scripts save and, with ``netCDF4``, their ``.nc``
(``src/impdar/lib/ApresData/load_apres.py``).

A ``.DAT`` acquisition keeps the counts as they were read beside their scale (see the package's docstring); every
other attribute is there on return."""
import datetime
import os
import re
from copy import deepcopy

import numpy as np
from scipy.io import loadmat

from . import ApresData
from ..ImpdarError import ImpdarError
from .ApresHeader import header_field

try:
    from netCDF4 import Dataset
    nc_load = True
except ImportError:
    nc_load = False

END_HEADER = '*** End Header ***'
_MSG_FORMAT = ('Loading functions have only been written for rmb5 data.' + ' ' * 24 +
               'Look back to the original Matlab scripts if you need to implement earlier formats.')
CHIRP_INTERVAL = 1.6384 / (24. * 3600.)      # days


def load_apres(fns_apres, burst=1, fs=40000, *args, **kwargs):
    """Load every file of ``fns_apres`` and stack them along a new first axis into one object of ``bnum =
    len(files)`` bursts.  A file that cannot be loaded is left out, as in the reference (:60-66); with none left
    that is its ``IndexError``.  ``fn`` of the result is the first name without its extension."""
    apres_data = []
    for fn in fns_apres:
        try:
            apres_data.append(load_apres_single_file(fn, burst=burst, fs=fs, *args, **kwargs))
        except Exception:
            Warning('Cannot load file: ' + fn)

    out = deepcopy(apres_data[0])
    ext = os.path.splitext(fns_apres[0])[1]

    if len(apres_data) > 1 or ext in ['.DAT', '.dat']:
        for dat in apres_data[1:]:
            if out.snum != dat.snum:
                raise ValueError('Need the same number of vertical samples in each file')
            if out.cnum != dat.cnum:
                raise ValueError('Need the same number of chirps in each file')
            if not np.all(out.travel_time == dat.travel_time):
                raise ValueError('Need matching travel time vectors')
            if not np.all(out.frequencies == dat.frequencies):
                raise ValueError('Need matching frequency vectors')

        held = [dat.raw_counts() for dat in apres_data]
        if all(h is not None and h[0].dtype == held[0][0].dtype and h[1] == held[0][1] for h in held):
            out.set_counts(np.stack([h[0] for h in held]), held[0][1])       # the counts stay counts
            shape = out.raw_counts()[0].shape
        else:
            out.data = np.stack([dat.data for dat in apres_data])
            shape = np.shape(out.data)
        for name in ('chirp_num', 'chirp_att', 'chirp_time'):                # per chirp: a row per file
            setattr(out, name, np.stack([getattr(dat, name) for dat in apres_data]))
        for name in ('decday', 'time_stamp', 'lat', 'long', 'temperature1', 'temperature2', 'battery_voltage'):
            setattr(out, name, np.hstack([getattr(dat, name) for dat in apres_data]))   # per burst: an entry per file
        out.bnum = shape[0]

    out.fn = os.path.splitext(fns_apres[0])[0]
    return out


def load_apres_single_file(fn_apres, burst=1, fs=40000, *args, **kwargs):
    """Load one file by its extension.  For a ``.DAT`` file ``burst`` is the number, from 1, of the burst to load.

    The reference reads ``burst = 1`` only: for a later burst it reads the first header again and seeks to an offset
    counted in the characters of the header's ``str(bytes)`` form.  Here ``burst = k > 1`` walks the file: each
    burst's own header, then ``cnum snum 2`` bytes of counts (``4`` in an averaged burst), which start -- as in the
    reference -- at the byte after the end-of-header marker."""
    ext = os.path.splitext(fn_apres)[1]
    if ext == '.mat':
        if 'vdat' in loadmat(fn_apres):       # the struct of the BAS scripts
            return load_BAS_mat(fn_apres)
        return ApresData(fn_apres)
    elif ext == '.h5':
        return ApresData(fn_apres)
    elif ext == '.nc':
        return load_BAS_nc(fn_apres)
    elif ext not in ['.dat', '.DAT']:
        raise ValueError('Expecting a certain filetype; either .mat, .h5, .dat, .DAT, .nc')

    apres_data = ApresData(None)
    header = apres_data.header
    header.update_parameters(fn_apres)
    counts, divisor = load_burst(apres_data, burst, fs)
    if header.file_format is None:
        raise TypeError("File format is 'None', cannot load")
    att_set = header.attenuator1 + 1.0j * header.attenuator2

    _derive_band(header)
    apres_data.dt = 1. / header.fs

    cnum, snum = apres_data.cnum, apres_data.snum
    if counts.size != cnum * snum:
        raise ValueError('the burst holds %d of its %d x %d samples' % (counts.size, cnum, snum))
    apres_data.chirp_num = np.arange(cnum)
    apres_data.chirp_att = np.zeros((cnum)).astype(np.cdouble)
    apres_data.chirp_time = np.zeros((cnum))
    header.chirp_interval = CHIRP_INTERVAL
    for chirp in range(cnum):
        apres_data.chirp_att[chirp] = att_set[chirp // cnum]      # (the first setting for every chirp: reference :202)
        # one time stamp in the header's 2000 bytes, or NumPy's error for a vector in a scalar's place (reference :203)
        apres_data.chirp_time[chirp], = apres_data.decday + header.chirp_interval * chirp
    apres_data.set_counts(counts.reshape(cnum, snum), divisor)

    _sample_axes(apres_data)
    apres_data.data_dtype = np.dtype(float)
    apres_data.check_attrs()
    return apres_data


def _fields(header_string, key):
    """Every occurrence of ``key`` in the header string, each up to the next backslash (reference :337-343)."""
    starts = [m.start() for m in re.finditer(key, header_string)]
    ends = [header_string[ind:].find('\\') for ind in starts]
    return [header_string[s + len(key):e + s] for s, e in zip(starts, ends)]


def load_burst(self, burst=1, fs=40000, max_header_len=2000, burst_pointer=0):
    """Read burst number ``burst`` of the file whose header ``self.header`` has been read: the burst's settings and
    records into ``self``, and return ``(counts, divisor)``, the flat payload as it is in the file (uint16, or uint32
    with ``Average=2``) and what its volts are divided by.

    As in the reference (:269) a burst is looked for only while ``max_header_len`` bytes or more follow its start."""
    header = self.header
    if header.fn is None:
        raise TypeError('Read in the header before loading data.')
    if header.file_format != 5:
        raise TypeError(_MSG_FORMAT)
    try:
        fid = open(header.fn, 'rb')
    except FileNotFoundError:
        self.flags.file_read_code = 'Unable to read file' + header.fn
        raise ImpdarError('Cannot open file', header.fn)

    with fid:
        fid.seek(0, 2)
        file_len = fid.tell()
        burst_count = 1
        data_ind = None
        while burst_count <= burst and burst_pointer <= file_len - max_header_len:
            header.read_header(header.fn, max_header_len, offset=burst_pointer)
            hs = header.header_string
            try:
                keys = ['N_ADC_SAMPLES=', 'NSubBursts=', 'Average=', 'nAttenuators=', 'Attenuator1=', 'AFGain=', 'TxAnt=',
                        'RxAnt=']
                output = [header_field(hs, k) for k in keys]
                output = ['' if o is None else o for o in output]
                self.snum = int(output[0])
                header.average = int(output[2])
                header.n_subbursts = int(output[1])
                header.n_attenuators = int(output[3])
                header.attenuator1 = np.array(output[4].split(',')).astype(int)[:header.n_attenuators]
                header.attenuator2 = np.array(output[5].split(',')).astype(int)[:header.n_attenuators]
                header.tx_ant = np.array(output[6].split(',')).astype(int)
                header.rx_ant = np.array(output[7].split(',')).astype(int)
                header.tx_ant = header.tx_ant[header.tx_ant == 1]
                header.rx_ant = header.rx_ant[header.rx_ant == 1]
                if header.average != 0:
                    self.cnum = 1
                else:
                    self.cnum = header.n_subbursts * len(header.tx_ant) * len(header.rx_ant) * header.n_attenuators
            except ValueError:
                self.flags.file_read_code = 'Corrupt header in burst' + str(burst_count) + 'for file' + header.fn
                self.bnum = burst_count
                raise ImpdarError('Burst Read Failed.')
            # the payload starts at the byte after the marker (the CR LF that ends the marker's line is its first
            # sample): the reference's own offset (:364-366)
            fid.seek(burst_pointer)
            marker = fid.read(max_header_len).find(END_HEADER.encode())
            if marker < 0:
                self.flags.file_read_code = 'Corrupt header in burst' + str(burst_count) + 'for file' + header.fn
                self.bnum = burst_count
                raise ImpdarError('Burst Read Failed.')
            data_ind = burst_pointer + marker + len(END_HEADER)
            if burst_count < burst:
                burst_pointer = data_ind + self.cnum * self.snum * (4 if header.average != 0 else 2)
            burst_count += 1

        hs = header.header_string
        if 'Time stamp' not in hs:
            self.flags.file_read_code = 'Burst' + str(self.bnum) + 'not found in file' + header.fn
        else:
            self.time_stamp = np.array([datetime.datetime.strptime(str_time, '%Y-%m-%d %H:%M:%S')
                                        for str_time in _fields(hs, 'Time stamp=')])
            self.decday = _datenum(self.time_stamp)
        self.lat = np.array(_fields(hs, 'Latitude=')).astype(float)
        self.long = np.array(_fields(hs, 'Longitude=')).astype(float)
        self.temperature1 = np.array(_fields(hs, 'Temp1=')).astype(float)
        self.temperature2 = np.array(_fields(hs, 'Temp2=')).astype(float)
        self.battery_voltage = np.array(_fields(hs, 'BatteryVoltage=')).astype(float)

        if burst_count != burst + 1:
            self.flags.file_read_code = 'Burst' + str(self.bnum) + 'not found in file' + header.fn
            self.bnum = burst_count - 1
            raise ImpdarError('Burst {:d} not found in file {:s}'.format(self.bnum, header.fn))
        if header.average == 1:
            # (the reference asks NumPy for a dtype 'float4', which does not exist: its TypeError)
            raise TypeError('Average=1 (a burst stacked into 4-byte floats) is not supported')
        fid.seek(data_ind)
        counts = np.fromfile(fid, dtype='<u4' if header.average == 2 else '<u2', count=self.cnum * self.snum)
        divisor = float(header.n_subbursts * header.n_attenuators) if header.average == 2 else 1.
        self.bnum = burst

    # temperatures above 300 are a wrapped negative reading
    self.temperature1[self.temperature1 > 300] -= 512
    self.temperature2[self.temperature2 > 300] -= 512
    self.flags.file_read_code = 'Successful Read'
    return counts, divisor


# header attribute <- field of the BAS scripts' ``vdat`` struct, and the same for the object itself
_BAS_HEADER = {'f0': 'f0', 'fs': 'fs', 'f1': 'f1', 'fc': 'fc', 'attenuator1': 'Attenuator_1', 'attenuator2': 'Attenuator_2',
               'chirp_length': 'T', 'chirp_grad': 'K', 'bandwidth': 'B', 'lambdac': 'lambdac', 'er': 'er', 'ci': 'ci',
               'n_subbursts': 'SubBurstsInBurst', 'average': 'Average'}
_BAS_OBJECT = {'snum': 'Nsamples', 'cnum': 'chirpNum', 'bnum': 'Burst', 'decday': 'TimeStamp'}
# header attribute <- (attribute of a bas-apres netCDF burst, conversion)
_NC_HEADER = {'noDwellHigh': ('NoDwell', int), 'f0': ('StartFreq', float), 'f_stop': ('StopFreq', float),
              'ramp_up_step': ('FreqStepUp', float), 'ramp_down_step': ('FreqStepDn', float), 'tstep_up': ('TStepUp', float),
              'tstep_down': ('TStepDn', float), 'snum': ('N_ADC_SAMPLES', float), 'n_attenuators': ('nAttenuators', int),
              'tx_ant': ('TxAnt', None), 'rx_ant': ('RxAnt', None), 'average': ('Average', float),
              'n_subbursts': ('NSubBursts', int)}


def _datenum(stamps):
    """Matlab's datenum of ``datetime`` objects."""
    since = np.asarray(stamps) - datetime.datetime(1, 1, 1)
    return np.array([d.days + d.seconds / 86400. for d in since]) + 366.


def _derive_band(header):
    """``f1``, ``bandwidth``, ``fc`` and, for ice of relative permittivity 3.18, ``er``, ``ci``, ``lambdac`` from the chirp."""
    header.f1 = header.f0 + header.chirp_length * header.chirp_grad / 2. / np.pi
    header.bandwidth = header.chirp_length * header.chirp_grad / 2 / np.pi
    header.fc = header.f0 + header.bandwidth / 2.
    header.er = 3.18
    header.ci = 3e8 / np.sqrt(header.er)
    header.lambdac = header.ci / header.fc


def _sample_axes(dat):
    """``travel_time`` (microseconds) and ``frequencies`` of the samples of a chirp."""
    seconds = dat.dt * np.arange(dat.snum)
    dat.frequencies = dat.header.f0 + seconds * dat.header.chirp_grad / (2. * np.pi)
    dat.travel_time = seconds * 1.0e6


def load_BAS_mat(fn, chirp_interval=CHIRP_INTERVAL):
    """Load the ``vdat`` struct of a ``.mat`` file saved by the British Antarctic Survey's Matlab scripts: its scalars
    by the two tables above, ``t`` and ``f`` as the sample axes, ``vif`` as the data (one burst where it is 2-d),
    chirps numbered from 1 and timed ``chirp_interval`` days apart from ``TimeStamp``."""
    vdat = loadmat(fn)['vdat'][0]
    dat = ApresData(None)
    for target, table in ((dat.header, _BAS_HEADER), (dat, _BAS_OBJECT)):
        for attr, field in table.items():
            setattr(target, attr, vdat[field][0][0][0])
    dat.header.chirp_interval = chirp_interval
    dat.dt = 1.0 / dat.header.fs
    dat.travel_time, dat.frequencies = vdat['t'][0].T, vdat['f'][0].T
    dat.chirp_num = np.arange(dat.cnum) + 1
    dat.chirp_att = vdat['chirpAtt'][0]
    dat.chirp_time = dat.decday + chirp_interval * np.arange(0.0, dat.cnum, 1.0)
    vif = vdat['vif'][0]
    dat.data = vif[None] if vif.ndim == 2 else vif
    dat.check_attrs()
    return dat


def load_BAS_nc(fn, fs=40000, chirp_interval=CHIRP_INTERVAL, *args, **kwargs):
    """Load the first burst of a netCDF file written by https://github.com/antarctica/bas-apres (a group per burst,
    or the burst at the root), with the chirp derived from its attributes as ``ApresHeader.update_parameters`` derives
    it from the registers.  Needs ``netCDF4``."""
    if not nc_load:
        raise ImportError('Need the netCDF4 library to load nc files.')
    with Dataset(fn, 'r') as fin:
        burst = fin.groups[list(fin.groups.keys())[0]] if len(fin.groups) > 0 else fin
        attrs = vars(burst).copy()
        data = np.array([burst.variables['data'][:]])

    dat = ApresData(None)
    header = dat.header
    header.fs, header.fn, header.file_format = fs, fn, 'BAS_nc'
    for attr, (key, convert) in _NC_HEADER.items():
        setattr(header, attr, attrs[key] if convert is None else convert(attrs[key]))
    header.attenuator1 = np.array(attrs['Attenuator1'].split(',')).astype(int)[:header.n_attenuators]
    header.attenuator2 = np.array(attrs['AFGain'].split(',')).astype(int)[:header.n_attenuators]
    header.chirp_interval = chirp_interval
    header.nsteps_DDS = round(abs((header.f_stop - header.f0) / header.ramp_up_step))
    header.chirp_length = int(header.nsteps_DDS * header.tstep_up)
    header.nchirp_samples = round(header.chirp_length * header.fs)
    if header.nchirp_samples > header.snum:
        header.chirp_length = header.snum / header.fs
    header.chirp_grad = 2. * np.pi * (header.ramp_up_step / header.tstep_up)
    header.ramp_dir = 'down' if header.f_stop > 400e6 else 'up'
    _derive_band(header)

    dat.data, dat.bnum = data, 1
    dat.snum, dat.cnum = int(attrs['N_ADC_SAMPLES']), header.n_subbursts
    dat.dt = 1.0 / header.fs
    for attr, key in (('temperature1', 'Temp1'), ('temperature2', 'Temp2'), ('battery_voltage', 'BatteryVoltage')):
        setattr(dat, attr, np.array([float(attrs[key])]))
    dat.time_stamp = np.array([datetime.datetime.strptime(attrs['Time stamp'], '%Y-%m-%d %H:%M:%S')])
    dat.decday = _datenum(dat.time_stamp)
    dat.chirp_time = dat.decday + chirp_interval * np.arange(0.0, dat.cnum, 1.0)
    dat.chirp_att = np.full(dat.cnum, header.attenuator1[0] + 1j * header.attenuator2[0], dtype=np.cdouble)
    dat.chirp_num = np.array([np.arange(dat.cnum) + 1])
    _sample_axes(dat)
    dat.data_dtype = dat.data.dtype
    dat.check_attrs()
    return dat
