"""What the instrument-file tests share: the shapes and (layout, in_kind, op) combinations of the decode sweep, writers of
small GSSI / pulseEKKO / RAMAC / Tek files, a NumPy restatement of the decode that follows the reference's readers trace
by trace (``np.nanmean`` itself, one record at a time: the expected value of the GPU sweep), and the flattening of a
loaded object into what ``np.savez`` stores.  Nothing here imports the package under test."""
import collections
import datetime
import os
import struct
import warnings

import numpy as np

I16, I32, F32 = 0, 1, 2
NONE, GSSI_TOP, TEK_BIAS, PE_DEMEAN = 0, 1, 2, 3
NATIVE, OUT_F32, OUT_F64 = 0, 1, 2
IN_DTYPE = {I16: np.dtype('<i2'), I32: np.dtype('<i4'), F32: np.dtype('<f4')}
OUT_DTYPES = {NATIVE: None, OUT_F32: np.float32, OUT_F64: np.float64}

Layout = collections.namedtuple('Layout', 'base stride head snum tnum in_kind op')

# one-trace file and the GSSI minimum; both sides of the 8-element break in the mean's order; a window of exactly and just
# under 100; tile edges on both axes and both sides of 64; odd snum (2-byte aligned records), odd tnum (unaligned rows)
SHAPES = [(3, 1), (3, 5), (7, 3), (8, 2), (9, 65), (63, 64), (65, 63), (100, 2), (101, 129), (137, 5), (129, 257)]

# every valid (format layout, in_kind, op)
COMBOS = {
    'gssi16': ('gssi', I16, GSSI_TOP),
    'gssi32': ('gssi', I32, GSSI_TOP),
    'pe16': ('pe', I16, PE_DEMEAN),
    'pe32f': ('pe', F32, PE_DEMEAN),
    'ramac': ('ramac', I16, NONE),
    'tek': ('tek', I16, TEK_BIAS),
    'plain32': ('ramac', I32, NONE),
    'plain32f': ('ramac', F32, NONE),
}


def layout_for(fmt, in_kind, op, snum, tnum, base=None):
    """The format's record layout at any (snum, tnum): the sweep uses a Tek-like layout at other lengths than 1000 and a
    GSSI-like one with a short file header (``base``)."""
    el = IN_DTYPE[in_kind].itemsize
    if fmt == 'gssi':
        return Layout(32768 * el if base is None else base, snum * el, 0, snum, tnum, in_kind, op)
    if fmt == 'pe':
        return Layout(base or 0, 128 + snum * el, 128, snum, tnum, in_kind, op)
    if fmt == 'tek':
        return Layout(base or 0, 20 + snum * el, 20, snum, tnum, in_kind, op)
    return Layout(base or 0, snum * el, 0, snum, tnum, in_kind, op)


def samples_for(in_kind, snum, tnum, seed):
    """(tnum, snum) samples.  Integers over the whole range with both extremes present; floats spread over e^+-20, one
    NaN inside the 100-sample window of trace 0 and an all-NaN window in trace 1 (where there is one)."""
    rng = np.random.default_rng(seed)
    dt = IN_DTYPE[in_kind]
    if in_kind == F32:
        a = (rng.standard_normal((tnum, snum)) * np.exp(rng.uniform(-20., 20., (tnum, snum)))).astype(dt)
        a[0, min(snum, 100) // 2] = np.nan
        a[0, 0] = -0.0
        if tnum > 1:
            a[1, :100] = np.nan
        return a
    info = np.iinfo(dt)
    a = rng.integers(info.min, info.max, (tnum, snum), endpoint=True).astype(dt)
    at = int(rng.integers(a.size))
    a.flat[at] = info.min
    a.flat[(at + 1) % a.size] = info.max
    return a


def raw_for(layout, samples, seed=0):
    """The bytes of a file with these samples: everything outside them (file header, trace headers) is noise."""
    L = layout
    el = IN_DTYPE[L.in_kind].itemsize
    rng = np.random.default_rng(1000 + seed)
    buf = rng.integers(0, 256, L.base + L.stride * L.tnum, dtype=np.uint8)
    for t in range(L.tnum):
        at = L.base + t * L.stride + L.head
        buf[at:at + L.snum * el] = np.frombuffer(samples[t].astype(IN_DTYPE[L.in_kind]).tobytes(), dtype=np.uint8)
    return buf.tobytes()


def restate(raw, layout):
    """The reference readers' ``data`` for this layout, one record at a time: (snum, tnum), native dtype."""
    L = layout
    dt = IN_DTYPE[L.in_kind]
    native = np.dtype(dt.name)
    out = np.zeros((L.snum, L.tnum), dtype=native)
    for t in range(L.tnum):
        at = L.base + t * L.stride + L.head
        trace = np.frombuffer(raw, dtype=dt, count=L.snum, offset=at)
        if L.op == PE_DEMEAN:
            wide = tuple(float(x) for x in trace) if L.in_kind == F32 else tuple(int(x) for x in trace)
            with np.errstate(all='ignore'), warnings.catch_warnings():
                warnings.simplefilter('ignore')
                wide = wide - np.nanmean(wide[:100])
                out[:, t] = wide
        else:
            out[:, t] = trace
    if L.op == GSSI_TOP:
        out[0, :] = out[2, :]
        out[1, :] = out[2, :]
    elif L.op == TEK_BIAS:
        out -= 512
    return out


def expected(native, out_kind):
    """``reference_data.astype(out dtype)``."""
    with np.errstate(all='ignore'):
        return native if out_kind == NATIVE else native.astype(OUT_DTYPES[out_kind])


def same_bits(got, want):
    """dtype, shape, NaN positions, and every other value as bits (the sign of zero included)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind != 'f':
        return got.tobytes() == want.tobytes()
    gn, wn = np.isnan(got), np.isnan(want)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(u)[~gn], want.view(u)[~wn]))


# ---------------------------------------------------------------------------------------------------- file writers
def gssi_date(when):
    """The four bytes of a GSSI header date: 5 bits of seconds / 2, 6 of minutes, 5 of hours, 5 day, 4 month, 7 years
    since 1980, low bit first."""
    word = (when.second // 2) | (when.minute << 5) | (when.hour << 11) | (when.day << 16) | (when.month << 21) | \
           ((when.year - 1980) << 25)
    return struct.pack('<I', word)


def write_dzt(path, samples, bits, range_ns=100., trig=0, chan=1, when=datetime.datetime(2019, 7, 26, 16, 58, 42),
              header_bytes=None, tail=b''):
    """A GSSI .DZT with (tnum, snum) unsigned counts of 16 or 32 bits."""
    tnum, snum = samples.shape
    el = bits // 8
    head = bytearray(32768 * el if header_bytes is None else header_bytes)
    head[0:2] = struct.pack('<H', 0x00ff)
    head[2:4] = struct.pack('<H', 1024)
    head[4:6] = struct.pack('<H', snum)
    head[6:8] = struct.pack('<H', bits)
    head[8:10] = struct.pack('<h', trig)
    head[26:30] = struct.pack('<f', range_ns)
    head[32:36] = gssi_date(when)
    head[52:54] = struct.pack('<H', chan)
    with open(path, 'wb') as f:
        f.write(bytes(head))
        f.write(np.ascontiguousarray(samples, dtype='<u%d' % el).tobytes())
        f.write(tail)
    return path


def write_dzg(path, scans, t0=(0, 3, 20)):
    """A .DZG with one $GSSIS / $GPGGA pair per entry of ``scans``, one second and a few metres apart."""
    with open(path, 'w') as f:
        for k, scan in enumerate(scans):
            sec = t0[2] + k
            f.write('$GSSIS,%d,-1\n' % scan)
            f.write('$GPGGA,%02d%02d%02d,4739.%04d,N,12218.%04d,W,1,07,1.2,%.1f,M,-18.4,M,,*46\n\n'
                    % (t0[0], t0[1] + sec // 60, sec % 60, 2552 + 3 * k, 5815 - 2 * k, 30.0 + 0.5 * k))
    return path


PE_GENERATIONS = ('first', 'v1.2', 'v1.6')


def pe_header_text(generation, snum, tnum, window=300., timezero=13.48, template=None):
    """The .HD text of the three pulseEKKO header generations.  'first' has no ``pulseEKKO`` string (version 1.0, the date
    on line 4, ``\\r\\r\\n`` line ends: ``template`` is such a header, whose counts are replaced); 'v1.2' is a version
    <= 1.5 with the date on line 2 as mm/dd/yyyy; 'v1.6' a version > 1.5 with %Y-%b-%d."""
    if generation == 'first':
        out = []
        for line in template.split('\r\r\n'):
            if line.startswith('NUMBER OF TRACES'):
                line = 'NUMBER OF TRACES   = %d ' % tnum
            elif line.startswith('NUMBER OF PTS/TRC'):
                line = 'NUMBER OF PTS/TRC  = %d ' % snum
            elif line.startswith('TIMEZERO AT POINT'):
                line = 'TIMEZERO AT POINT  = %.2f ' % timezero
            elif line.startswith('TOTAL TIME WINDOW'):
                line = 'TOTAL TIME WINDOW  = %.3f ' % window
            out.append(line)
        return '\r\r\n'.join(out)
    name, date = {'v1.2': ('pulseEKKO 1.2', '04/20/2018'), 'v1.6': ('pulseEKKO 1.6', '2018-Apr-20')}[generation]
    return '\n'.join(['1234', 'Data Collected with ' + name, date, 'NUMBER OF TRACES   = %d' % tnum,
                      'NUMBER OF PTS/TRC  = %d' % snum, 'TIMEZERO AT POINT  = %.2f' % timezero,
                      'TOTAL TIME WINDOW  = %.3f' % window, 'STARTING POSITION  = 0.0000', 'STEP SIZE USED     = 1.0000',
                      'NOMINAL FREQUENCY  = 500.00', 'NUMBER OF STACKS   = 4', ''])


def write_pe(stem, samples, generation, template=None, gps_text=None, **kw):
    """stem.DT1 + stem.HD (+ stem.GPS) with (tnum, snum) samples: int16 for the first generation, float32 after."""
    tnum, snum = samples.shape
    first = generation == 'first'
    with open(stem + '.HD', 'w', newline='') as f:
        f.write(pe_header_text(generation, snum, tnum, template=template, **kw))
    rng = np.random.default_rng(7)
    with open(stem + '.DT1', 'wb') as f:
        for t in range(tnum):
            h = np.zeros((25,), dtype='<f4')
            h[0], h[1], h[2], h[5], h[7], h[8] = t + 1, float(t), snum, 2 if first else 4, 4, kw.get('window', 300.)
            h[3] = rng.uniform(-5, 5)
            h[9:20] = rng.uniform(-100, 100, 11).astype('<f4')
            h[23] = 79832.0 + 0.25 * t
            f.write(h.tobytes())
            f.write(b'c%-27d' % t)
            f.write(np.ascontiguousarray(samples[t], dtype='<i2' if first else '<f4').tobytes())
    if gps_text is not None:
        with open(stem + '.GPS', 'w') as f:
            f.write(gps_text)
    return stem + '.DT1'


def write_tek(path, samples, cut=0):
    """A Tek .DAT with (tnum, 1000) uint16 samples; ``cut`` bytes are taken off its end."""
    tnum = samples.shape[0]
    out = bytearray()
    for t in range(tnum):
        out += struct.pack('<fHhffHH', 190.5 + 0.001 * t, 3 * t, 1000 + 2 * t, 0.002, 2.0e-9, 16, samples.shape[1])
        out += np.ascontiguousarray(samples[t], dtype='<u2').tobytes()
    with open(path, 'wb') as f:
        f.write(bytes(out[:len(out) - cut]))
    return path


# ---------------------------------------------------------------------------------------------------- loaded objects
SKIP_ATTRS = ('fn', '_dev', '_dev_widen', '_picks_struct', 'picks', 'data_dtype', 'gps_data', 'traceheaders', 'flags',
              'stodeep_attrs', 't_srs')
GPS_ATTRS = ('lat', 'lon', 'x', 'y', 'z', 'dist', 'dectime', 'qual', 'sats', 'times', 'scans', 'geo_offset', 'all_data')
TH_ATTRS = ('trace_numbers', 'positions', 'points_per_trace', 'topography', 'bytes_per_point', 'n_stacks', 'time_window',
            'pos', 'receive', 'transmit', 'tz_adjustment', 'zero_flag', 'time_of_day', 'comment_flag', 'comment',
            'header_index')


def _plain(v):
    if v is None:
        return '<None>'
    if isinstance(v, (datetime.datetime, datetime.date)):
        return 'datetime:' + v.isoformat()
    a = np.asarray(v)
    if a.dtype.kind == 'O':
        return np.array([str(x) for x in a.ravel()]).reshape(a.shape)
    if a.dtype.kind == 'M' or a.dtype.kind == 'm':
        return a.astype(np.int64)
    return v


def flatten_object(dat):
    """Every attribute of a loaded RadarData as a dict for ``np.savez``: ``gps.*`` for the gps_data object,
    ``th.*`` for the pulseEKKO trace headers, ``flags.*``; None as '<None>'; the file name left out."""
    out = {}
    for k, v in vars(dat).items():
        if k in SKIP_ATTRS:
            continue
        out[k] = _plain(v)
    out['data.dtype'] = str(np.asarray(dat.data).dtype)
    for k in dat.flags.attrs:
        out['flags.' + k] = _plain(getattr(dat.flags, k))
    gps = getattr(dat, 'gps_data', None)
    if gps is not None:
        for k in GPS_ATTRS:
            if getattr(gps, k, None) is not None:
                out['gps.' + k] = _plain(getattr(gps, k))
    th = getattr(dat, 'traceheaders', None)
    if th is not None:
        for k in TH_ATTRS:
            out['th.' + k] = _plain(getattr(th, k))
    return out


def same_value(got, want):
    """Equal dtype, shape and bits (NaN positions equal); strings by value."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype.kind in 'US' or want.dtype.kind in 'US':
        return got.shape == want.shape and got.dtype.kind == want.dtype.kind and bool(np.all(got == want))
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def object_differences(dat, g):
    """Names of the fixture's entries that the loaded object does not reproduce bit for bit."""
    mine = flatten_object(dat)
    bad = [k for k in g if not k.startswith('_') and (k not in mine or not same_value(mine[k], g[k]))]
    bad += ['+' + k for k in mine if k not in g]
    return bad


# ---------------------------------------------------------------------------------------------------- loader cases
GOLDEN_FILES = ('ten_col.rd3', 'ten_col.rad', 'ten_col.cor', 'ten_col_nogps.rd3', 'ten_col_nogps.rad', 'test_tek.DAT',
                'test_gssi.DZT', 'test_gssi.DZG')
RAW_MAT_CASES = {'ramac': 'LD_R1_ramac_cor', 'tek': 'LD_T1_tek', 'gssi': 'LD_G2_gssi16_dzg', 'pe': 'LD_P1_first_i16_gps'}


def _counts(bits, snum, tnum, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << bits, (tnum, snum), dtype=np.uint64)
    a[0, 0], a[-1, -1] = 0, (1 << bits) - 1
    return a.astype('<u%d' % (bits // 8))


def loader_cases(tmp, golden):
    """Make every file of the loader cases under ``tmp`` (the reference's sample files are copied from ``golden``);
    returns {fixture name: (filetype, file name)}, in the order the fixtures are made."""
    for name in GOLDEN_FILES:
        with open(os.path.join(golden, name), 'rb') as src, open(os.path.join(tmp, name), 'wb') as dst:
            dst.write(src.read())
    with open(os.path.join(golden, 'test_pe.HD'), newline='') as f:
        template = f.read()
    with open(os.path.join(golden, 'test_pe.GPS')) as f:
        gps_text = f.read()
    j = lambda name: os.path.join(tmp, name)                                     # noqa: E731
    cases = collections.OrderedDict()
    cases['LD_R1_ramac_cor'] = ('ramac', j('ten_col.rd3'))
    cases['LD_R2_ramac_nocor'] = ('ramac', j('ten_col_nogps.rd3'))
    cases['LD_T1_tek'] = ('tek', j('test_tek.DAT'))
    cases['LD_G1_gssi32_sample'] = ('gssi', j('test_gssi.DZT'))
    write_dzt(j('g16.DZT'), _counts(16, 33, 70, 1), 16, range_ns=80., trig=3, chan=2)
    write_dzg(j('g16.DZG'), [1, 12, 23, 34, 45, 56, 67])
    cases['LD_G2_gssi16_dzg'] = ('gssi', j('g16.DZT'))
    write_dzt(j('g16n.DZT'), _counts(16, 65, 9, 2), 16, range_ns=120., when=datetime.datetime(1980, 1, 1))
    cases['LD_G3_gssi16_nodzg'] = ('gssi', j('g16n.DZT'))
    k = 0
    for gen in PE_GENERATIONS:
        for with_gps in (True, False):
            k += 1
            first = gen == 'first'
            name = 'LD_P%d_%s_%s_%s' % (k, gen.replace('.', ''), 'i16' if first else 'f32', 'gps' if with_gps else 'nogps')
            snum, tnum = (137, 41) if with_gps else (63, 5)
            rng = np.random.default_rng(10 + k)
            samples = rng.integers(-3000, 3000, (tnum, snum)) + 500 if first else \
                (1000. * rng.standard_normal((tnum, snum)) + 40.).astype(np.float32)
            cases[name] = ('pe', write_pe(j('pe%d' % k), samples, gen, template=template,
                                          gps_text=gps_text if with_gps else None))
    cases['LD_P7_v16_f32_binades_nan'] = ('pe', write_pe(j('pe7'), samples_for(F32, 137, 5, 77), 'v1.6'))
    cases['LD_P8_first_i16_wrap'] = ('pe', write_pe(j('pe8'), samples_for(I16, 101, 4, 78), 'first', template=template))
    return cases


def error_cases(tmp, golden):
    """{name: (filetype, file name)} of files the reference's readers refuse."""
    with open(os.path.join(golden, 'test_pe.HD'), newline='') as f:
        template = f.read()
    j = lambda name: os.path.join(tmp, name)                                     # noqa: E731
    out = collections.OrderedDict()
    write_dzt(j('zpart.DZT'), _counts(16, 33, 4, 3), 16, tail=b'\0' * 10)
    out['gssi_partial_last_trace'] = ('gssi', j('zpart.DZT'))
    write_dzt(j('zs2.DZT'), _counts(16, 2, 6, 4), 16)
    out['gssi_snum_2'] = ('gssi', j('zs2.DZT'))
    for ext in ('rd3', 'rad'):
        with open(os.path.join(golden, 'ten_col_nogps.' + ext), 'rb') as src, open(j('zextra.' + ext), 'wb') as dst:
            dst.write(src.read() + (b'\0\0' if ext == 'rd3' else b''))
    out['ramac_two_extra_bytes'] = ('ramac', j('zextra.rd3'))
    write_tek(j('zcut.DAT'), _counts(16, 1000, 6, 5), cut=1000)
    out['tek_cut_inside_a_record'] = ('tek', j('zcut.DAT'))
    write_pe(j('znohd'), np.zeros((3, 9), dtype=np.int16), 'first', template=template)
    os.remove(j('znohd.HD'))
    out['pe_missing_hd'] = ('pe', j('znohd.DT1'))
    write_pe(j('znogga'), np.zeros((3, 9), dtype=np.int16), 'first', template=template,
             gps_text='Trace #1 at position 0.000000\n$GPRMC,221032.00,A,4820.9,N,12102.7,W,0.0,0.0,200418,,*67\n')
    out['pe_gps_without_gga'] = ('pe', j('znogga.DT1'))
    return out
