"""What the ApRES file tests share: a writer of synthetic RMB2 burst files (the project's own code: the layout is the
instrument's, an ASCII header of ``key=value`` lines ended by CR LF, the marker ``*** End Header ***``, CR LF, then the
counts), the NumPy decode of the counts, and the comparison of a loaded object with a fixture.

The loader, like the reference, takes the payload from the byte right after the marker: the CR LF is its first
sample (0x0A0D) and the last of the written counts is not read.  :func:`payload` gives what is read."""
import numpy as np

MARKER = b'*** End Header ***'
# the instrument's usual chirp: 200 to 400 MHz in 40000 steps of 5 kHz, one every 25 us
REGS = {'Reg00': '00000008', 'Reg01': '000C0820', 'Reg02': '0D1F41C8', 'Reg0B': '6666666633333333',
        'Reg0C': '000053E3000053E3', 'Reg0D': '186A186A'}
PAD = 2100       # bytes after the last payload: the loader looks for a burst only where 2000 bytes or more follow


def header_text(nsub=3, natt=2, snum=101, average=0, att1='30,10,0,0', afgain='-4,-14,0,0', tx='1,0,0,0,0,0,0,0',
                rx='1,0,0,0,0,0,0,0', fsmode=0, stamp='2019-12-25 03:45:10', lat=-78.5, lon=112.25, temp1=24.1875,
                temp2=510.5, volt=12.36, regs=None, fmt=5, drop=()):
    """The ASCII header of one burst.  ``fmt`` 5 carries ``SW_Issue=``; 4 ``SubBursts in burst:`` in its place; 3 the
    burst-header line alone; 2 ``RADAR TIME``; None none of the keywords.  ``drop`` leaves keys out."""
    regs = dict(REGS, **(regs or {}))
    lines = ['', {5: '*** Burst Header ***', 4: '*** Burst Header ***', 3: '*** Burst Header ***', 2: 'RADAR TIME',
                  None: 'Header'}[fmt],
             'Time stamp=%s' % stamp, 'RMB_Issue=1d', 'VAB_Issue=C']
    if fmt == 5:
        lines.append('SW_Issue=101.2')
    if fmt == 4:
        lines.append('SubBursts in burst:%d' % nsub)
    lines += ['Venom_Issue=0.1.3', 'Alternate=0', 'NSubBursts=%d' % nsub, 'Average=%d' % average, 'N_ADC_SAMPLES=%d' % snum,
              'SamplingFreqMode=%d' % fsmode, 'nAttenuators=%d' % natt, 'Attenuator1=%s' % att1, 'AFGain=%s' % afgain,
              'TxAnt=%s' % tx, 'RxAnt=%s' % rx]
    lines += ['%s="%s"' % (k, regs[k]) for k in ('Reg00', 'Reg01', 'Reg02', 'Reg0B', 'Reg0C', 'Reg0D')]
    lines += ['Latitude=%s' % lat, 'Longitude=%s' % lon, 'Temp1=%s' % temp1, 'Temp2=%s' % temp2, 'BatteryVoltage=%s' % volt]
    lines = [ln for ln in lines if ln.split('=')[0] + '=' not in drop]
    return ('\r\n'.join(lines) + '\r\n').encode('ascii')


def counts_of(seed, n, average=0):
    """``n`` seeded counts with both ends of the range among them: uint16, or uint32 for ``Average=2``."""
    rng = np.random.RandomState(seed)
    if average == 2:
        c = rng.randint(0, 2**32, size=n, dtype=np.uint64).astype('<u4')
        c[:3] = (0, 2**32 - 1, 65535)[:len(c[:3])]
    else:
        c = rng.randint(0, 2**16, size=n).astype('<u2')
        c[:2] = (0, 65535)[:len(c[:2])]
    return c


def chirp_counts(seed, cnum, snum, tones=((0.021, 2000.), (0.083, 800.), (0.19, 300.)), noise=400.):
    """uint16 counts of ``cnum`` chirps that look like an instrument's: a few beat tones on mid-scale, the same in every chirp, with
    noise strong enough that no range bin is small against the rounding of the strongest (``check_range`` needs that)."""
    rng = np.random.RandomState(seed)
    k = np.arange(snum)
    sig = sum(a * np.cos(2. * np.pi * f * k + 0.3 + 7. * f) for f, a in tones)
    return np.clip(np.rint(32768. + sig[None, :] + noise * rng.standard_normal((cnum, snum))), 0, 65535).astype('<u2').reshape(-1)


def burst_bytes(counts, **header):
    return header_text(**header) + MARKER + b'\r\n' + np.ascontiguousarray(counts).tobytes()


def write_dat(path, bursts, pad=PAD):
    """``bursts``: what :func:`burst_bytes` returned, in file order."""
    with open(str(path), 'wb') as f:
        for b in bursts:
            f.write(b)
        f.write(b'\0' * pad)
    return str(path)


def payload(burst, n, dtype='<u2'):
    """The ``n`` elements the loader reads of one burst: from the byte after the marker."""
    start = burst.index(MARKER) + len(MARKER)
    return np.frombuffer(burst[start:start + n * np.dtype(dtype).itemsize], dtype=dtype)


def decode(counts, divisor=1):
    """The reference's expression (``load_apres.py:392-395``)."""
    volts = counts.astype(float) * 2.5 / 2**16.
    if divisor != 1:
        volts /= divisor
    return volts


# ------------------------------------------------------------------------------------------------ the cases
# name -> one dict of header_text's arguments (and a seed) per file
DAT_CASES = {
    'D1_3x2x101': [dict(seed=1)],
    'D2_1x1x64': [dict(seed=2, nsub=1, natt=1, snum=64, att1='15,0,0,0', afgain='-14,0,0,0')],
    'D3_average2_uint32': [dict(seed=3, average=2)],
    'D4_two_files': [dict(seed=4), dict(seed=5, stamp='2019-12-26 04:00:00', temp1=301.5, volt=12.11)],
    'D5_three_files': [dict(seed=6, snum=64), dict(seed=7, snum=64, lat=-78.75), dict(seed=8, snum=64, temp2=20.25)],
    'D6_two_antennas': [dict(seed=9, nsub=2, natt=1, snum=33, tx='1,1,0,0,0,0,0,0', rx='1,0,1,0,0,0,0,0')],
}
# name -> the files of a load_apres call that the reference refuses
DAT_ERRORS = {
    'snum_mismatch': ([dict(seed=1), dict(seed=2, snum=64)], {}),
    'cnum_mismatch': ([dict(seed=1), dict(seed=2, nsub=2)], {}),
    'frequencies_mismatch': ([dict(seed=1), dict(seed=2, regs={'Reg0B': '6666666633333000'})], {}),
    'too_short_for_the_loop': ([dict(seed=1)], dict(pad=100)),
    'average1': ([dict(seed=1, average=1)], {}),
    'format4': ([dict(seed=1, fmt=4)], {}),
    'format3': ([dict(seed=1, fmt=3)], {}),
    'format2': ([dict(seed=1, fmt=2)], {}),
    'format_unknown': ([dict(seed=1, fmt=None)], {}),
}
HEADER_CASES = {
    'H1_up': {},
    'H2_down': dict(regs={'Reg0B': '7333333333333333'}),
    'H3_updown': dict(regs={'Reg01': '000E0820'}),
    'H4_fsmode1': dict(fsmode=1),
    'H5_chirp_longer_than_record': dict(snum=101),
    'H6_chirp_shorter_than_record': dict(snum=60000, regs={'Reg0D': '00010001'}),
    'H7_format4': dict(fmt=4),
    'H8_format3': dict(fmt=3),
    'H9_format2': dict(fmt=2),
    'H10_format_unknown': dict(fmt=None),
}
APDAR_COMMANDS = ('load', 'proc', 'diffproc', 'qpproc', 'range', 'stack', 'uncertainty', 'pdiff', 'unwrap', 'rdiff', 'rotate',
                  'coherence', 'cpe', 'plot')
FLOW = dict(snum=1001, nsub=3, natt=2, p=2, max_range=4000., noise_bed_range=3000., seeds=(21, 22))


# acquisitions with a bed: one file of 6 chirps x 6300 samples each, 2996 range bins within 4000 m at pad factor 2
BED = dict(snum=6300, nsub=3, natt=2, p=2, max_range=4000., noise_bed_range=3000., bins=2996, bed=2100, sigma=200.,
           slope=1.0e-3, names=('time1', 'time2', 'HH', 'HV', 'VH', 'VV'))


def bed_spectrum(seed, slope=0., noise=0.02):
    """Complex amplitude per range bin of a synthetic site: random phases under a power envelope that falls a decade
    along the record, a bed return (a Gaussian bump of BED['sigma'] bins, 30 x the local level) at bin BED['bed'] and a
    floor 20 x lower below it.  ``slope`` turns the phase along range (a later acquisition of a straining column);
    ``noise`` adds that share of the local level, drawn from ``seed + 500``."""
    n, bed = BED['bins'], BED['bed']
    rng = np.random.RandomState(seed)
    j = np.arange(n)
    base = 10. ** (-0.5 * j / n)
    env = np.where(j < bed, base, base / 20.) + 30. * base[bed] * np.exp(-(j - bed) ** 2. / (2. * BED['sigma'] ** 2.))
    spec = env * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    spec = spec * np.exp(1j * slope * 4. * np.pi * j)
    rng = np.random.RandomState(seed + 500 + int(slope * 1e6))
    spec = spec + noise * env * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    spec[0] = 0.
    return spec


def bed_counts(spec, seed):
    """uint16 counts of BED's chirps whose range conversion at pad factor p has ``spec``'s envelope: the chirp is the
    real series with amplitude ``spec[k]`` at k cycles per p snum samples, on mid-scale, a count of noise per chirp."""
    cnum, snum, N = BED['nsub'] * BED['natt'], BED['snum'], BED['p'] * BED['snum']
    full = np.zeros(N // 2 + 1, dtype=complex)
    full[:len(spec)] = spec
    x = np.fft.irfft(full, N)[:snum]
    x = x * (12000. / np.max(np.abs(x)))
    rng = np.random.RandomState(seed + 900)
    return np.clip(np.rint(32768. + x[None, :] + rng.standard_normal((cnum, snum))), 0, 65535).astype('<u2').reshape(-1)


def bed_files(folder):
    """Two ``.DAT`` files (two bursts of one column, a count of noise apart) per name of BED['names']: site_time1 and
    site_time2 share a column (the second strained and a day later); site_HH ... site_VV are four draws, HV and VH of
    one column with noise of their own."""
    seeds = {'time1': (41, 0.), 'time2': (41, BED['slope']), 'HH': (42, 0.), 'HV': (43, 0.), 'VH': (43, 2.e-6), 'VV': (44, 0.)}
    out = {}
    for i, name in enumerate(BED['names']):
        seed, slope = seeds[name]
        spec = bed_spectrum(seed, slope)
        out[name] = [write_dat('%s/site_%s_%d.DAT' % (folder, name, b),
                               [burst_bytes(bed_counts(spec, seed + 10 * i + b), snum=BED['snum'], nsub=BED['nsub'], natt=BED['natt'],
                                            stamp='2019-12-2%d 03:4%d:10' % (5 + (name == 'time2'), b))]) for b in range(2)]
    return out


def n_counts(nsub=3, natt=2, snum=101, average=0, tx='1,0,0,0,0,0,0,0', rx='1,0,0,0,0,0,0,0', **others):
    if average:
        return snum
    return nsub * natt * tx.split(',').count('1') * rx.split(',').count('1') * snum


def case_bursts(files):
    """One burst (bytes) per file of a case."""
    out = []
    for spec in files:
        spec = dict(spec)
        seed = spec.pop('seed')
        out.append(burst_bytes(counts_of(seed, n_counts(**spec), spec.get('average', 0)), **spec))
    return out


def case_files(folder, name, files, pad=PAD):
    return [write_dat('%s/%s_%d.DAT' % (folder, name, i), [b], pad=pad) for i, b in enumerate(case_bursts(files))]


def flow_files(folder, stem='flow', seeds=None):
    """Two files of FLOW's shape with instrument-like chirps."""
    cnum = FLOW['nsub'] * FLOW['natt']
    return [write_dat('%s/%s_%d.DAT' % (folder, stem, i),
                      [burst_bytes(chirp_counts(seed, cnum, FLOW['snum']), snum=FLOW['snum'], nsub=FLOW['nsub'], natt=FLOW['natt'],
                                   stamp='2019-12-2%d 03:45:10' % (5 + i))])
            for i, seed in enumerate(seeds or FLOW['seeds'])]


# ------------------------------------------------------------------------------------------------ objects and fixtures
HEADER_SKIP = ('attrs', 'attr_dims', 'fn')


def _plain(v):
    """A value as something ``np.savez`` stores without pickling."""
    if v is None:
        return '<None>'
    if isinstance(v, np.dtype):
        return 'dtype:' + str(v)
    a = np.asarray(v)
    if a.dtype.kind == 'O':
        return np.array([str(x) for x in a.ravel()]).reshape(a.shape)
    return v


def flatten_object(dat, prefix=''):
    """Every attribute of a loaded object as a dict of arrays for ``np.savez``: ``flags`` and ``header`` under
    ``flags.`` / ``header.``; None as the string '<None>'; file names, which hold a directory, left out."""
    out = {}
    for k, v in vars(dat).items():
        if k in ('_data', '_counts', '_counts_divisor'):
            continue
        if k in ('flags', 'header'):
            for kk, vv in vars(v).items():
                if kk not in HEADER_SKIP:
                    out['%s.%s' % (k, kk)] = _plain(vv)
        elif k not in ('fn', 'fn1', 'fn2'):
            out[prefix + k] = _plain(v)
    if 'data' not in out:
        out['data'] = _plain(dat.data)
    return out


def same_value(got, want):
    """Equal type kind, dtype, shape and bits (NaN equal to NaN)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype.kind in 'US' or want.dtype.kind in 'US':
        return got.shape == want.shape and got.dtype.kind == want.dtype.kind and bool(np.all(got == want))
    if got.dtype.kind == 'O' or want.dtype.kind == 'O':
        return got.shape == want.shape and bool(np.all(got == want))
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def assert_object_equals(dat, g, skip=()):
    got = flatten_object(dat)
    want = {k: g[k] for k in g if not k.startswith('_')}
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    for k in want:
        if k not in skip:
            assert same_value(got[k], want[k]), (k, got[k], want[k])
