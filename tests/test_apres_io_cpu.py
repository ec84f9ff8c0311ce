"""ApRES files in and out without a GPU: the containers, the burst header, the ``.DAT`` and ``.mat`` loaders, ``save``,
the pair and quad loaders and the ``apdar`` command line, held to the ``AI_*`` fixtures that
``tests/golden/make_golden_apres_io.py`` recorded from the reference on the files of ``apres_io_ref.py``'s writer.

An object equals its fixture when it has the same attributes (``flags.*`` and ``header.*`` included, file names apart)
and each has the fixture's dtype, shape and bits.  The device steps are replaced by the NumPy restatements of
``apres_ref.py``; ``range_counts``, the route of an acquisition that still holds its counts, by the restatement on
the NumPy decode."""
import contextlib
import json
import os
import shutil
from unittest.mock import patch

import numpy as np
import pytest
from scipy.io import loadmat, savemat

import apres_io_ref as io
import apres_ref as ref
from conftest import GOLDEN, golden
from impdar_amd import apres as apm
from impdar_amd.bin import apdar
from impdar_amd.lib.ApresData import (ApresData, ApresQuadPol, ApresTimeDiff, load_apres, load_quadpol,
                                      load_time_diff)
from impdar_amd.lib.ApresData.ApresFlags import ApresFlags, QuadPolFlags, TimeDiffFlags
from impdar_amd.lib.ApresData.ApresHeader import ApresHeader
from impdar_amd.lib.ImpdarError import ImpdarError
from test_apres_cpu import kernels_in_numpy, same_bits

EXC = {'ValueError': ValueError, 'TypeError': TypeError, 'IndexError': IndexError, 'ImpdarError': ImpdarError,
       'ImportError': ImportError, 'FileNotFoundError': FileNotFoundError}
MATS = {'raw': ApresData, 'proc': ApresData, 'timediff': ApresTimeDiff, 'quadpol': ApresQuadPol}


def range_counts_in_numpy(counts, divisor, t, chunk=0):
    return ref.range_rows(io.decode(counts.reshape(-1, t.snum), divisor), t)


def chain_in_numpy(dat, p, max_range=4000, winfun='blackman', num_chirps=None, d_raw=None):
    apm.apres_range(dat, p, max_range, winfun)
    apm.stacking(dat, num_chirps)


@contextlib.contextmanager
def host_only():
    with kernels_in_numpy(), patch.object(apm, 'range_counts', range_counts_in_numpy), patch.object(apm, 'chain', chain_in_numpy):
        yield


def mat(name):
    return os.path.join(GOLDEN, 'AI_%s.mat' % name)


# ------------------------------------------------------------------------------------------------ header
@pytest.mark.parametrize('name', sorted(io.HEADER_CASES))
def test_header_parameters_are_the_references(tmp_path, name):
    g = golden('AI_' + name)
    fn = io.write_dat(tmp_path / (name + '.DAT'), [io.burst_bytes(io.counts_of(1, 8), **io.HEADER_CASES[name])])
    h = ApresHeader()
    if '_exc_type' in g:
        with pytest.raises(EXC[g['_exc_type'].item()]) as e:
            h.update_parameters(fn)
        assert str(e.value) == g['_message'].item()
        return
    h.update_parameters(fn)
    got = {k: io._plain(v) for k, v in vars(h).items() if k not in io.HEADER_SKIP}
    assert sorted(got) == sorted(g)
    for k in g:
        assert io.same_value(got[k], g[k]), (k, got[k], g[k])
    assert h.fn == fn


def test_header_cases_take_every_branch():
    g = {k: golden('AI_' + k) for k in io.HEADER_CASES}
    assert [g[k]['ramp_dir'].item() for k in ('H1_up', 'H2_down', 'H3_updown')] == ['up', 'down', 'upDown']
    assert 'nchirpsPerPeriod' in g['H3_updown'] and 'nchirpsPerPeriod' not in g['H1_up']
    assert float(g['H4_fsmode1']['fs']) == 4e4                     # the reference never selects 80 kHz
    assert float(g['H5_chirp_longer_than_record']['chirp_length']) == 101 / 4e4
    assert int(g['H6_chirp_shorter_than_record']['nchirp_samples']) <= 60000
    assert [int(g[k]['file_format']) for k in ('H1_up', 'H7_format4', 'H8_format3', 'H9_format2')] == [5, 4, 3, 2]
    assert g['H10_format_unknown']['_exc_type'].item() == 'ImpdarError'
    h = ApresHeader()
    with pytest.raises(TypeError, match='Must input file name'):
        h.update_parameters()


def test_header_and_flags_defaults_and_matlab_round_trip(tmp_path):
    h = ApresHeader()
    assert (h.fsysclk, h.fs) == (1e9, 4e4) and len(h.attrs) == 30 == len(h.attr_dims)
    assert all(getattr(h, k) is None for k in h.attrs[2:])
    assert np.isnan(h.to_matlab()['f0']) and 'attrs' in h.to_matlab()
    f = ApresFlags()
    assert (f.file_read_code, f.range, f.stack, f.uncertainty) == (None, 0, 0, False)
    t = TimeDiffFlags()
    assert t.phase_diff is False and t.strain.shape == (2,) and t.attr_dims == [None, None, None, 2, None]
    q = QuadPolFlags()
    assert q.cpe is True and q.coherence.shape == (3,) and q.attrs == ['rotation', 'coherence', 'phasegradient', 'cpe']
    t.strain = np.array([1.5, 2.5])
    savemat(str(tmp_path / 'f.mat'), {'flags': t.to_matlab(), 'q': q.to_matlab()})
    m = loadmat(str(tmp_path / 'f.mat'))
    back, qback = TimeDiffFlags(), QuadPolFlags()
    back.from_matlab(m['flags'])
    qback.from_matlab(m['q'])
    assert np.array_equal(back.strain, [1.5, 2.5]) and np.isnan(back.file_read_code)
    assert np.array_equal(qback.rotation, np.zeros(2)) and qback.cpe == 1


# ------------------------------------------------------------------------------------------------ .DAT
@pytest.mark.parametrize('name', sorted(io.DAT_CASES))
def test_dat_files_load_to_the_references_object(tmp_path, name):
    files = io.DAT_CASES[name]
    fns = io.case_files(str(tmp_path), name, files)
    dat = load_apres.load_apres(fns)
    counts, divisor = dat.raw_counts()
    assert counts.shape == (dat.bnum, dat.cnum, dat.snum) and counts.dtype.itemsize == (4 if files[0].get('average') else 2)
    assert dat.fn == os.path.splitext(fns[0])[0] and dat.header.fn == fns[0]
    io.assert_object_equals(dat, golden('AI_' + name))
    assert dat.raw_counts() is not None                              # reading the volts keeps the counts
    want = np.stack([io.decode(io.payload(b, dat.cnum * dat.snum, counts.dtype), divisor).reshape(dat.cnum, dat.snum)
                     for b in io.case_bursts(files)])
    assert same_bits(dat.data, want)
    dat.data = dat.data
    assert dat.raw_counts() is None


def test_dat_cases_cover_the_shapes():
    g = {k: golden('AI_' + k) for k in io.DAT_CASES}
    assert g['D1_3x2x101']['data'].shape == (1, 6, 101) and g['D2_1x1x64']['data'].shape == (1, 1, 64)
    assert g['D3_average2_uint32']['data'].shape == (1, 1, 101) and int(g['D3_average2_uint32']['header.average']) == 2
    assert g['D4_two_files']['data'].shape == (2, 6, 101) and g['D5_three_files']['data'].shape == (3, 6, 64)
    assert g['D6_two_antennas']['data'].shape == (1, 8, 33)
    assert float(g['D1_3x2x101']['temperature2'][0]) == 510.5 - 512 and float(g['D4_two_files']['temperature1'][1]) == 301.5 - 512
    assert g['D1_3x2x101']['flags.file_read_code'].item() == 'Successful Read'
    # the divisor of the averaged burst is no power of two, and the payload starts with the CR LF
    assert int(g['D3_average2_uint32']['header.n_subbursts']) * int(g['D3_average2_uint32']['header.n_attenuators']) == 6
    assert g['D1_3x2x101']['data'][0, 0, 0] == 0x0A0D * 2.5 / 65536.


def run_error(label, tmp):
    name, _, level = label.partition(':')
    if name in io.DAT_ERRORS:
        files, kw = io.DAT_ERRORS[name]
        fns = io.case_files(tmp, 'E_' + name, files, **kw)
        if level == 'load_apres':
            return load_apres.load_apres(fns)
        return [load_apres.load_apres_single_file(f) for f in fns]
    a, b = os.path.join(tmp, 'tt_a.mat'), os.path.join(tmp, 'tt_b.mat')
    raw = ApresData(mat('raw'))
    raw.save(a)
    if name == 'travel_time_mismatch':
        raw.travel_time = raw.travel_time * 2.
        raw.save(b)
        return load_apres.load_apres([a, b])
    if name in ('check_attrs_none', 'check_attrs_missing'):
        d = ApresData(None)
        if name == 'check_attrs_missing':
            del d.data
        return d.check_attrs()
    if name == 'check_attrs_optional_missing':
        d = ApresData(a)
        del d.lat
        return d.check_attrs()
    return {'timediff_check_attrs_none': lambda: ApresTimeDiff(None).check_attrs(),
            'quadpol_check_attrs_none': lambda: ApresQuadPol(None).check_attrs(),
            'save_extension': lambda: ApresData(a).save(os.path.join(tmp, 'x.txt')),
            'timediff_extension': lambda: ApresTimeDiff(os.path.join(tmp, 'x.txt')),
            'single_file_extension': lambda: load_apres.load_apres_single_file(os.path.join(tmp, 'x.txt'))}[name]()


ERRORS = golden('AI_Z_errors')


@pytest.mark.parametrize('row', range(len(ERRORS['label'])), ids=[str(x) for x in ERRORS['label']])
def test_errors_are_the_references(tmp_path, row):
    label, exc_type, message = (str(ERRORS[k][row]) for k in ('label', 'exc_type', 'message'))
    with pytest.raises(EXC[exc_type]) as e:
        run_error(label, str(tmp_path))
    assert type(e.value) is EXC[exc_type]
    got = ', '.join(str(a) for a in e.value.args) if len(e.value.args) > 1 else str(e.value)
    if label == 'average1:single_file':
        # the reference asks NumPy for a dtype 'float4' (its message); here the TypeError names the mode
        assert message == "data type 'float4' not understood" and 'Average=1' in got
    else:
        assert got.replace(str(tmp_path), '<folder>') == message


def test_the_error_cases_are_all_there():
    labels = set(str(x) for x in ERRORS['label'])
    for name in ('snum_mismatch', 'cnum_mismatch', 'frequencies_mismatch', 'travel_time_mismatch', 'too_short_for_the_loop'):
        assert name + ':load_apres' in labels
    for name in ('format4', 'format3', 'format2', 'format_unknown', 'average1', 'too_short_for_the_loop'):
        assert name + ':single_file' in labels


def test_second_burst_of_a_file_is_walked_to(tmp_path):
    """The reference reads the first burst only; here burst 2 is found behind the first one's payload, against the
    writer's own bytes."""
    specs = [dict(nsub=2, natt=2, snum=300), dict(nsub=2, natt=2, snum=300, stamp='2020-01-02 10:00:00', lat=-70.5)]
    counts = [io.counts_of(31, 1200), io.counts_of(32, 1200)]
    bursts = [io.burst_bytes(c, **s) for c, s in zip(counts, specs)]
    fn = io.write_dat(tmp_path / 'two.DAT', bursts)
    first = load_apres.load_apres([fn])
    second = load_apres.load_apres([fn], burst=2)
    assert same_bits(first.data[0], io.decode(io.payload(bursts[0], 1200)).reshape(4, 300))
    # the second header starts one count before the end of the first payload as the loader counts it: its payload is
    # found from its own marker
    assert same_bits(second.data[0], io.decode(io.payload(bursts[1], 1200)).reshape(4, 300))
    assert np.array_equal(second.data[0].reshape(-1)[1:], io.decode(counts[1])[:-1])
    assert second.bnum == 1 and second.lat[0] == -70.5 and str(second.time_stamp[0]) == '2020-01-02 10:00:00'
    assert first.lat[0] == -78.5
    with pytest.raises(ImpdarError, match='Burst Read Failed.'):        # the padding holds no header
        load_apres.load_apres_single_file(fn, burst=3)
    fn = io.write_dat(tmp_path / 'tight.DAT', bursts, pad=0)
    with pytest.raises(ImpdarError, match='Burst 2 not found in file'):
        load_apres.load_apres_single_file(fn, burst=3)


# ------------------------------------------------------------------------------------------------ .mat
@pytest.mark.parametrize('name', sorted(MATS))
def test_reference_written_mat_loads_saves_and_reloads(tmp_path, name):
    dat = MATS[name](mat(name))
    assert dat.fn == mat(name)
    io.assert_object_equals(dat, golden('AI_M_' + name))
    out = str(tmp_path / 'again.mat')
    dat.save(out)
    io.assert_object_equals(MATS[name](out), golden('AI_M_' + name))
    # what a header holds beyond its `attrs` (average, n_subbursts, chirp_interval) is written by the loader's object and
    # not read back, here as in the reference: the file of a reloaded object lacks those three fields
    compare_mat_files(out, mat(name), header_lost=('average', 'n_subbursts', 'chirp_interval'))


def compare_mat_files(ours, theirs, header_lost=()):
    ours, theirs = loadmat(ours), loadmat(theirs)
    assert sorted(ours) == sorted(theirs)
    for k in theirs:
        if k.startswith('__'):
            continue
        if k in ('flags', 'header'):
            assert ours[k].shape == theirs[k].shape == (1, 1)
            lost = header_lost if k == 'header' else ()
            assert [n for n in theirs[k].dtype.names if n not in lost] == list(ours[k].dtype.names), k
            for kk in ours[k].dtype.names:
                a, b = ours[k][kk][0][0], theirs[k][kk][0][0]
                assert a.shape == b.shape and a.dtype == b.dtype and (kk == 'fn' or a.tobytes() == b.tobytes()), (k, kk)
        else:
            if k not in ('fn', 'fn1', 'fn2'):
                assert ours[k].shape == theirs[k].shape and ours[k].dtype == theirs[k].dtype, k
                assert ours[k].tobytes() == theirs[k].tobytes(), k


def test_saved_dat_acquisition_is_the_references_file(tmp_path):
    """``scipy.io.loadmat`` of a ``.DAT`` acquisition saved here and of the one the reference saved: the same keys,
    struct fields, shapes, dtypes and bytes."""
    fns = io.case_files(str(tmp_path), 'D1_3x2x101', io.DAT_CASES['D1_3x2x101'])
    dat = load_apres.load_apres(fns)
    dat.header.fn = os.path.basename(dat.header.fn)
    out = str(tmp_path / 'raw.mat')
    dat.save(out)
    assert dat.raw_counts() is not None
    compare_mat_files(out, mat('raw'))


def test_save_refuses_other_extensions_and_h5_needs_its_library(tmp_path):
    dat = ApresData(mat('raw'))
    with pytest.raises(ValueError, match=r'File extension choices are \.h5 and \.mat \(legacy\)'):
        dat.save(str(tmp_path / 'x.npy'))
    try:
        import h5py                                                  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError):
            dat.save(str(tmp_path / 'x.h5'))
        with pytest.raises(ImportError):
            ApresData(str(tmp_path / 'x.h5'))
    try:
        import netCDF4                                               # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match='Need the netCDF4 library to load nc files.'):
            load_apres.load_apres_single_file(str(tmp_path / 'x.nc'))


def test_save_casts_back_to_the_loaded_dtype(tmp_path):
    dat = ApresData(mat('raw'))
    dat.data_dtype = np.dtype(np.float32)
    dat.save(str(tmp_path / 'f32.mat'))
    assert loadmat(str(tmp_path / 'f32.mat'))['data'].dtype == np.float32
    dat.data = dat.data.copy()
    dat.data[0, 0, 0] = np.nan
    # (a float16 array is what the int8 / int16 rule hands to savemat, which has no such type and writes doubles)
    for dtype, want in ((np.int16, np.float64), (np.int32, np.float32), (np.int64, np.float64)):
        dat.data_dtype = dtype
        dat.save(str(tmp_path / 'nan.mat'))
        back = loadmat(str(tmp_path / 'nan.mat'))['data']
        assert back.dtype == want and np.isnan(back[0, 0, 0]) and np.isfinite(back[0, 0, 1:]).all()
    dat.data_dtype = np.int16
    dat.data = np.nan_to_num(dat.data)
    dat.save(str(tmp_path / 'int.mat'))
    assert loadmat(str(tmp_path / 'int.mat'))['data'].dtype == np.int16
    none = ApresData(None)
    none.save(str(tmp_path / 'none.mat'))
    assert loadmat(str(tmp_path / 'none.mat'))['data'].item() == 0


def test_datetime_property(tmp_path):
    dat = load_apres.load_apres(io.case_files(str(tmp_path), 'D4', io.DAT_CASES['D4_two_files']))
    assert dat.datetime.dtype.kind == 'M' and dat.datetime.shape == (2,)
    # (the reference's expression, :200-201: Matlab's datenum counts from a day before Python's ordinal, so the stamps
    # 2019-12-25 03:45:10 and 2019-12-26 04:00:00 come back a day early, less the rounding of the day's fraction)
    assert [str(d)[:16] for d in dat.datetime] == ['2019-12-24T03:45', '2019-12-25T03:59']


def test_bas_mat(tmp_path):
    rng = np.random.RandomState(3)
    vif = rng.standard_normal((4, 50))
    t = np.arange(50.) / 4e4
    vdat = {'f0': 2e8, 'fs': 4e4, 'f1': 4e8, 'fc': 3e8, 'Attenuator_1': np.array([30., 10.]), 'Attenuator_2': np.array([-4., -14.]),
            'T': 1., 'K': 2. * np.pi * 2e8, 'B': 2e8, 'lambdac': 0.56, 'er': 3.18, 'ci': 1.68e8, 'Nsamples': 50, 'chirpNum': 4,
            'Burst': 1, 'SubBurstsInBurst': 4, 'Average': 0, 't': t, 'f': 2e8 + t * 2e8, 'chirpAtt': np.full(4, 30. - 4j),
            'TimeStamp': 737784.5, 'vif': vif}
    fn = str(tmp_path / 'bas.mat')
    savemat(fn, {'vdat': vdat})
    for dat in (load_apres.load_BAS_mat(fn), load_apres.load_apres_single_file(fn)):
        assert dat.data.shape == (1, 4, 50) and np.array_equal(dat.data[0], vif)
        assert (dat.snum, dat.cnum, dat.bnum) == (50, 4, 1) and dat.header.fs == 4e4 and dat.dt == 1. / 4e4
        assert np.array_equal(dat.chirp_num, [1, 2, 3, 4]) and dat.decday == 737784.5
        assert np.array_equal(dat.chirp_time, 737784.5 + 1.6384 / 86400. * np.arange(4.))
        assert np.array_equal(np.ravel(dat.travel_time), t) and dat.header.chirp_grad == 2. * np.pi * 2e8
        assert dat.data_dtype == np.float64


def test_quadpol_fujita(tmp_path):
    rng = np.random.RandomState(4)
    model = {k: rng.standard_normal(40) + 1j * rng.standard_normal(40) for k in ('shh', 'shv', 'svh', 'svv')}
    model.update(range=np.arange(40.) * 2., c=3e8, epsr=3.12)
    fn = str(tmp_path / 'model.mat')
    savemat(fn, model)

    class Model(object):
        pass
    obj = Model()
    vars(obj).update(model)
    for qp in (load_quadpol.load_quadpol_fujita(fn), load_quadpol.load_quadpol_fujita(obj)):
        assert qp.snum == 40 and all(np.array_equal(getattr(qp, k), model[k]) for k in ('shh', 'shv', 'svh', 'svv', 'range'))
        assert np.array_equal(qp.travel_time, model['range'] / (3e8 / np.sqrt(3.12)))
        assert qp.dt == np.mean(np.gradient(qp.travel_time)) and qp.data_dtype == np.complex128 and qp.decday > 737000


# ------------------------------------------------------------------------------------------------ pair and quad
def pair_fields(diff, a, b):
    assert same_bits(diff.data, a.data.flatten().astype(complex)) and same_bits(diff.data2, b.data.flatten().astype(complex))
    assert same_bits(diff.range, a.Rcoarse) and diff.snum == a.snum and diff.dt == a.dt
    assert same_bits(diff.unc1, a.uncertainty) and same_bits(diff.unc2, b.uncertainty)
    assert diff.fn1 == a.header.fn and diff.fn == diff.fn1 + '_diff_' + diff.fn2 and diff.data_dtype == np.complex128
    assert type(diff.flags) is TimeDiffFlags and diff.flags.file_read_code == a.flags.file_read_code
    assert same_bits(np.asarray(diff.header.f0), np.asarray(a.header.f0))


def test_time_diff_loader_forms_and_errors(tmp_path, capsys):
    for t in ('time1', 'time2'):
        shutil.copy(mat('proc'), str(tmp_path / ('site_%s_proc.mat' % t)))
    proc = ApresData(mat('proc'))
    names = (str(tmp_path / 'site_time1_proc.mat'), str(tmp_path / 'site_time2_proc.mat'))
    with host_only():
        for form in (str(tmp_path / 'site'), names, list(names), (ApresData(names[0]), ApresData(names[1]))):
            pair_fields(load_time_diff.load_time_diff(form), proc, proc)
    assert 'Restacked acquisition #1 to a 1-d array.' in capsys.readouterr().out
    shutil.copy(mat('proc'), str(tmp_path / 'site_time2_other.mat'))
    with pytest.raises(FileNotFoundError, match='Need exactly one file matching each time acqusition'):
        load_time_diff.load_time_diff(str(tmp_path / 'site'))
    with pytest.raises(FileNotFoundError):
        load_time_diff.load_time_diff(str(tmp_path / 'nothing'))
    with pytest.raises(ValueError, match='fn must be a glob for files with _time1, _time2, or a 2-tuple'):
        load_time_diff.load_time_diff(names + names[:1])
    short = ApresData(names[0])
    short.data, short.snum, short.travel_time = short.data[:, :, :-1], short.snum - 1, short.travel_time
    with host_only(), pytest.raises(ValueError, match='Need the same number of vertical samples in each file'):
        load_time_diff.load_time_diff((ApresData(names[0]), short))
    other = ApresData(names[0])
    other.travel_time = other.travel_time * 2.
    with host_only(), pytest.raises(ValueError, match='Need matching travel time vectors'):
        load_time_diff.load_time_diff((ApresData(names[0]), other))
    saved = ApresTimeDiff(mat('timediff'))
    io.assert_object_equals(load_time_diff.load_time_diff(mat('timediff'), load_single_acquisitions=False), golden('AI_M_timediff'))
    assert saved.data.ndim == 1 and saved.data.dtype == np.complex128


def test_pair_of_raw_files_is_stacked_and_ranged(tmp_path):
    """Acquisitions that are neither stacked nor converted: the loader does both, pad factor 2, the reference's order
    (stacking first, on the raw chirps)."""
    fns = io.flow_files(str(tmp_path))
    with host_only():
        diff = load_time_diff.load_time_diff((fns[0], fns[1]))
        want = []
        for fn in fns:
            dat = load_apres.load_apres([fn])
            apm.stacking(dat)
            apm.apres_range(dat, 2)
            want.append(dat)
    assert want[0].data.shape == (1, 1, want[0].snum) and want[0].flags.stack == 6 and want[0].flags.range == 4000
    assert same_bits(diff.data, want[0].data.flatten()) and same_bits(diff.data2, want[1].data.flatten())
    assert same_bits(diff.range, want[0].Rcoarse) and diff.unc1 is None


def test_quadpol_loader_forms_and_errors(tmp_path):
    for pol in ('HH', 'HV', 'VH', 'VV'):
        shutil.copy(mat('proc'), str(tmp_path / ('site_%s.mat' % pol)))
    proc = ApresData(mat('proc'))
    names = [str(tmp_path / ('site_%s.mat' % pol)) for pol in ('HH', 'HV', 'VH', 'VV')]
    with host_only():
        for form in (str(tmp_path / 'site'), names, tuple(names)):
            qp = load_quadpol.load_quadpol(form)
            for k in ('shh', 'shv', 'svh', 'svv', 'data'):
                assert same_bits(getattr(qp, k), proc.data.flatten().astype(np.cdouble)), k
            assert same_bits(qp.range, proc.Rcoarse) and same_bits(qp.travel_time, proc.travel_time) and qp.snum == proc.snum
            assert type(qp.flags) is QuadPolFlags and qp.flags.file_read_code == proc.flags.file_read_code
            assert qp.data_dtype == np.complex128 and qp.header.fn == proc.header.fn
    os.remove(names[2])
    with pytest.raises(FileNotFoundError, match='Need exactly one file matching each polarization'):
        load_quadpol.load_quadpol(str(tmp_path / 'site'))
    with pytest.raises(ValueError, match='fn must be a glob for files with _HH, _HV, etc., or a 4-tuple'):
        load_quadpol.load_quadpol(names[:3])
    io.assert_object_equals(load_quadpol.load_quadpol(mat('quadpol'), load_single_pol=False), golden('AI_M_quadpol'))
    g = golden('AI_F3_qp')
    qp = ApresQuadPol(mat('quadpol'))
    for k in ('shh', 'shv', 'svh', 'svv', 'range', 'travel_time'):
        assert same_bits(getattr(qp, k), g[k]), k


def test_methods_are_the_packages_functions():
    for cls, names in ((ApresData, ('apres_range', 'stacking', 'phase_uncertainty', 'save')),
                       (ApresTimeDiff, ('phase_diff', 'phase_unwrap', 'range_diff', 'strain_rate', 'bed_pick', 'save')),
                       (ApresQuadPol, ('rotational_transform', 'coherence2d', 'phase_gradient2d', 'find_cpe',
                                       'phase_gradient_to_fabric', 'save'))):
        assert all(callable(getattr(cls, k)) for k in names)
    assert ApresData.apres_range is apm.apres_range and ApresTimeDiff.bed_pick is apm.bed_pick


def test_counts_route_and_float_route_agree_on_the_host(tmp_path):
    """With the kernels in NumPy both routes of ``apres_range`` run the same restatement on the same volts."""
    fns = io.flow_files(str(tmp_path))
    a, b = load_apres.load_apres(fns), load_apres.load_apres(fns)
    b.data = b.data.copy()
    assert a.raw_counts() is not None and b.raw_counts() is None
    with host_only():
        a.apres_range(2, 4000.)
        b.apres_range(2, 4000.)
    assert a.raw_counts() is None and a.data_dtype == np.complex128
    for k in ('data', 'spec', 'Rfine', 'Rcoarse'):
        assert same_bits(getattr(a, k), getattr(b, k)), k


# ------------------------------------------------------------------------------------------------ apdar
def test_apdar_parses_to_the_references_defaults():
    want = json.loads(golden('AI_P_apdar')['json'].item())
    parser = apdar._get_args()
    assert sorted(want) == sorted(io.APDAR_COMMANDS)
    for cmd in io.APDAR_COMMANDS:
        args = vars(parser.parse_args([cmd, 'x.mat']))
        args['func'] = args['func'].__name__
        assert json.loads(json.dumps(args)) == want[cmd], cmd
    args = parser.parse_args(['proc', '-max_range', '150', '-num_chirps', '4', 'a.mat', 'b.mat', '-o', 'out.mat'])
    assert (args.max_range, args.num_chirps, args.fns, args.o) == (150., 4, ['a.mat', 'b.mat'], 'out.mat')
    with pytest.raises(SystemExit):
        parser.parse_args(['load', '-acq_type', 'triple', 'x'])


def test_apdar_output_names():
    assert apdar.output_name(['a.DAT', 'b.DAT'], 'apraw') == 'a_apraw.mat'
    assert apdar.output_name(['dir/a_apraw.mat'], 'proc') == 'dir/a_proc.mat'
    assert apdar.output_name(['a_tdraw.mat'], 'diffproc') == 'a_diffproc.mat'
    assert apdar.output_name(['a_proc.mat'], 'stacked') == 'a_proc_stacked.mat'
    assert apdar.output_name(['a.mat'], 'proc', o='given.mat') == 'given.mat'
    parser = apdar._get_args()
    assert parser.parse_args(['unwrap', 'x']).name == 'proc' == parser.parse_args(['rdiff', 'x']).name


def test_apdar_plot_raises_and_fallback_reports_every_attempt(tmp_path):
    with pytest.raises(NotImplementedError, match='apdar plot'):
        apdar.main(['plot', 'x.mat'])
    bad = str(tmp_path / 'x.txt')
    with pytest.raises(ImpdarError) as e:
        apdar.load(fns=[bad])
    for kind in ('single: ', 'timediff: ', 'quadpol: '):
        assert kind in str(e.value)
    # the single attempt says why the file did not load, not only that none was left
    assert 'Expecting a certain filetype; either .mat, .h5, .dat, .DAT, .nc' in str(e.value)
    short = io.case_files(str(tmp_path), 'short', io.DAT_ERRORS['too_short_for_the_loop'][0], pad=100)
    with pytest.raises(ImpdarError, match='Burst 0 not found in file'):
        apdar.load(fns=short)
    with pytest.raises(ImpdarError):
        apdar.main(['stack', bad])


def test_apdar_load_then_proc_on_the_host(tmp_path):
    fns = io.flow_files(str(tmp_path))
    apdar.main(['load', '-acq_type', 'single'] + fns)
    raw = str(tmp_path / 'flow_0_apraw.mat')
    back = ApresData(raw)
    assert back.data.shape == (2, 6, 1001) and same_bits(back.data, load_apres.load_apres(fns).data)
    g = golden('AI_F1_flow')
    assert same_bits(back.data, g['raw'])
    np.random.seed(5)
    with host_only(), np.errstate(invalid='ignore'):
        apdar.main(['proc', raw])
        apdar.main(['range', raw, '-o', str(tmp_path / 'r.mat')])
        apdar.main(['stack', str(tmp_path / 'r.mat')])
    proc = ApresData(str(tmp_path / 'flow_0_proc.mat'))
    assert proc.data.shape == g['stacked'].shape and proc.flags.stack == 12 and proc.flags.range == 4000.
    assert same_bits(proc.Rcoarse, g['Rcoarse']) and proc.uncertainty.shape == g['uncertainty'].shape
    assert np.max(np.abs(proc.data - g['stacked'])) <= 1e-9 * np.max(np.abs(g['stacked']))
    assert ApresData(str(tmp_path / 'r_stacked.mat')).data.shape == (1, 1, proc.snum)
    # the three-way fallback takes a saved pair for what it is
    shutil.copy(mat('timediff'), str(tmp_path / 'pair_tdraw.mat'))
    with host_only():
        apdar.main(['pdiff', str(tmp_path / 'pair_tdraw.mat')])
    assert ApresTimeDiff(str(tmp_path / 'pair_pdiff.mat')).co.shape == golden('AI_F2_pdiff')['co'].shape


# ------------------------------------------------------------------------------------------------ the full pair and quad flows
def test_apdar_diffproc_on_the_references_pair(tmp_path):
    """``apdar diffproc`` with its defaults on the pair the reference saved, the phase difference in NumPy: the
    reference's ``time_diff_processing`` on the same bits at the bars of ``check_diff`` and ``check_time_diff``."""
    from test_apres_io_gpu import check_pair
    out = str(tmp_path / 'pair_diffproc.mat')
    with host_only():
        apdar.main(['diffproc', mat('bed_tdraw'), '-o', out])
    check_pair(ApresTimeDiff(out), golden('AI_B1_diffproc'))
    with host_only():
        apdar.main(['diffproc', mat('bed_tdraw'), '-window', '40', '-step', '10', '-w_surf', '-0.3', '-o', out])
    other = ApresTimeDiff(out)
    assert np.array_equal(other.flags.phase_diff, [40, 10]) and len(other.co) == len(apm.phase_diff_windows(other.snum, 40, 10)) == 296


def test_apdar_qpproc_on_the_references_quad(tmp_path):
    from test_apres_flows_cpu import kernels_in_numpy as quad_kernels_in_numpy
    from test_apres_io_gpu import check_quad
    out = str(tmp_path / 'quad_qpproc.mat')
    with quad_kernels_in_numpy():
        apdar.main(['qpproc', mat('bed_qpraw'), '-nthetas', '24', '-o', out])
    check_quad(ApresQuadPol(out), golden('AI_B2_qpproc'))
