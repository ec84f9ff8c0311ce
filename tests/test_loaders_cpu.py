"""The instrument loaders (impdar_amd.lib.loaders, lib.gpslib, rawload.decode_host) against the LD_* fixtures that
tests/golden/make_golden_loaders.py recorded from the reference's readers: every attribute bit for bit.  Host code is
NumPy and SciPy on both sides, so there is no tolerance.  No GPU."""
import json
import os
import struct

import numpy as np
import pytest

import rawload_ref as R
from conftest import GOLDEN, golden

INT64_MAX = (1 << 63) - 1


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('loaders'))
    return R.loader_cases(tmp, GOLDEN), R.error_cases(tmp, GOLDEN)


@pytest.fixture(scope='module')
def loaded(files):
    from impdar_amd.lib import loaders
    return {name: loaders.load(filetype, fn)[0] for name, (filetype, fn) in files[0].items()}


CASES = ['LD_R1_ramac_cor', 'LD_R2_ramac_nocor', 'LD_T1_tek', 'LD_G1_gssi32_sample', 'LD_G2_gssi16_dzg', 'LD_G3_gssi16_nodzg',
         'LD_P1_first_i16_gps', 'LD_P2_first_i16_nogps', 'LD_P3_v12_f32_gps', 'LD_P4_v12_f32_nogps', 'LD_P5_v16_f32_gps',
         'LD_P6_v16_f32_nogps', 'LD_P7_v16_f32_binades_nan', 'LD_P8_first_i16_wrap']


def test_the_case_table_is_the_fixtures(files):
    assert list(files[0]) == CASES
    for name in CASES:
        assert os.path.exists(os.path.join(GOLDEN, name + '.npz'))


@pytest.mark.parametrize('name', CASES)
def test_every_attribute_equals_the_reference(loaded, name):
    g = golden(name)
    dat = loaded[name]
    assert R.object_differences(dat, g) == []
    assert str(dat.data.dtype) == str(g['data.dtype']) and dat.data_dtype == dat.data.dtype
    assert dat._dev is None


@pytest.mark.parametrize('name', CASES)
def test_the_restatement_equals_the_fixture(files, name):
    """tests/rawload_ref.py's trace-by-trace decode, the GPU sweep's expected value, is the reference's data."""
    from impdar_amd import rawload
    filetype, fn = files[0][name]
    g = golden(name)
    snum, tnum = g['data'].shape
    stem = os.path.splitext(fn)[0]
    raw = open({'pe': stem + '.DT1', 'ramac': stem + '.rd3'}.get(filetype, fn), 'rb').read()
    bits = 8 * g['data'].dtype.itemsize
    L = {'gssi': lambda: rawload.gssi_layout(snum, tnum, bits), 'ramac': lambda: rawload.ramac_layout(snum, tnum),
         'tek': lambda: rawload.tek_layout(tnum), 'pe': lambda: rawload.pe_layout(snum, tnum, bits == 16)}[filetype]()
    assert R.same_bits(R.restate(raw, R.Layout(*L)), g['data'])
    assert R.same_bits(rawload.decode_host(raw, L), g['data'])


def test_decode_host_equals_the_restatement_on_the_sweep():
    from impdar_amd import rawload
    for snum, tnum in R.SHAPES:
        for name, (fmt, in_kind, op) in R.COMBOS.items():
            L = R.layout_for(fmt, in_kind, op, snum, tnum, 1026 if fmt == 'gssi' else None)
            raw = R.raw_for(L, R.samples_for(in_kind, snum, tnum, 1000 * snum + tnum), seed=snum + tnum)
            assert R.same_bits(rawload.decode_host(raw, rawload.Layout(*L)), R.restate(raw, L)), (name, snum, tnum)


def test_the_written_cases_hold_what_they_are_for(files):
    """The wide-binade file has a NaN inside one trace's window and an all-NaN window; the wrap file leaves int16."""
    g = golden('LD_P7_v16_f32_binades_nan')['data']
    assert np.isnan(g[:, 1]).all() and np.isnan(g[:, 0]).sum() == 1 and not np.isnan(g[:, 2:]).any()
    stem = os.path.splitext(files[0]['LD_P7_v16_f32_binades_nan'][1])[0]
    raw = np.frombuffer(open(stem + '.DT1', 'rb').read(), dtype=np.uint8).reshape(5, 128 + 4 * 137)[:, 128:]
    samples = np.abs(raw.copy().view('<f4').astype(np.float64))
    samples = samples[np.isfinite(samples) & (samples != 0)]
    assert np.log2(samples.max() / samples.min()) > 40
    stem = os.path.splitext(files[0]['LD_P8_first_i16_wrap'][1])[0]
    raw = np.frombuffer(open(stem + '.DT1', 'rb').read(), dtype=np.uint8).reshape(4, 128 + 202)[:, 128:]
    samples = raw.copy().view('<i2').astype(np.float64)
    exact = samples - samples[:, :100].mean(axis=1)[:, None]
    assert (np.abs(exact) > 32767).any()
    wrapped = golden('LD_P8_first_i16_wrap')['data'].T.astype(np.float64)
    assert (np.abs(wrapped - np.trunc(exact)) % 65536 == 0).all()


def test_errors_have_the_reference_type(files):
    from impdar_amd.lib import loaders
    from impdar_amd.lib.ImpdarError import ImpdarError
    from impdar_amd.lib.loaders import load_gssi, load_pulse_ekko, load_ramac, load_tek
    g = golden('LD_Z_errors')
    direct = {'gssi': load_gssi.load_gssi, 'pe': load_pulse_ekko.load_pe, 'ramac': load_ramac.load_ramac,
              'tek': load_tek.load_tek}
    types = {'ValueError': ValueError, 'IndexError': IndexError, 'error': struct.error, 'ImpdarError': ImpdarError,
             'FileNotFoundError': FileNotFoundError}
    assert sorted(k[:-5] for k in g if k.endswith('.type')) == sorted(files[1])
    for name, (filetype, fn) in files[1].items():
        want = types[str(g[name + '.type'])]
        with pytest.raises(want) as exc:
            direct[filetype](fn)
        assert type(exc.value) is want
        if name in ('tek_cut_inside_a_record', 'pe_gps_without_gga'):     # the reference's own text
            assert str(exc.value) == str(g[name + '.message'])
    assert str(g['tek_cut_inside_a_record.message']) == 'pressure needs length tnum 5'
    # as the reference's load(), the package's swallows an unreadable pulseEKKO file with a message
    assert loaders.load('pe', files[1]['pe_missing_hd'][1]) == []


@pytest.mark.parametrize('filetype', sorted(R.RAW_MAT_CASES))
def test_save_writes_what_the_reference_writes(loaded, filetype, tmp_path):
    from scipy.io import loadmat
    from impdar_amd.lib.RadarData import RadarData
    want = loadmat(os.path.join(GOLDEN, 'LD_%s_raw.mat' % filetype))
    fn = str(tmp_path / 'x_raw.mat')
    loaded[R.RAW_MAT_CASES[filetype]].save(fn)
    got = loadmat(fn)
    keys = lambda m: sorted(k for k in m if not k.startswith('__'))                 # noqa: E731
    assert keys(got) == keys(want)
    for k in keys(want):
        if k == 'flags':
            for field in want[k].dtype.names:
                assert R.same_value(got[k][field][0, 0], want[k][field][0, 0]), field
        elif k != 'fn':
            assert R.same_value(got[k], want[k]), k
    back = RadarData(fn)
    assert R.same_bits(back.data, loaded[R.RAW_MAT_CASES[filetype]].data)
    assert back.snum == loaded[R.RAW_MAT_CASES[filetype]].snum and back.tnum == loaded[R.RAW_MAT_CASES[filetype]].tnum


def test_the_load_parser_matches_the_reference():
    from impdar_amd.bin import impdarexec
    from impdar_amd.lib import loaders
    want = json.load(open(os.path.join(GOLDEN, 'LD_P_impdar.json')))
    parser = impdarexec._get_args()
    for filetype in ('gssi', 'pe', 'ramac', 'tek'):
        ns = vars(parser.parse_args(['load', filetype, 'a', 'b', '-o', 'x']))
        assert ns.pop('func') is loaders.load_and_exit
        ref = dict(want[filetype])
        assert ref.pop('func') == 'load_and_exit'
        assert ns == ref
    assert loaders.FILETYPE_OPTIONS == ['mat', 'pe', 'gssi', 'ramac', 'tek']
    with pytest.raises(SystemExit):
        parser.parse_args(['load', 'segy', 'a'])
    assert vars(parser.parse_args(['proc', '-vbp', '1', '2', 'f.mat']))['vbp'] == [1.0, 2.0]      # proc is untouched


def test_load_and_exit_names_its_outputs(files, tmp_path, monkeypatch):
    from impdar_amd.lib import loaders
    from impdar_amd.lib.RadarData import RadarData
    src = files[0]['LD_R1_ramac_cor'][1]
    want = golden('LD_R1_ramac_cor')['data']
    for ext in ('rd3', 'rad', 'cor'):
        for stem in ('one', 'two'):
            (tmp_path / ('%s_l.%s' % (stem, ext))).write_bytes(open(src[:-3] + ext, 'rb').read())
    one, two = str(tmp_path / 'one_l.rd3'), str(tmp_path / 'two_l.rd3')
    loaders.load_and_exit('ramac', one)                                  # beside the input
    assert R.same_bits(RadarData(str(tmp_path / 'one_l_raw.mat')).data, want)
    loaders.load_and_exit('ramac', [one], o=str(tmp_path / 'named.mat'))    # one file, a name
    assert R.same_bits(RadarData(str(tmp_path / 'named.mat')).data, want)
    with pytest.raises(FileNotFoundError):
        loaders.load_and_exit('ramac', [one, two], o=str(tmp_path / 'missing'))
    # a folder: the reference joins it and the whole input name without a separator
    out = tmp_path / 'out'
    out.mkdir()
    monkeypatch.chdir(tmp_path)
    loaders.load_and_exit('ramac', ['one_l.rd3', 'two_l.rd3'], o='out/')
    assert sorted(os.listdir(str(out))) == ['one_l_raw.mat', 'two_l_raw.mat']


def test_the_command_line_writes_a_loadable_file(files, tmp_path, monkeypatch):
    from impdar_amd.bin import impdarexec
    from impdar_amd.lib.RadarData import RadarData
    out = str(tmp_path / 'x_raw.mat')
    monkeypatch.setattr('sys.argv', ['impdar', 'load', 'ramac', os.path.join(GOLDEN, 'ten_col.rd3'), '-o', out])
    impdarexec.main()
    assert R.same_bits(RadarData(out).data, golden('LD_R1_ramac_cor')['data'])


def test_unknown_unprovided_and_mat_types(tmp_path, loaded):
    from impdar_amd.lib import loaders
    with pytest.raises(ValueError, match='Unrecognized filetype'):
        loaders.load('nonsense', ['x'])
    for filetype, missing in (('segy', 'segyio'), ('gprMax', 'h5py'), ('mcords_nc', 'netCDF4'), ('gecko', 'not provided'),
                              ('apres', 'not provided')):
        with pytest.raises(NotImplementedError, match=missing):
            loaders.load(filetype, ['x'])
    fn = str(tmp_path / 'm.mat')
    loaded['LD_T1_tek'].save(fn)
    back = loaders.load('mat', fn)
    assert len(back) == 1 and R.same_bits(back[0].data, loaded['LD_T1_tek'].data)
    # srs arguments are accepted and, without GDAL, change nothing
    a = loaders.load('ramac', os.path.join(GOLDEN, 'ten_col.rd3'), t_srs='EPSG:3413', s_srs='EPSG:4326')[0]
    assert R.object_differences(a, golden('LD_R1_ramac_cor')) == []


def test_gpslib_without_gdal():
    from impdar_amd.lib import gpslib
    for f in (lambda: gpslib.get_utm_conversion(1., 2.), lambda: gpslib.get_conversion('EPSG:3413'),
              lambda: gpslib.get_rev_conversion('EPSG:3413')):
        if not gpslib.conversions_enabled:
            with pytest.raises(ImportError, match='Cannot convert coordinates: osr not importable'):
                f()
    with pytest.raises(ValueError, match='I can only do gga sentences right now'):
        gpslib.nmea_all_info(['$GPRMC,1,2,3'])
    assert gpslib.hhmmss2dec(np.array([120000.0]))[0] == 0.5


# ------------------------------------------------------------------------------------- the descriptor check
def plan(hip_mod, nbytes, base, stride, head, snum, tnum, in_kind, op, out_kind=R.NATIVE):
    import ctypes as C
    out = C.c_longlong(-1)
    rc = hip_mod.load().impdar_rawload_plan(nbytes, base, stride, head, snum, tnum, in_kind, op, out_kind, C.byref(out))
    return rc, out.value


def test_plan_accepts_the_four_layouts():
    from impdar_amd import _hip, rawload
    for L, nbytes in ((rawload.gssi_layout(2048, 64, 32), 131072 + 64 * 8192), (rawload.gssi_layout(33, 70, 16), 65536 + 70 * 66),
                      (rawload.pe_layout(137, 41, True), 41 * (128 + 274)), (rawload.pe_layout(137, 41, False), 41 * (128 + 548)),
                      (rawload.ramac_layout(512, 10), 10240), (rawload.tek_layout(12), 24240)):
        for out_kind, size in ((R.NATIVE, R.IN_DTYPE[L.in_kind].itemsize), (R.OUT_F32, 4), (R.OUT_F64, 8)):
            assert plan(_hip, nbytes, *L, out_kind=out_kind) == (0, L.snum * L.tnum * size)
            assert rawload.plan(nbytes, L, out_kind) == L.snum * L.tnum * size
        assert plan(_hip, nbytes - 1, *L)[0] == _hip.ERR_ARG


def test_plan_rejects_what_the_route_header_lists():
    from impdar_amd import _hip, rawload
    ARG, UNS = _hip.ERR_ARG, _hip.ERR_UNSUPPORTED
    I16, I32, F32 = R.I16, R.I32, R.F32
    cases = [
        # nbytes, base, stride, head, snum, tnum, in_kind, op                       what
        ((INT64_MAX, 0, 1 << 62, 0, 4, 4, I16, R.NONE), ARG),                       # stride * tnum overflows
        ((INT64_MAX, INT64_MAX - 8, 16, 0, 4, 2, I16, R.NONE), ARG),                # base + ... overflows
        ((INT64_MAX, 0, INT64_MAX, INT64_MAX - 3, 4, 1, I16, R.NONE), ARG),         # head + snum * elem overflows
        ((1000, 0, 20, 14, 4, 2, I16, R.NONE), ARG),                                # head + snum * elem > stride
        ((1000, 0, 16, 0, 5, 2, I32, R.NONE), ARG),
        ((99, 0, 50, 0, 25, 2, I16, R.NONE), ARG),                                  # the last record ends past nbytes
        ((100, 4, 50, 0, 25, 2, I16, R.NONE), ARG),
        ((70, 0, 50, 20, 15, 2, I16, R.NONE), ARG),                                 # (a short last record would do, not this)
        ((1000, 0, 4, 0, 2, 10, I16, R.GSSI_TOP), ARG),                             # GSSI_TOP with snum < 3
        ((1000, 0, 8, 0, 0, 10, I16, R.NONE), ARG),                                 # snum < 1
        ((1000, 0, 8, 0, 4, 0, I16, R.NONE), ARG),                                  # tnum < 1
        ((1000, 0, 8, 0, -1, 10, I16, R.NONE), ARG),
        ((1000, -2, 8, 0, 4, 10, I16, R.NONE), ARG),
        ((1000, 0, 8, 0, 2, 10, I32, R.TEK_BIAS), UNS),                             # op / kind pairs that do not exist
        ((1000, 0, 8, 0, 2, 10, F32, R.TEK_BIAS), UNS),
        ((1000, 0, 8, 0, 2, 10, I32, R.PE_DEMEAN), UNS),
        ((1000, 0, 16, 0, 4, 10, F32, R.GSSI_TOP), UNS),
        ((1000, 0, 8, 0, 2, 10, 3, R.NONE), UNS),
        ((1000, 0, 8, 0, 2, 10, I16, 4), UNS),
    ]
    for args, want in cases:
        rc, size = plan(_hip, *args)
        assert (rc, size) == (want, 0), args
        with pytest.raises(ValueError if want == ARG else NotImplementedError):
            rawload.plan(args[0], rawload.Layout(*args[1:]))
    assert plan(_hip, 1000, 0, 8, 0, 2, 10, I16, R.NONE, out_kind=3)[0] == UNS
    # the limits themselves pass
    assert plan(_hip, 100, 0, 50, 0, 25, 2, I16, R.NONE) == (0, 100)
    assert plan(_hip, 90, 0, 50, 20, 15, 2, I16, R.NONE)[0] == ARG and plan(_hip, 100, 0, 50, 20, 15, 2, I16, R.NONE)[0] == 0
    assert plan(_hip, 12, 0, 6, 0, 3, 2, I16, R.GSSI_TOP) == (0, 12)
    # 2^31 - 1 samples by as many traces: sizes beyond 32 bits are exact
    big = (1 << 31) - 1
    assert plan(_hip, INT64_MAX, 0, 2 * big, 0, big, big, I16, R.NONE, out_kind=R.OUT_F64)[0] == ARG   # 8 * big^2 > 2^63
    assert plan(_hip, INT64_MAX, 0, 2 * big, 0, big, big, I16, R.NONE) == (0, 2 * big * big)


def test_decode_host_checks_as_the_plan_does():
    from impdar_amd import rawload
    with pytest.raises(ValueError):
        rawload.decode_host(b'\0' * 99, rawload.Layout(0, 50, 0, 25, 2, R.I16, R.NONE))
    with pytest.raises(ValueError):
        rawload.decode_host(b'\0' * 100, rawload.Layout(0, 4, 0, 2, 10, R.I16, R.GSSI_TOP))
    with pytest.raises(NotImplementedError):
        rawload.decode_host(b'\0' * 100, rawload.Layout(0, 8, 0, 2, 10, R.F32, R.TEK_BIAS))


HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_the_route_header_is_plain_host_cxx(tmp_path):
    """csrc/rawload_route.h compiles as the only include of a C++ (not HIP) translation unit: no HIP types, nothing taken
    from the place it is included at."""
    import subprocess
    from conftest import ROOT
    src = tmp_path / 'route_alone.cpp'
    src.write_text('#include "rawload_route.h"\nint main() { RawloadDesc d; return rawload_route(d).status == IMPDAR_OK; }\n')
    subprocess.check_call([HIPCC, '-x', 'c++', '-std=c++17', '-fsyntax-only', '-Wall', '-Werror', '-I',
                           os.path.join(ROOT, 'impdar_amd', 'csrc'), str(src)])
