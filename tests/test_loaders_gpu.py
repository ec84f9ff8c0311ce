"""The instrument-file decode in HBM (csrc/rawload.hip) against the NumPy restatement of tests/rawload_ref.py, bit for
bit, at the smallest shapes where the kernels can go wrong; the loaders' resident form against their host form; one chain
that starts from a file's bytes.  Reads only tests/golden/ and what it writes to tmp_path."""
import ctypes as C
import functools
import os
import shutil

import numpy as np
import pytest

import rawload_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(name, snum, tnum, base=None):
    """(raw bytes, layout, the restated native result) of one sweep case: made once, shared, never written to."""
    fmt, in_kind, op = R.COMBOS[name]
    L = R.layout_for(fmt, in_kind, op, snum, tnum, base)
    raw = R.raw_for(L, R.samples_for(in_kind, snum, tnum, 1000 * snum + tnum), seed=snum + tnum)
    want = R.restate(raw, L)
    want.setflags(write=False)
    return raw, L, want


def layout_of(L):
    from impdar_amd import rawload
    return rawload.Layout(*L)


@pytest.mark.parametrize('name', sorted(R.COMBOS))
@pytest.mark.parametrize('snum,tnum', R.SHAPES)
def test_decode_dev_equals_the_restatement(hip, name, snum, tnum):
    from impdar_amd import rawload
    raw, L, want = case(name, snum, tnum)
    for out_kind, out_dtype in R.OUT_DTYPES.items():
        d = rawload.decode_dev(raw, layout_of(L), out_dtype)
        got = d.to_host()
        d.free()
        assert got.shape == (snum, tnum)
        assert R.same_bits(got, R.expected(want, out_kind)), (name, snum, tnum, out_kind)


@pytest.mark.parametrize('name', ['pe16', 'pe32f', 'gssi32'])
def test_host_bytes_in_equals_device_bytes_in(hip, name):
    """impdar_rawload (host bytes) and impdar_rawload_dev (bytes already in HBM) run the same decode."""
    from impdar_amd import rawload
    raw, L, want = case(name, 101, 129)
    ctx = hip.context()
    d_raw = hip.DeviceArray.from_host(ctx, np.frombuffer(raw, dtype=np.uint8))
    for out_kind, out_dtype in R.OUT_DTYPES.items():
        a = rawload.decode_dev(raw, layout_of(L), out_dtype)
        b = rawload.decode_dev(d_raw, layout_of(L), out_dtype)
        ha, hb = a.to_host(), b.to_host()
        a.free()
        b.free()
        assert ha.tobytes() == hb.tobytes()
        assert R.same_bits(ha, R.expected(want, out_kind))
    d_raw.free()


@pytest.mark.parametrize('name,base', [('gssi16', 1026), ('gssi32', 1026), ('gssi16', 1025), ('gssi32', 1027)])
def test_a_base_that_is_no_multiple_of_four(hip, name, base):
    """A GSSI-like layout with an odd header: records at 2 bytes past a multiple of 4, and at an odd byte."""
    from impdar_amd import rawload
    raw, L, want = case(name, 65, 63, base)
    ctx = hip.context()
    d_raw = hip.DeviceArray.from_host(ctx, np.frombuffer(raw, dtype=np.uint8))
    for src in (raw, d_raw):
        for out_kind, out_dtype in R.OUT_DTYPES.items():
            d = rawload.decode_dev(src, layout_of(L), out_dtype)
            got = d.to_host()
            d.free()
            assert R.same_bits(got, R.expected(want, out_kind)), (name, base, out_kind)
    d_raw.free()


def test_two_calls_return_the_same_bits(hip):
    from impdar_amd import rawload
    raw, L, _ = case('pe32f', 129, 257)
    outs = []
    for _ in range(2):
        d = rawload.decode_dev(raw, layout_of(L), np.float64)
        outs.append(d.to_host().tobytes())
        d.free()
    assert outs[0] == outs[1]


def test_a_rejected_layout_launches_nothing(hip):
    """The device entry points answer as the plan does (the kernels are never handed such a layout)."""
    from impdar_amd import rawload
    raw, L, _ = case('ramac', 9, 65)
    with pytest.raises(ValueError):
        rawload.decode_dev(raw[:-2], layout_of(L))
    with pytest.raises(NotImplementedError):
        rawload.decode_dev(raw, layout_of(L)._replace(op=R.TEK_BIAS, in_kind=R.F32))


# ------------------------------------------------------------------------------------------ the loaders, resident
@pytest.fixture(scope='module')
def files(tmp_path_factory):
    return R.loader_cases(str(tmp_path_factory.mktemp('loaders_gpu')), GOLDEN)


@pytest.mark.parametrize('resident', ['float32', 'float64'])
@pytest.mark.parametrize('name', ['LD_R1_ramac_cor', 'LD_T1_tek', 'LD_G1_gssi32_sample', 'LD_G2_gssi16_dzg',
                                  'LD_P1_first_i16_gps', 'LD_P7_v16_f32_binades_nan'])
def test_resident_load_equals_the_host_load(hip, files, name, resident):
    from impdar_amd.lib import loaders
    filetype, fn = files[name]
    host = loaders.load(filetype, fn)[0]
    dat = loaders.load(filetype, fn, resident=resident)[0]
    assert dat.data is None and dat._dev is not None and dat._dev.shape == (host.snum, host.tnum)
    assert dat.data_dtype == host.data.dtype and dat._dev.dtype == np.dtype(resident)
    assert dat.to_device() is dat                     # already there
    for attr in ('snum', 'tnum', 'dt', 'trig', 'travel_time', 'decday', 'dist', 'trace_int'):
        assert R.same_value(getattr(dat, attr), getattr(host, attr)), attr
    dat.check_attrs()
    dat.from_device()
    with np.errstate(all='ignore'):
        assert R.same_bits(dat.data, host.data.astype(resident))


def test_a_chain_from_the_file_bytes(hip, files):
    """load resident -> vertical band pass -> download equals the host load widened, uploaded and run the same way: the
    same kernels on the same input bits."""
    from impdar_amd.lib import loaders, process
    filetype, fn = files['LD_P1_first_i16_gps']
    dat = loaders.load(filetype, fn, resident='float32')[0]
    assert process.process([dat], vbp=(20., 100.))
    dat.from_device()
    host = loaders.load(filetype, fn)[0]
    host.data = host.data.astype(np.float32)
    host.to_device()
    assert process.process([host], vbp=(20., 100.))
    host.from_device()
    assert dat.data.dtype == host.data.dtype and dat.data.shape == host.data.shape
    assert R.same_bits(dat.data, host.data)
    assert np.isfinite(dat.data).all() and np.abs(dat.data).max() > 0
    assert dat.flags.bpass.tolist() == host.flags.bpass.tolist()
