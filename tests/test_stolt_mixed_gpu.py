"""Stolt on the library's own mixed-radix row transforms (csrc/own_fft_mixed.h) at sizes 2^a 3^b 5^c 7^d that are no power of
two: against the oracle at the bars of tests/test_stolt_gpu.py (float64 max|diff| <= 1e-12 max|ref|, float32 relative L2
<= 1e-4), against the rocFFT form of the same call at the bars of tests/test_knobs_gpu.py (relative L2 < 2e-6 float32,
< 1e-13 float64), and which route a size takes: by default the mixed route only where a length is above 1024 (where rocFFT
compiles kernels at run time), IMPDAR_STOLT_FFT=mixed wherever the lengths allow."""
import ctypes as C
import json

import numpy as np
import pytest

from conftest import rel_l2, rel_max

pytestmark = pytest.mark.gpu

F64_TOL = 1e-12
F32_L2 = 1e-4
VEL, HTAPER, VTAPER = 1.68e8, 7, 11


def _dat(data, geo):
    from impdar_amd.lib.RadarData import RadarData
    d = RadarData(None)
    d.data, (d.snum, d.tnum) = data.copy(), data.shape
    d.travel_time, d.dist, d.trace_int, d.dt = geo['travel_time'], geo['dist'], geo['trace_int'], geo['dt']
    return d


def _kernel(hip):
    buf = C.create_string_buffer(1024)
    hip.check(hip.load().impdar_ctx_last_metrics(hip.context(), buf, len(buf)), 'metrics')
    return json.loads(buf.value.decode())['kernel']


def _case(snum, tnum, dtype):
    from impdar_amd import synth
    from oracle import mig_oracle
    geo = synth.geometry(snum, tnum)
    data = synth.noise_radargram(snum, tnum, seed=snum + tnum)
    data = (data * 3000).astype(dtype) if dtype == np.int16 else data.astype(dtype)
    want = mig_oracle.stolt(data, geo['dt'], geo['trace_int'], geo['dist'], VEL, HTAPER, VTAPER)
    return geo, data, want


def _migrate(hip, monkeypatch, data, geo, knob):
    if knob is None:
        monkeypatch.delenv('IMPDAR_STOLT_FFT', raising=False)
    else:
        monkeypatch.setenv('IMPDAR_STOLT_FFT', knob)
    d = _dat(data, geo)
    d.migrate('stolt', vel=VEL, htaper=HTAPER, vtaper=VTAPER)
    monkeypatch.delenv('IMPDAR_STOLT_FFT', raising=False)
    return d.data, _kernel(hip)


def _meets_the_oracle_bar(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    if got.dtype == np.float32:
        print('relative L2 against the oracle %.3g' % rel_l2(got, want))
        assert rel_l2(got, want) < F32_L2, rel_l2(got, want)
    else:
        print('max|diff| / max|ref| against the oracle %.3g' % rel_max(got, want))
        assert rel_max(got, want) < F64_TOL, rel_max(got, want)


@pytest.mark.parametrize('snum,tnum,dtype,rows', [
    (96, 160, np.float64, True),        # rows form, both axes mixed
    (250, 100, np.float64, True),       # rows form; C2C of 250, the R2C's complex length 50
    (120, 60, np.float32, False),       # fewer than 64 traces: the [w][kx] form
    (300, 75, np.float64, False),       # an odd number of traces: the [w][kx] form
    (128, 1250, np.float32, True),      # the power-of-two kernel and the mixed one in one call
    (1500, 64, np.float32, True),       # mixed over time, a power of two over the traces
    (96, 160, np.int16, True),          # tapered on the host: no weights on the device
])
def test_mixed_route_against_oracle_and_rocfft(hip, monkeypatch, snum, tnum, dtype, rows):
    geo, data, want = _case(snum, tnum, dtype)
    got, kernel = _migrate(hip, monkeypatch, data, geo, 'mixed')
    assert 'mixed radix' in kernel and 'own row transforms' in kernel, kernel
    assert ('stolt_stretch_rows' in kernel) == rows, kernel
    _meets_the_oracle_bar(got, want)
    lib_form, kernel = _migrate(hip, monkeypatch, data, geo, 'rocfft')
    assert 'rocFFT' in kernel, kernel
    err = rel_l2(got, lib_form)
    print('relative L2 against the rocFFT form %.3g' % err)
    assert err < (2e-6 if got.dtype == np.float32 else 1e-13), err


def test_default_takes_the_mixed_route_above_1024(hip, monkeypatch):
    geo, data, want = _case(64, 1280, np.float32)
    got, kernel = _migrate(hip, monkeypatch, data, geo, None)
    assert 'mixed radix' in kernel and 'stolt_stretch_rows' in kernel, kernel
    _meets_the_oracle_bar(got, want)
    again, kernel = _migrate(hip, monkeypatch, data, geo, 'own')         # (the default, spelled out)
    assert 'mixed radix' in kernel and np.array_equal(again, got)


@pytest.mark.parametrize('snum,tnum', [(96, 160), (64, 1100)])
def test_default_keeps_rocfft(hip, monkeypatch, snum, tnum):
    """No length above 1024 (nothing for rocFFT to compile), or a length with a factor 11: rocFFT's plans, as before."""
    geo, data, want = _case(snum, tnum, np.float32)
    got, kernel = _migrate(hip, monkeypatch, data, geo, None)
    assert 'rocFFT' in kernel and 'mixed radix' not in kernel, kernel
    _meets_the_oracle_bar(got, want)


def test_power_of_two_sizes_do_not_change_with_the_knob(hip, monkeypatch):
    geo, data, _ = _case(256, 128, np.float32)
    one, kernel1 = _migrate(hip, monkeypatch, data, geo, None)
    two, kernel2 = _migrate(hip, monkeypatch, data, geo, 'mixed')
    assert kernel1 == kernel2 and 'mixed radix' not in kernel1, (kernel1, kernel2)
    assert one.tobytes() == two.tobytes()


def test_kx_that_is_not_antisymmetric_takes_the_form_with_all_wavenumbers(hip, monkeypatch):
    """Through the C API: the rows form holds the wavenumbers k < 0 through kx[k] == -kx[tnum - k]; an axis without that
    symmetry runs the [w][kx] form and gives rocFFT's image."""
    snum, tnum = 96, 160
    geo, data, _ = _case(snum, tnum, np.float64)
    lib, ctx = hip.load(), hip.context()
    kx = np.ascontiguousarray(2. * np.pi * np.fft.fftfreq(tnum, d=float(np.mean(geo['trace_int']))))
    kx[1] *= 1.01
    ws = np.ascontiguousarray(2. * np.pi * np.fft.rfftfreq(snum, d=geo['dt']))
    dp = C.POINTER(C.c_double)
    outs = {}
    for knob in ('mixed', 'rocfft'):
        monkeypatch.setenv('IMPDAR_STOLT_FFT', knob)
        out = np.empty((snum, tnum))
        hip.check(lib.impdar_stolt(ctx, data.ctypes.data_as(C.c_void_p), hip.dtype_code(data.dtype), snum, tnum, kx.ctypes.data_as(dp),
                                   ws.ctypes.data_as(dp), VEL, float(HTAPER), float(VTAPER), out.ctypes.data_as(C.c_void_p)), 'impdar_stolt')
        outs[knob] = out, _kernel(hip)
    monkeypatch.delenv('IMPDAR_STOLT_FFT', raising=False)
    assert 'mixed radix' in outs['mixed'][1] and 'stolt_stretch_rows' not in outs['mixed'][1], outs['mixed'][1]
    assert 'rocFFT' in outs['rocfft'][1]
    err = rel_max(outs['mixed'][0], outs['rocfft'][0])
    print('max|diff| / max|ref| against the rocFFT form %.3g' % err)
    assert err < 1e-13, err


def test_resident_radargram_takes_the_same_route(hip, monkeypatch):
    geo, data, _ = _case(128, 1250, np.float32)
    host, kernel = _migrate(hip, monkeypatch, data, geo, None)
    assert 'mixed radix' in kernel, kernel
    d = _dat(data, geo)
    d.to_device()
    d.migrate('stolt', vel=VEL, htaper=HTAPER, vtaper=VTAPER)
    kernel = _kernel(hip)
    d.from_device()
    assert 'mixed radix' in kernel and 'stolt_stretch_rows' in kernel, kernel
    assert d.data.dtype == host.dtype and d.data.tobytes() == host.tobytes()
