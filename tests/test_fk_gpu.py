"""The f-k fan filter and the f-k spectrum on the GPU, held to the yardstick of tests/fk_ref.py: max|dev - hi| <= 8 max|ref - hi|
with ``hi`` the contract in longdouble and ``ref`` the same with the transforms in the data's precision -- the house margin for
a different order of the same sums.  The shapes reach every transform route and every kernel layout:

    64 x 64     own rows, power of two              32 x 1280   mixed-radix rows by default
    32 x 16     own [w][kx], power of two           63 x 65     rocFFT, odd snum (the inverse plan beside Stolt's)
    96 x 160    mixed-radix rows ('mixed')          100 x 96    rocFFT, default
    96 x 75     mixed-radix [w][kx], tnum odd       2 x 64, 128 x 3   rocFFT, smallest

Largest ratio max|dev - hi| / max|ref - hi| seen on an MI355X: see DESIGN.md 4.19.
"""
import itertools
import os
import sys
from unittest.mock import patch

import numpy as np
import pytest

import fk_ref
import stolt_route_cases as SC

pytestmark = pytest.mark.gpu

DT, DX = 1.0e-8, 1.0
V0 = DX / DT            # one sample per trace
SHAPES = [(64, 64, None), (32, 16, None), (96, 160, 'mixed'), (96, 75, 'mixed'), (32, 1280, None), (63, 65, None), (100, 96, None),
          (2, 64, None), (128, 3, None)]
IDS = ['%dx%d%s' % (s, t, '-' + k if k else '') for s, t, k in SHAPES]
KERNELS = {(64, 64): 'fk_fan_rows', (32, 16): 'fk_fan_wkx', (96, 160): 'fk_fan_rows', (96, 75): 'fk_fan_wkx', (32, 1280): 'fk_fan_rows',
           (63, 65): 'fk_fan_kxw', (100, 96): 'fk_fan_kxw', (2, 64): 'fk_fan_kxw', (128, 3): 'fk_fan_kxw'}
# either edge and both (tapers apart: (1 / 5) 1.2 <= (1 / 0.8) 0.8 in units of 1 / V0)
FANS = [dict(va_lo=1.2 * V0, taper=0.25), dict(va_hi=6.0 * V0, taper=0.1), dict(va_lo=0.8 * V0, va_hi=5.0 * V0, taper=0.2)]


def make(snum, tnum, dtype):
    from impdar_amd import synth
    from impdar_amd.lib.RadarData import RadarData
    geo = synth.geometry(snum, tnum, dt=DT, dx=DX)
    d = RadarData(None)
    d.data, d.snum, d.tnum = fk_ref.radargram(snum, tnum, dtype), snum, tnum
    d.travel_time, d.dist, d.trace_int, d.dt = geo['travel_time'], geo['dist'], geo['trace_int'], geo['dt']
    d.fn = ''
    return d


def ref_axes(d):
    """The full frequency axis of the yardstick and the library's own wavenumbers."""
    from impdar_amd.lib.migrationlib.mig_hip import _kx
    return 2. * np.pi * np.fft.fftfreq(d.snum, d.dt), _kx(d)


def err(a, hi):
    return float(np.max(np.abs(np.asarray(a).astype(fk_ref.LD) - hi)))


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('snum,tnum,word', SHAPES, ids=IDS)
def test_fan_filter_against_the_yardstick(hip, snum, tnum, word, dtype):
    """pass and reject, each dip, either and both edges; pass + reject of one fan sums to x within the bar of that sum."""
    d0 = make(snum, tnum, dtype)
    w, kx = ref_axes(d0)
    worst = 0.0
    with SC.knob(word):
        for fan, dip in itertools.product(FANS, fk_ref.DIPS):
            got, ref = {}, {}
            for mode in fk_ref.MODES:
                d = make(snum, tnum, dtype)
                d.fk_filter(mode=mode, dip=dip, **fan)
                assert SC.last_metrics()['kernel'].startswith(KERNELS[(snum, tnum)] + ' (')
                assert d.data.dtype == dtype and d.data.shape == (snum, tnum)
                hi = fk_ref.fan(d0.data, w, kx, 'hi', mode=mode, dip=dip, **fan)
                ref[mode] = fk_ref.fan(d0.data, w, kx, 'ref', mode=mode, dip=dip, **fan)
                got[mode] = d.data
                e_dev, e_ref = err(d.data, hi), err(ref[mode], hi)
                worst = max(worst, e_dev / e_ref)
                print('fan %dx%d %s %s %s %s: dev %.3e ref %.3e ratio %.2f' % (snum, tnum, np.dtype(dtype).name, sorted(fan), dip, mode,
                                                                           e_dev, e_ref, e_dev / e_ref))
                assert e_dev <= 8 * e_ref, (fan, dip, mode)
            x = d0.data.astype(fk_ref.LD)
            s_dev = err(got['pass'].astype(np.float64) + got['reject'].astype(np.float64), x)
            s_ref = err(ref['pass'].astype(np.float64) + ref['reject'].astype(np.float64), x)
            print('sum %dx%d %s %s %s: dev %.3e ref %.3e' % (snum, tnum, np.dtype(dtype).name, sorted(fan), dip, s_dev, s_ref))
            assert s_dev <= 8 * s_ref, (fan, dip)
    print('largest ratio %dx%d %s: %.2f' % (snum, tnum, np.dtype(dtype).name, worst))


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('snum,tnum,word', SHAPES, ids=IDS)
def test_fk_spectrum_against_the_yardstick(hip, snum, tnum, word, dtype):
    """|fft2|^2 over the frequencies >= 0, the columns in fftshift order (even and odd tnum), float64 whatever the data; exact
    axes; host and resident give the same bits."""
    d = make(snum, tnum, dtype)
    with SC.knob(word):
        f, k, P = d.fk_spectrum()
        d.to_device()
        P_res = d.fk_spectrum()[2]
        d.from_device()
    m = snum // 2 + 1
    assert P.dtype == np.float64 and P.shape == (m, tnum)
    assert np.array_equal(P, P_res)
    assert np.array_equal(f, (2. * np.pi * np.fft.rfftfreq(snum, d=d.dt)) / (2. * np.pi) * 1.0e-6)
    assert np.allclose(f, np.fft.rfftfreq(snum, DT) * 1.0e-6, rtol=1e-15, atol=0)
    assert np.array_equal(k, np.fft.fftshift(ref_axes(d)[1]) / (2. * np.pi))
    assert k[tnum // 2] == 0.0 and np.all(np.diff(k) > 0)
    hi = fk_ref.power(d.data, 'hi')
    e_dev, e_ref = err(P, hi), err(fk_ref.power(d.data, 'ref'), hi)
    print('power %dx%d %s: dev %.3e ref %.3e ratio %.2f' % (snum, tnum, np.dtype(dtype).name, e_dev, e_ref, e_dev / e_ref))
    assert e_dev <= 8 * e_ref


@pytest.mark.parametrize('snum,tnum,word', [SHAPES[0], SHAPES[3], SHAPES[5], SHAPES[6]], ids=[IDS[0], IDS[3], IDS[5], IDS[6]])
def test_host_resident_in_place_and_repeated_calls_give_the_same_bits(hip, snum, tnum, word):
    from impdar_amd import _hip, fk
    fan = fk.check_fan((snum, tnum), va_lo=0.8 * V0, va_hi=5.0 * V0, taper=0.2, mode='pass', dip='down_right')
    for dtype in (np.float32, np.float64):
        d = make(snum, tnum, dtype)
        kx, ws = fk._axes(d)
        with SC.knob(word):
            host = fk.fan_host(d.data, kx, ws, fan)
            again = fk.fan_host(d.data, kx, ws, fan)
            dev = _hip.DeviceArray.from_host(_hip.context(), d.data)
            out = _hip.DeviceArray(_hip.context(), (snum, tnum), dtype)
            fk.fan_dev(dev, kx, ws, fan, out=out)
            apart = out.to_host()
            assert np.array_equal(dev.to_host(), d.data)            # d_data is left alone when d_out is another array
            fk.fan_dev(dev, kx, ws, fan)
            in_place = dev.to_host()
            dev.free()
            out.free()
            e = make(snum, tnum, dtype)
            e.to_device()
            e.fk_filter(va_lo=0.8 * V0, va_hi=5.0 * V0, taper=0.2, dip='down_right')
            assert e.data is None and e._dev is not None            # the radargram stayed in HBM
            e.from_device()
        for other in (again, apart, in_place, e.data):
            assert np.array_equal(host, other)


def test_entries_refuse_before_any_device_work(hip):
    """The C entries, with null device pointers that any device work would fault on ... and no context call: ERR_ARG first."""
    import ctypes as C
    lib, ctx = hip.load(), hip.context()
    kx, ws = np.zeros(8), np.zeros(5)
    data = np.zeros((8, 8), dtype=np.float32)
    p = data.ctypes.data_as(C.c_void_p)
    nan = float('nan')
    bad = [(0, 8, 8, nan, nan, 0.1, 0, 0), (0, 8, 8, 0.0, nan, 0.1, 0, 0), (0, 8, 8, nan, float('inf'), 0.1, 0, 0),
           (0, 8, 8, 1.0, nan, 1.0, 0, 0), (0, 8, 8, 1.0, nan, -0.5, 0, 0), (0, 8, 8, 1.0, 1.1, 0.1, 0, 0), (0, 1, 8, 1.0, nan, 0.1, 0, 0),
           (0, 8, 1, 1.0, nan, 0.1, 0, 0), (2, 8, 8, 1.0, nan, 0.1, 0, 0), (0, 8, 8, 1.0, nan, 0.1, 2, 0), (0, 8, 8, 1.0, nan, 0.1, 0, 3)]
    for dtype, snum, tnum, lo, hi_, taper, mode, dip in bad:
        for fn in (lib.impdar_fk_fan, lib.impdar_fk_fan_dev):
            rc = fn(ctx, p, dtype, snum, tnum, hip.as_dp(kx)[1], hip.as_dp(ws)[1], lo, hi_, taper, mode, dip, p)
            assert rc == hip.ERR_ARG, (dtype, snum, tnum, lo, hi_, taper, mode, dip)
            assert hip.last_error()
    for dtype, snum, tnum in ((2, 8, 8), (0, 1, 8), (0, 8, 1)):
        assert lib.impdar_fk_power(ctx, p, dtype, snum, tnum, hip.as_dp(kx)[1], hip.as_dp(ws)[1], hip.as_dp(np.zeros(64))[1]) == hip.ERR_ARG
        assert lib.impdar_fk_power_dev(ctx, p, dtype, snum, tnum, hip.as_dp(kx)[1], hip.as_dp(ws)[1], p) == hip.ERR_ARG
    assert np.all(data == 0)


@pytest.mark.parametrize('snum,tnum', [(64, 64), (100, 96)])
def test_stolt_fk_stolt_shares_one_plan(hip, snum, tnum):
    """stolt -> fk -> stolt at one size: the two images are bit-identical and nothing was planned after the first call (the
    f-k metrics line: "planned" 0, and "plans_built" the same two Stolt calls later)."""
    def stolt():
        d = make(snum, tnum, np.float32)
        d.migrate('stolt', vel=1.68e8, htaper=8, vtaper=6)
        return d.data

    def fk_call():
        d = make(snum, tnum, np.float32)
        d.fk_filter(va_lo=1.2 * V0, taper=0.25)
        return SC.last_metrics()
    first = stolt()
    m1 = fk_call()
    assert m1['entry'] == 'impdar_fk_fan' and m1['planned'] == 0
    assert m1['kernel_ms'] >= 0 and m1['device_ms'] >= m1['kernel_ms']
    third = stolt()
    m2 = fk_call()
    assert np.array_equal(first, third)
    assert m2['planned'] == 0 and m2['plans_built'] == m1['plans_built']
    # ... and another size is planned
    d = make(snum, tnum + 2, np.float32)
    d.fk_filter(va_lo=1.2 * V0, taper=0.25)
    m3 = SC.last_metrics()
    assert m3['planned'] == 1 and m3['plans_built'] == m1['plans_built'] + 1


def test_integer_data_is_widened(hip):
    d = make(32, 16, np.float64)
    d.data = np.round(d.data * 100).astype(np.int16)
    want = d.data.astype(np.float64)
    e = make(32, 16, np.float64)
    e.data = want.copy()
    d.fk_filter(va_hi=6.0 * V0)
    e.fk_filter(va_hi=6.0 * V0)
    assert d.data.dtype == np.float64 and np.array_equal(d.data, e.data)


def _line_file(tmp_path, snum=96, tnum=60):
    from impdar_amd import synth
    from impdar_amd.lib.NoInitRadarData import NoInitRadarData
    geo = synth.geometry(snum, tnum, dt=DT, dx=DX)
    d = NoInitRadarData(big=True)
    d.data = fk_ref.radargram(snum, tnum, np.float64)
    d.snum, d.tnum = snum, tnum
    for k in ('lat', 'long', 'trace_num', 'decday', 'trig', 'pressure'):
        setattr(d, k, np.zeros(tnum))
    d.travel_time, d.dist, d.trace_int, d.dt = geo['travel_time'], geo['dist'], geo['trace_int'], geo['dt']
    d.flags.bpass = np.array([1., 2., 30.])
    fn = str(tmp_path / 'line_raw.mat')
    d.save(fn)
    return d, fn


def test_impproc_fk_end_to_end(hip, tmp_path):
    """`impproc fk` on a .mat file: <name>_fk.mat by main's naming rule, the keys a saved file has, the flags as they were, the
    data the yardstick's."""
    from scipy.io import loadmat
    from impdar_amd.bin import impproc
    from impdar_amd.lib.RadarData import RadarData
    d, fn = _line_file(tmp_path)
    argv = ['impproc', 'fk', '--va_lo', str(0.8 * V0), '--va_hi', str(5.0 * V0), '--taper', '0.2', '--mode', 'reject', '--dip', 'down_left', fn]
    with patch.object(sys, 'argv', argv):
        impproc.main()
    out_fn = str(tmp_path / 'line_fk.mat')
    assert os.path.exists(out_fn)
    before, after = loadmat(fn), loadmat(out_fn)
    assert set(after.keys()) == set(before.keys())
    assert after['flags'].dtype.names == before['flags'].dtype.names
    for name in before['flags'].dtype.names:
        assert np.array_equal(after['flags'][name][0, 0], before['flags'][name][0, 0]), name
    r = RadarData(out_fn)
    w, kx = ref_axes(r)
    fan = dict(va_lo=0.8 * V0, va_hi=5.0 * V0, taper=0.2, mode='reject', dip='down_left')
    hi = fk_ref.fan(d.data, w, kx, 'hi', **fan)
    assert err(r.data, hi) <= 8 * err(fk_ref.fan(d.data, w, kx, 'ref', **fan), hi)


def test_plot_fk_draws_the_spectrum_in_db(hip):
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    from impdar_amd.lib import plot
    d = make(32, 16, np.float32)
    f, k, P = d.fk_spectrum()
    fig, ax = plot.plot_fk(d)
    try:
        img = ax.get_images()[0]
        assert np.array_equal(np.asarray(img.get_array()), 10.0 * np.log10(P / np.max(P)))
        x0, x1, y0, y1 = img.get_extent()
        assert x0 < k[0] < k[-1] < x1 and y0 < f[0] < f[-1] < y1
        assert ax.get_xlabel() and ax.get_ylabel()
        fig2, ax2 = plt.subplots()
        assert plot.plot_fk(d, fig=fig2, ax=ax2) == (fig2, ax2)
    finally:
        plt.close('all')
