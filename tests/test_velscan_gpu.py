"""The Stolt velocity scan on the device (csrc/stolt.hip: impdar_stolt_scan[_dev]; its kernels: csrc/stolt_kernels.h) at the smallest shapes that reach every route:

  traces first, power of two (tnum = 64 is the gate)        64 x 64, 128 x 64      float32, float64
  [w][kx], power of two (tnum < 64)                         64 x 32                float32, float64
  rocFFT (odd snum: the output loses a row; small non-power-of-two)  65 x 50 float64, 100 x 48 float32
  traces first, mixed radix (tnum > 1024, tnum / 2 = 1200)  96 x 2400              float32
  integer data (tapered on the host)                        128 x 64               int16

Every image of a scan must be, bit for bit, what ``migrate('stolt', vel=v)`` gives; the sums are held to a longdouble
evaluation of those images at (n + 4) u (velscan_ref.sum_bound).  The input is synth's white noise, which fills the whole
band, as the other Stolt tests' is.  One set of scans and single migrations per shape is shared by the tests (``case``)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import velscan_ref as ref
from conftest import rel_l2, rel_max

pytestmark = pytest.mark.gpu

VELS = 1.68e8 * np.array([0.8, 0.9, 1.0, 1.1, 1.25])
HT, VT = 7, 11
CASES = [(64, 64, np.float32, 'rows'), (64, 64, np.float64, 'rows'), (128, 64, np.float32, 'rows'), (128, 64, np.float64, 'rows'),
         (64, 32, np.float32, 'wkx'), (64, 32, np.float64, 'wkx'), (65, 50, np.float64, 'rocfft'), (100, 48, np.float32, 'rocfft'),
         (96, 2400, np.float32, 'mixed'), (128, 64, np.int16, 'rows'),
         # (beyond the table: float32 rows of 50 traces start 8 bytes off a 16-byte boundary every other row -- the reduction's
         # one-by-one loads of whole groups)
         (65, 50, np.float32, 'rocfft')]
IDS = ['%dx%d-%s-%s' % (s, t, np.dtype(d).name, r) for s, t, d, r in CASES]
# what the metrics line's kernel string holds on each route (and what it must not hold)
KERNEL = {'rows': (['stolt_stretch_scan_rows', 'traces first'], ['mixed radix']),
          'mixed': (['stolt_stretch_scan_rows', 'traces first', 'mixed radix'], []),
          'wkx': (['stolt_stretch_scan_t', 'own row transforms'], ['traces first', 'mixed radix']),
          'rocfft': (['stolt_stretch', 'rocFFT'], ['own row transforms'])}


def make(snum, tnum, dtype, data=None):
    from impdar_amd import synth
    from impdar_amd.lib.RadarData import RadarData
    geo = synth.geometry(snum, tnum)
    if data is None:
        data = synth.noise_radargram(snum, tnum, seed=snum + tnum)
        data = (data * 3000).astype(dtype) if dtype == np.int16 else data.astype(dtype)
    d = RadarData(None)
    d.data, d.snum, d.tnum = data.copy(), snum, tnum
    d.travel_time, d.dist, d.trace_int, d.dt = geo['travel_time'], geo['dist'], geo['trace_int'], geo['dt']
    return d, geo


def last_metrics():
    from impdar_amd import _hip
    buf = C.create_string_buffer(1024)
    _hip.check(_hip.load().impdar_ctx_last_metrics(_hip.context(), buf, len(buf)), 'metrics')
    return json.loads(buf.value.decode())


@functools.lru_cache(maxsize=None)
def case(snum, tnum, dtype):
    """dict(dat, geo, scans: the host scan keeping image k for k < 5, single: migrate('stolt') at each velocity, metrics)."""
    dat, geo = make(snum, tnum, dtype)
    scans = [dat.velocity_scan(VELS, htaper=HT, vtaper=VT, keep=k) for k in range(len(VELS))]
    metrics = last_metrics()
    single = []
    for v in VELS:
        d, _ = make(snum, tnum, dtype)
        d.migrate('stolt', vel=float(v), htaper=HT, vtaper=VT)
        single.append(d.data)
    return dict(dat=dat, geo=geo, scans=scans, single=single, metrics=metrics)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('snum, tnum, dtype, route', CASES, ids=IDS)
def test_images_are_the_single_migrations(hip, snum, tnum, dtype, route):
    c = case(snum, tnum, dtype)
    before = make(snum, tnum, dtype)[0].data
    assert same_bits(c['dat'].data, before)                       # the scan left the radargram alone
    want_dtype = np.float32 if dtype == np.float32 else np.float64
    oracle = ref.images(before, c['geo'], VELS, HT, VT)
    for k in range(len(VELS)):
        img = c['scans'][k].image
        assert img.dtype == want_dtype and img.shape == (2 * (snum // 2), tnum)
        assert same_bits(img, c['single'][k]), k
        assert oracle[k].dtype == img.dtype
        if dtype == np.float32:
            err = rel_l2(img, oracle[k])
            print(k, 'rel_l2', err)
            assert err < 1e-4
        else:
            err = rel_max(img, oracle[k])
            print(k, 'rel_max', err)
            assert err < 1e-12
    if dtype == np.int16:
        return                                                    # (integer radargrams cannot be held on the device)
    res, _ = make(snum, tnum, dtype)
    res.to_device()
    for k in range(len(VELS)):
        scan = res.velocity_scan(VELS, htaper=HT, vtaper=VT, keep=k)
        assert isinstance(scan.image, hip.DeviceArray) and scan.image.dtype == want_dtype
        assert same_bits(scan.image.to_host(), c['single'][k]), k
        assert same_bits(scan.l2, c['scans'][k].l2) and same_bits(scan.l1, c['scans'][k].l1) and same_bits(scan.l4, c['scans'][k].l4)
        scan.image.free()
    res.from_device()
    assert same_bits(res.data, before) and (res.snum, res.tnum) == (snum, tnum)


@pytest.mark.parametrize('snum, tnum, dtype, route', CASES, ids=IDS)
def test_sums_against_longdouble(hip, snum, tnum, dtype, route):
    c = case(snum, tnum, dtype)
    imgs = [s.image for s in c['scans']]
    for t0, t1 in ((0, tnum), (3, tnum - 5), (17, 18)):
        scan = c['scans'][0] if (t0, t1) == (0, tnum) else c['dat'].velocity_scan(VELS, htaper=HT, vtaper=VT, traces=(t0, t1))
        assert scan.traces == (t0, t1)
        got = np.stack([scan.l1, scan.l2, scan.l4], axis=2)
        want = ref.exact_sums(imgs, t0, t1)
        assert np.isfinite(got).all() and (want[:, :, 1] > 0).any()
        err = np.abs(got - want)
        print((t0, t1), 'max rel err / u', float(np.max(err / np.where(want > 0, want, 1))) / ref.U, 'bound / u', ref.sum_bound(t1 - t0) / ref.U)
        assert (err <= ref.sum_bound(t1 - t0) * want).all()


@pytest.mark.parametrize('snum, tnum, dtype, route', CASES, ids=IDS)
def test_batching_and_repeats_give_the_same_bits(hip, snum, tnum, dtype, route):
    from impdar_amd import velscan
    c = case(snum, tnum, dtype)
    first = c['scans'][4]
    for mb in (0, 1, 2, 0):                                        # 2: a ragged last batch of one; 0 again: a second call
        scan = velscan.stolt_velocity_scan(c['dat'], VELS, htaper=HT, vtaper=VT, keep=4, max_batch=mb)
        want_b = {0: 5, 1: 1, 2: 2}[mb]
        m = last_metrics()
        assert (m['entry'], m['B'], m['nv']) == ('impdar_stolt_scan', want_b, 5), m
        for name in ('l1', 'l2', 'l4', 'image'):
            assert same_bits(getattr(scan, name), getattr(first, name)), (mb, name)
    one = c['dat'].velocity_scan(VELS[2:3], htaper=HT, vtaper=VT, keep=0)
    assert one.l2.shape == (1, 2 * (snum // 2)) and same_bits(one.l2[0], first.l2[2]) and same_bits(one.l4[0], first.l4[2])
    assert same_bits(one.image, c['scans'][2].image)


@pytest.mark.parametrize('snum, tnum, dtype, route', CASES, ids=IDS)
def test_metrics_name_the_route(hip, snum, tnum, dtype, route):
    m = case(snum, tnum, dtype)['metrics']
    assert m['entry'] == 'impdar_stolt_scan' and m['nv'] == 5 and m['B'] == 5
    has, has_not = KERNEL[route]
    assert all(s in m['kernel'] for s in has) and not any(s in m['kernel'] for s in has_not), m


@pytest.mark.parametrize('snum, tnum, dtype, route', [c for c in CASES if c[2] != np.int16], ids=[i for i in IDS if 'int16' not in i])
def test_nan_sample_gives_nan_sums(hip, snum, tnum, dtype, route):
    """One NaN in the radargram is a NaN in every sample of every image (the transforms spread it), and NumPy's sums of such an
    image are NaN: so are the scan's, and there is no best velocity."""
    dat, _ = make(snum, tnum, dtype)
    dat.data[snum // 3, tnum // 2] = np.nan
    scan = dat.velocity_scan(VELS, htaper=HT, vtaper=VT, keep=1)
    assert np.isnan(scan.image).all()
    assert np.isnan(ref.ref_sums([scan.image], 0, tnum)).all()
    assert np.isnan(scan.l1).all() and np.isnan(scan.l2).all() and np.isnan(scan.l4).all()
    with pytest.raises(ValueError, match='no finite focus value'):
        scan.best()


def test_argument_checks_of_the_c_abi(hip):
    from impdar_amd import velscan
    data = np.ones((8, 8), dtype=np.float32)
    kx, ws = np.zeros(8), np.arange(5.0)
    for vels, t0, t1, keep in (([], 0, 8, -1), ([1e8, -1.0], 0, 8, -1), ([1e8, np.inf], 0, 8, -1), ([1e8, np.nan], 0, 8, -1),
                               ([1e8], -1, 8, -1), ([1e8], 4, 4, -1), ([1e8], 0, 9, -1), ([1e8], 0, 8, 1), ([1e8], 0, 8, -2)):
        with pytest.raises(ValueError):
            velscan.scan_host(data, kx, ws, np.array(vels, dtype=np.float64), 7, 11, t0, t1, keep=keep)


SINGLE_CALL = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + '/tests')
import test_velscan_gpu as t
out = {}
for snum, tnum in ((64, 64), (64, 32), (100, 48)):
    d, _ = t.make(snum, tnum, np.float32)
    d.migrate('stolt', vel=1.68e8, htaper=t.HT, vtaper=t.VT)
    out['%dx%d' % (snum, tnum)] = d.data
np.savez(sys.argv[2], **out)
'''


def test_single_call_is_unchanged_by_a_scan_in_the_same_process(hip, tmp_path):
    """migrate('stolt') before and after a scan (which shares its plan and buffers) gives the bits of a process that never scanned."""
    fresh = str(tmp_path / 'fresh.npz')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, '-c', SINGLE_CALL, root, fresh], check=True, timeout=120)
    with np.load(fresh) as z:
        for snum, tnum in ((64, 64), (64, 32), (100, 48)):
            want = z['%dx%d' % (snum, tnum)]
            for step in ('before', 'after'):
                d, _ = make(snum, tnum, np.float32)
                d.migrate('stolt', vel=1.68e8, htaper=HT, vtaper=VT)
                assert same_bits(d.data, want), (snum, tnum, step)
                if step == 'before':
                    scanned, _ = make(snum, tnum, np.float32)
                    scanned.velocity_scan(VELS, htaper=HT, vtaper=VT, keep=2, max_batch=2)


def test_scan_focuses_on_the_device(hip):
    """The 256 x 256 diffractor case of test_velscan_cpu.py in float32: best index 6, and the varimax curve within 1e-4 relative of
    the CPU restatement's (oracle images in float32, float64 sums)."""
    from impdar_amd import synth, velscan
    snum = tnum = 256
    data = synth.diffractor_radargram(snum, tnum, vel=1.69e8, fc=5.0e6, ndiff=8, dtype=np.float32)
    dat, geo = make(snum, tnum, np.float32, data=data)
    vels = 1.69e8 * np.linspace(0.7, 1.3, 13)
    window, region = (tnum // 8, tnum - tnum // 8), (snum // 8, snum - snum // 8)
    scan = dat.velocity_scan(vels, htaper=10, vtaper=10, traces=window)
    got = scan.varimax(samples=region)
    want = velscan.VelocityScan(vels, ref.ref_sums(ref.images(data, geo, vels, 10, 10), *window), window).varimax(samples=region)
    print('device', got, 'restatement', want)
    assert scan.best(samples=region) == (6, vels[6])
    assert np.max(np.abs(got - want) / want) < 1e-4
