"""The Wiener and median kernels at their smallest breaking shapes on the GPU: the sweep of ``denoise_sweep.py`` (its
docstring has the references and the bars, ``test_denoise_sweep_cpu.py`` the seams each case crosses) with
``impdar_amd.denoise``'s entries in the restatement's place.

  wiener   every window on 65 x 257, 3 x 1025 and 66 x 2049; every shape under (1, 10), (4, 6) and (65, 3); a flat band
           of +1000 that holds the pivot row of strip 0, and one that does not; NaN, +inf and -inf on both sides of the
           tile seam and the strip seam with the noise given; the (1, 1) window on every shape; the widest window the
           argument check admits
  median   N = 16 | 17, 32 | 33, 64 | 65 in every orientation, both halo extremes, reflection over many periods, the
           float64 radix path past column 255, 65537 rows through the radix kernel's row loop
  both     the resident entry gives the host-buffer entry's bits; a second call gives the first call's bits

Each test prints its worst |error| / bar (``-s``)."""
import numpy as np
import pytest

import denoise_sweep as ds
from impdar_amd import denoise as dn

pytestmark = pytest.mark.gpu

WN_GROUPS = ds.wiener_groups()
MD_GROUPS = ds.median_groups()
WIDEST = ((3, 5), (2, ds.HOR_WIN_MAX))
REPEAT_SHAPES = ((66, 2049), (65, 257))
RESIDENT_SHAPES = ((2, 3), (65, 257), (3, 1025), (66, 2049), (2050, 5), (65537, 3))
WORST = {}


def record(family, ratio, nratio):
    old = WORST.get(family, (0.0, 0.0))
    WORST[family] = (max(old[0], ratio), max(old[1], nratio))
    print('%s: |diff| = %.4f of the bar, noise error = %.4f of the bar; worst so far %.4f, %.4f'
          % ((family, ratio, nratio) + WORST[family]))


def resident_wiener(hip):
    def fn(x, m, n, noise):
        d_x = hip.DeviceArray.from_host(hip.context(), x)
        try:
            d_out, used = dn.wiener_dev(d_x, m, n, noise)
            try:
                return d_out.to_host(), used
            finally:
                d_out.free()
        finally:
            d_x.free()
    return fn


def resident_median(hip):
    def fn(x, m, n):
        d_x = hip.DeviceArray.from_host(hip.context(), x)
        try:
            d_out = dn.median_dev(d_x, m, n)
            try:
                return d_out.to_host()
            finally:
                d_out.free()
        finally:
            d_x.free()
    return fn


def wiener_call(fn, case):
    return fn(ds.wiener_input(case.shape, case.dtype, case.variant), case.win[0], case.win[1], case.given)


@pytest.mark.parametrize('key', list(WN_GROUPS))
def test_wiener_sweep(hip, key):
    record('wiener ' + key.split('-')[0], *ds.sweep_wiener(dn.wiener_host, WN_GROUPS[key]))


@pytest.mark.parametrize('shape', ds.WN_SHAPES, ids=[ds.SHAPE_NAMES[s] for s in ds.WN_SHAPES])
def test_wiener_unit_window(hip, shape):
    """The (1, 1) window.  float64: lVar is exactly 0 (the ``n == 1`` path takes no horizontal sum), so the reference's
    error on every shape.  float32: lVar = fl32(x * x) - x * x, the rounding error of the float32 square, and its mean
    is not zero on any of the shapes; the kernel and the long-double form agree: nothing is raised (the error is for a
    noise of exactly 0), the noise meets its bar and the output is lMean = x."""
    record('wiener unit window', *ds.check_wiener_unit_window(dn.wiener_host, shape))
    ds.check_wiener_unit_window(resident_wiener(hip), shape)


def test_wiener_widest_window(hip):
    """hor_win = 2**30 - 1 with m = 2 on 3 x 5: the cost does not depend on the window; every window is the whole
    row, all but five of its columns padding."""
    shape, win = WIDEST
    cases = [ds.WnCase(shape, win, dt, 'base', None) for dt in ds.DTYPES]
    record('wiener widest window', *ds.sweep_wiener(dn.wiener_host, cases))
    ds.sweep_wiener(resident_wiener(hip), cases)


@pytest.mark.parametrize('key', list(MD_GROUPS))
def test_median_sweep(hip, key):
    ds.sweep_median(dn.median_host, MD_GROUPS[key])


@pytest.mark.parametrize('shape', RESIDENT_SHAPES, ids=[ds.SHAPE_NAMES[s] for s in RESIDENT_SHAPES])
def test_resident_entry_gives_the_host_entry_bits(hip, shape):
    wn = [c for c in ds.all_cases(WN_GROUPS) if c.shape == shape]
    md = [c for c in ds.all_cases(MD_GROUPS) if c.shape == shape]
    assert wn or md
    for case in wn:
        host, host_noise = wiener_call(dn.wiener_host, case)
        res, res_noise = wiener_call(resident_wiener(hip), case)
        assert ds.same_bits(res, host) and np.float64(res_noise).tobytes() == np.float64(host_noise).tobytes(), case
    for case in md:
        x = ds.median_input(case.shape, case.dtype)
        assert ds.same_bits(resident_median(hip)(x, *case.win), dn.median_host(x, *case.win)), case


@pytest.mark.parametrize('shape', REPEAT_SHAPES, ids=[ds.SHAPE_NAMES[s] for s in REPEAT_SHAPES])
def test_second_call_gives_the_first_call_bits(hip, shape):
    """The noise is summed in a fixed order, so the estimate and with it the output repeat bit for bit; another
    case's call in between changes nothing."""
    wn = [c for c in ds.all_cases(WN_GROUPS) if c.shape == shape]
    md = [c for c in ds.all_cases(MD_GROUPS) if c.shape == shape]
    assert any(c.given is None for c in wn) and md
    first = [wiener_call(dn.wiener_host, c) for c in wn]
    for case, (out, noise) in zip(wn, first):
        again, noise2 = wiener_call(dn.wiener_host, case)
        assert ds.same_bits(again, out) and np.float64(noise2).tobytes() == np.float64(noise).tobytes(), case
    first = [dn.median_host(ds.median_input(c.shape, c.dtype), *c.win) for c in md]
    for case, out in zip(md, first):
        assert ds.same_bits(dn.median_host(ds.median_input(case.shape, case.dtype), *case.win), out), case
