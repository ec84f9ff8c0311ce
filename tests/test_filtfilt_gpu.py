"""Both filtfilt kernels against ``scipy.signal.filtfilt`` at every coefficient count they take.

* vertical (``impdar_filtfilt[_dev]``, csrc/preproc.hip, along time): 2..33 coefficients, float32 and float64 data,
  the shortest record SciPy accepts and lengths that put the 32-sample chunks on every alignment against the odd
  extension, whole and partial 16-trace wavefronts;
* horizontal (``impdar_hfiltfilt[_dev]``, csrc/hpass.hip, along traces): 2..17 coefficients, row counts around the
  rows per wavefront of each template, float32 and float64 input;
* the two kernels against each other on transposed data, non-finite input, the FIR path at every size up to its
  256 taps, ``vertical_band_pass`` at orders 11-16 on the host and resident paths, and the limits.

The designs (tests/filtfilt_ref.py) keep SciPy within 1e-13 of long double (tests/test_filtfilt_cpu.py), so a miss
is the kernel's.  The bar is the kernels' own claim, SciPy's float64 operation order: the IIR outputs equal SciPy's
bit for bit (float64, and float32 after the same cast), as measured on the MI355X at every case here.  The FIR kernel
sums in another order and with FMAs: 1e-12 * max|expected| for float64, one unit in the last place for float32."""
import ctypes as C

import numpy as np
import pytest

import filtfilt_ref as fr
from conftest import rel_max
from test_preproc_gpu import check_filtered, filt_dat

pytestmark = pytest.mark.gpu

VERT_SNUM_EXTRA = (1, 2, 5, 31, 32, 33, 97)     # snum - 3 * ncoef (1: the shortest record SciPy accepts)
VERT_TNUM = (1, 15, 17, 37)                     # traces: 16 per wavefront
HORIZ_TNUM_EXTRA = (1, 2, 31, 32, 33, 69)       # tnum - 3 * ncoef
FIR_NTAPS = (2, 8, 9, 17, 101, 255, 256)
FIR_TNUM = (1, 255, 257)                        # 256 traces per block
FIR_TOL = 1e-12


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def vert(x, s, dev):
    """filtfilt(b, a, x, axis=0) by impdar_filtfilt on a host copy of x, or by impdar_filtfilt_dev on a resident one."""
    from impdar_amd import _hip
    lib, ctx = _hip.load(), _hip.context()
    b, a, zi = s
    snum, tnum = x.shape
    code = _hip.dtype_code(x.dtype)
    if not dev:
        y = np.array(x, order='C')
        _hip.check(lib.impdar_filtfilt(ctx, y.ctypes.data_as(C.c_void_p), code, snum, tnum, _dp(b), _dp(a), len(b),
                                       _dp(zi)), 'impdar_filtfilt')
        return y
    d = _hip.DeviceArray.from_host(ctx, x)
    try:
        _hip.check(lib.impdar_filtfilt_dev(ctx, d.ptr, code, snum, tnum, _dp(b), _dp(a), len(b), _dp(zi)),
                   'impdar_filtfilt')
        return d.to_host()
    finally:
        d.free()


def horiz(x, s, dev):
    """filtfilt(b, a, x, axis=1) as float64 by impdar_hfiltfilt, or by impdar_hfiltfilt_dev on a resident copy (in
    place for float64, into a new float64 array for float32, as the library's own callers do)."""
    from impdar_amd import _hip
    lib, ctx = _hip.load(), _hip.context()
    b, a, zi = s
    snum, tnum = x.shape
    code = _hip.dtype_code(x.dtype)
    x = np.ascontiguousarray(x)
    if not dev:
        out = np.full((snum, tnum), -7.0)
        _hip.check(lib.impdar_hfiltfilt(ctx, x.ctypes.data_as(C.c_void_p), code, snum, tnum, _dp(b), _dp(a), len(b),
                                        _dp(zi), _dp(out)), 'impdar_hfiltfilt')
        return out
    d = _hip.DeviceArray.from_host(ctx, x)
    d_out = d if x.dtype == np.float64 else _hip.DeviceArray(ctx, (snum, tnum), np.float64)
    try:
        _hip.check(lib.impdar_hfiltfilt_dev(ctx, d.ptr, code, snum, tnum, _dp(b), _dp(a), len(b), _dp(zi), d_out.ptr),
                   'impdar_hfiltfilt')
        return d_out.to_host()
    finally:
        d.free()
        d_out.free()


def fir(x, taps, dev):
    """impdar_fir_shift (host copy) or impdar_fir_shift_dev (resident copy) of x."""
    from impdar_amd import _hip
    lib, ctx = _hip.load(), _hip.context()
    snum, tnum = x.shape
    code = _hip.dtype_code(x.dtype)
    if not dev:
        y = np.array(x, order='C')
        _hip.check(lib.impdar_fir_shift(ctx, y.ctypes.data_as(C.c_void_p), code, snum, tnum, _dp(taps), len(taps)),
                   'impdar_fir_shift')
        return y
    d = _hip.DeviceArray.from_host(ctx, x)
    try:
        _hip.check(lib.impdar_fir_shift_dev(ctx, d.ptr, code, snum, tnum, _dp(taps), len(taps)), 'impdar_fir_shift')
        return d.to_host()
    finally:
        d.free()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def scipy_filtfilt(s, x, axis):
    from scipy.signal import filtfilt
    return filtfilt(s[0], s[1], x, axis=axis)


def differences(case, host, dev, want):
    """What is wrong with the host / resident outputs of one case ([] if nothing)."""
    bad = []
    if not same(host, dev):
        bad.append('%s: host and resident forms differ' % case)
    if not same(host, want):
        bad.append('%s: differs from SciPy (max rel %.2e, %d of %d elements)'
                   % (case, rel_max(host, want), int(np.sum(bits(host) != bits(want))), host.size))
    return bad


def report(bad):
    return '%d failing case(s):\n' % len(bad) + '\n'.join(bad[:12])


# ------------------------------------------------------------------------------------------------ vertical kernel
@pytest.mark.parametrize('ncoef', range(fr.NCOEF_MIN, fr.VERT_MAX + 1))
def test_vertical_kernel_every_coefficient_count(hip, ncoef):
    s = fr.spec(*fr.design(ncoef))
    rng = np.random.default_rng(100 + ncoef)
    bad = []
    for dtype in (np.float64, np.float32):
        for extra in VERT_SNUM_EXTRA:
            snum = 3 * ncoef + extra
            x = rng.standard_normal((snum, max(VERT_TNUM))).astype(dtype)
            want_all = scipy_filtfilt(s, x, 0).astype(dtype)   # trace by trace: its first columns answer x's
            for tnum in VERT_TNUM:
                xs = np.ascontiguousarray(x[:, :tnum])
                bad += differences('%s snum=%d tnum=%d' % (np.dtype(dtype).name, snum, tnum),
                                   vert(xs, s, False), vert(xs, s, True), want_all[:, :tnum])
    assert not bad, report(bad)


@pytest.mark.parametrize('ncoef', [5, 11, 21, 33])   # the largest count of each template (NC = 5, 11, 21, 33)
def test_vertical_kernel_non_finite_input(hip, ncoef):
    """NaN at the first sample, at x[3*ncoef] (the farthest source of the left odd extension), mid-trace and at the
    last sample, +-inf in other traces, in both 16-trace wavefronts: SciPy's NaN / inf pattern, and every clean trace
    exact and finite."""
    s = fr.spec(*fr.design(ncoef))
    edge = 3 * ncoef
    snum, tnum = edge + 40, 20
    dirty = {0: [(0, np.nan)], 1: [(edge, np.nan)], 2: [(snum // 2, np.nan)], 3: [(snum - 1, np.nan)],
             6: [(snum // 3, np.inf)], 9: [(1, -np.inf)], 16: [(edge, np.inf), (snum - 2, np.nan)],
             18: [(snum - 1, -np.inf)]}
    clean = np.array([j not in dirty for j in range(tnum)])
    for dtype in (np.float64, np.float32):
        x = np.random.default_rng(ncoef).standard_normal((snum, tnum)).astype(dtype)
        for j, hits in dirty.items():
            for i, v in hits:
                x[i, j] = v
        with np.errstate(invalid='ignore', over='ignore'):
            want = scipy_filtfilt(s, x, 0).astype(dtype)
        assert not np.isfinite(want[:, ~clean]).any()
        for dev in (False, True):
            got = vert(x, s, dev)
            assert got.dtype == dtype
            np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
            np.testing.assert_array_equal(np.isinf(got), np.isinf(want))
            assert np.isfinite(got[:, clean]).all()
            assert same(got[:, clean], want[:, clean]), rel_max(got[:, clean], want[:, clean])


# ---------------------------------------------------------------------------------------------- horizontal kernel
def rows_per_wavefront(ncoef):
    return 64 // (4 if ncoef - 1 <= 4 else 8)   # hp_dispatch: 4 lanes per row up to 4 delays, else 8


@pytest.mark.parametrize('ncoef', range(fr.NCOEF_MIN, fr.HORIZ_MAX + 1))
def test_horizontal_kernel_every_coefficient_count(hip, ncoef):
    s = fr.spec(*fr.design(ncoef))
    rpw = rows_per_wavefront(ncoef)
    snums = (1, rpw - 1, rpw, rpw + 1, 2 * rpw + 3)
    rng = np.random.default_rng(200 + ncoef)
    bad = []
    for dtype in (np.float64, np.float32):
        for extra in HORIZ_TNUM_EXTRA:
            tnum = 3 * ncoef + extra
            x = rng.standard_normal((max(snums), tnum)).astype(dtype)
            want_all = scipy_filtfilt(s, x, 1)                 # float64, row by row
            for snum in snums:
                xs = np.ascontiguousarray(x[:snum])
                host, dev = horiz(xs, s, False), horiz(xs, s, True)
                assert host.dtype == dev.dtype == np.float64
                bad += differences('%s snum=%d tnum=%d' % (np.dtype(dtype).name, snum, tnum), host, dev,
                                   want_all[:snum])
    assert not bad, report(bad)


@pytest.mark.parametrize('ncoef', range(fr.NCOEF_MIN, fr.HORIZ_MAX + 1))
def test_horizontal_kernel_equals_vertical_kernel_on_the_transpose(hip, ncoef):
    """Both kernels claim SciPy's operation order, so they agree bit for bit whatever the local SciPy was built with:
    hfiltfilt(x) == filtfilt(x.T).T (float32 input: the vertical kernel returns float32, so compare after the cast)."""
    s = fr.spec(*fr.design(ncoef))
    rpw = rows_per_wavefront(ncoef)
    rng = np.random.default_rng(300 + ncoef)
    bad = []
    for dtype in (np.float64, np.float32):
        for extra in HORIZ_TNUM_EXTRA:
            for snum in (1, rpw + 1, 2 * rpw + 3):
                x = rng.standard_normal((snum, 3 * ncoef + extra)).astype(dtype)
                h = horiz(x, s, False).astype(dtype)
                v = vert(np.ascontiguousarray(x.T), s, False).T
                if not same(h, v):
                    bad.append('%s %s: max rel %.2e' % (np.dtype(dtype).name, x.shape, rel_max(h, v)))
    assert not bad, report(bad)


# ------------------------------------------------------------------------------------------------------ FIR path
@pytest.mark.parametrize('ntaps', FIR_NTAPS)
def test_fir_shift_every_size(hip, ntaps):
    """lfilter(taps, 1, x) shifted up by order = ntaps - 1 rows, the last `order` rows untouched (a record of
    `order` samples comes back unchanged), against the oracle."""
    from oracle import preproc_oracle as po
    order = ntaps - 1
    rng = np.random.default_rng(400 + ntaps)
    taps = rng.standard_normal(ntaps)
    bad = []
    for dtype in (np.float64, np.float32):
        for snum in (order, order + 1, order + 7, order + 8, order + 9, 3 * order + 5):
            x = rng.standard_normal((snum, max(FIR_TNUM))).astype(dtype)
            want_all = po.fir_shift(taps, x)                  # float64 (snum - order, 257), trace by trace
            for tnum in FIR_TNUM:
                xs = np.ascontiguousarray(x[:, :tnum])
                host, dev = fir(xs, taps, False), fir(xs, taps, True)
                case = '%s snum=%d tnum=%d' % (np.dtype(dtype).name, snum, tnum)
                if not same(host, dev):
                    bad.append(case + ': host and resident forms differ')
                n = max(snum - order, 0)
                if not same(host[n:], xs[n:]):
                    bad.append(case + ': the last %d rows were changed' % (snum - n))
                if n == 0:
                    continue
                got, want = host[:n], want_all[:, :tnum]
                if dtype == np.float64:
                    if not rel_max(got, want) <= FIR_TOL:
                        bad.append(case + ': max rel %.2e' % rel_max(got, want))
                else:
                    w32 = want.astype(np.float32)
                    if not np.all(np.abs(got.astype(np.float64) - w32.astype(np.float64)) <= np.spacing(np.abs(w32))):
                        bad.append(case + ': more than one ulp off')
    assert not bad, report(bad)


# ---------------------------------------------------------------------------------------------------- public API
@pytest.mark.parametrize('filttype,order', fr.API_DESIGNS)
def test_vertical_band_pass_high_orders(hip, filttype, order):
    """vertical_band_pass(10, 40 MHz) at dt = 1e-8, 23-33 coefficients: float64, float32 and int16 on the host path,
    float64 and float32 resident, against SciPy with the band-pass bars of test_preproc_gpu.py."""
    from oracle import preproc_oracle as po
    _, b, a = po.design(1e-8, *fr.API_BAND, order=order, filttype=filttype)
    raw = np.random.default_rng(500 + order).standard_normal((3 * len(b) + 150, 37))
    for dtype in (np.float64, np.float32, np.int16):
        data = (raw * 1000).astype(dtype) if dtype == np.int16 else raw.astype(dtype)
        want = scipy_filtfilt((b, a), data, 0).astype(dtype)
        for resident in ((False, True) if dtype != np.int16 else (False,)):
            d = filt_dat(data)
            if resident:
                d.to_device()
            d.vertical_band_pass(*fr.API_BAND, order=order, filttype=filttype)
            if resident:
                d.from_device()
            check_filtered(d.data, want)
            np.testing.assert_array_equal(d.flags.bpass, [1., 10., 40.])


# -------------------------------------------------------------------------------------------------------- limits
@pytest.mark.parametrize('kw,message', [
    (dict(order=17), r'impdar_filtfilt: 35 filter coefficients \(2\.\.33 supported\)'),
    (dict(filttype='fir', order=256), r'impdar_fir_shift: 257 taps \(1\.\.256 supported\)'),
])
def test_vertical_band_pass_limits_leave_everything_unchanged(hip, kw, message):
    data = np.random.default_rng(600).standard_normal((400, 21))
    for resident in (False, True):
        d = filt_dat(data)
        if resident:
            d.to_device()
        with pytest.raises(ValueError, match=message):
            d.vertical_band_pass(*fr.API_BAND, **kw)
        np.testing.assert_array_equal(d.flags.bpass, np.zeros(3))
        if resident:
            assert d.data is None
            assert same(d._dev.to_host(), data)
            d.from_device()
        assert same(d.data, data)


def test_horizontal_kernel_rejects_18_coefficients(hip):
    """impdar_hfiltfilt and impdar_hfiltfilt_dev through the library's own callers: the limit's message, and the
    input and the resident array (filtered in place when float64) unchanged."""
    from impdar_amd import _hip
    from impdar_amd import hpass as hp
    s = fr.spec(*fr.design(18))
    message = r'impdar_hfiltfilt: 18 filter coefficients \(2\.\.17 supported\)'
    for dtype in (np.float64, np.float32):
        x = np.random.default_rng(700).standard_normal((20, 200)).astype(dtype)
        keep = x.copy()
        with pytest.raises(ValueError, match=message):
            hp.filtfilt_host(x, s)
        assert same(x, keep)
        d = _hip.DeviceArray.from_host(_hip.context(), x)
        try:
            with pytest.raises(ValueError, match=message):
                hp.filtfilt_dev(d, s)
            assert same(d.to_host(), keep)
        finally:
            d.free()
