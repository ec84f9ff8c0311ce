"""The library's own mixed-radix row transforms (csrc/own_fft_mixed.h) through impdar_fft_rows_any_dev -- lengths 2^a 3^b 5^c 7^d,
what Stolt runs on at field sizes -- against numpy.fft at the bars of tests/test_own_fft_gpu.py: float32 relative L2 <= 2e-6,
float64 max|diff| <= 1e-13 * log2(n) * max|ref|.  Power-of-two lengths run on the power-of-two kernel, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# every radix alone and mixed, a radix-2 tail, odd lengths, the smallest and the largest
COMPLEX_N = [18, 21, 48, 60, 100, 625, 2401, 5000, 6561, 7500, 8000]
REAL_N = [36, 120, 1250, 10000, 16000]          # (1250: the complex length, 625, is odd)


def _run(hip, entry, mode, dtype, n, a, out_shape, out_dtype, scale=1.0, inplace=False):
    from impdar_amd import _hip
    lib, ctx = hip.load(), hip.context()
    d_in = _hip.DeviceArray.from_host(ctx, np.ascontiguousarray(a).view(dtype).reshape(a.shape[0], -1))
    n_out = int(np.prod(out_shape)) * (2 if np.issubdtype(out_dtype, np.complexfloating) else 1)
    d_out = d_in if inplace else _hip.DeviceArray(ctx, (out_shape[0], n_out // out_shape[0]), dtype)
    try:
        _hip.check(getattr(lib, entry)(ctx, mode, _hip.dtype_code(dtype), n, a.shape[0], d_in.ptr, d_out.ptr, float(scale)), entry)
        return d_out.to_host().reshape(out_shape[0], -1).view(out_dtype).reshape(out_shape)
    finally:
        d_in.free()
        if not inplace:
            d_out.free()


def _close(got, want, dtype, n):
    if dtype == np.float32:
        err = np.linalg.norm(got - want) / np.linalg.norm(want)
        print('n=%d float32 relative L2 %.3g' % (n, err))
        assert err < 2e-6, err
    else:
        err = np.max(np.abs(got - want)) / np.max(np.abs(want))
        print('n=%d float64 max|diff| / max|ref| %.3g' % (n, err))
        assert err < 1e-13 * np.log2(n), err


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n', COMPLEX_N)
def test_complex_rows_against_numpy(hip, n, dtype):
    rng = np.random.default_rng(n)
    batch = 37 if n <= 4096 else 5
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    z = (rng.standard_normal((batch, n)) + 1j * rng.standard_normal((batch, n))).astype(cdt)
    inv = np.fft.ifft(z.astype(np.complex128), axis=1)
    _close(_run(hip, 'impdar_fft_rows_any_dev', 0, dtype, n, z, (batch, n), cdt), np.fft.fft(z.astype(np.complex128), axis=1), dtype, n)
    _close(_run(hip, 'impdar_fft_rows_any_dev', 1, dtype, n, z, (batch, n), cdt, scale=1.0 / n, inplace=True), inv, dtype, n)
    _close(_run(hip, 'impdar_fft_rows_any_dev', 4, dtype, n, z, (batch, n), dtype, scale=1.0 / n), inv.real, dtype, n)      # Re only


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n', REAL_N)
def test_real_rows_against_numpy(hip, n, dtype):
    rng = np.random.default_rng(n)
    batch = 37 if n <= 4096 else 5
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    x = rng.standard_normal((batch, n)).astype(dtype)
    X = np.fft.rfft(x.astype(np.float64), axis=1)
    _close(_run(hip, 'impdar_fft_rows_any_dev', 2, dtype, n, x, (batch, n // 2 + 1), cdt), X, dtype, n)
    Xc = X.astype(cdt)
    _close(_run(hip, 'impdar_fft_rows_any_dev', 3, dtype, n, Xc, (batch, n), dtype, scale=1.0 / n), np.fft.irfft(Xc.astype(np.complex128), n=n, axis=1), dtype, n)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n', [64, 4096])
def test_power_of_two_lengths_run_on_the_power_of_two_kernel(hip, n, dtype):
    rng = np.random.default_rng(n)
    batch = 37
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    z = (rng.standard_normal((batch, n)) + 1j * rng.standard_normal((batch, n))).astype(cdt)
    x = rng.standard_normal((batch, n)).astype(dtype)
    X = np.fft.rfft(x.astype(np.float64), axis=1).astype(cdt)
    for mode, a, shape, odt in ((0, z, (batch, n), cdt), (1, z, (batch, n), cdt), (4, z, (batch, n), dtype), (2, x, (batch, n // 2 + 1), cdt),
                                (3, X, (batch, n), dtype)):
        one = _run(hip, 'impdar_fft_rows_dev', mode, dtype, n, a, shape, odt, scale=0.5)
        two = _run(hip, 'impdar_fft_rows_any_dev', mode, dtype, n, a, shape, odt, scale=0.5)
        assert one.tobytes() == two.tobytes(), (mode, n)


def test_rejects_what_it_cannot_do(hip):
    from impdar_amd import _hip
    lib, ctx = hip.load(), hip.context()
    d = _hip.DeviceArray(ctx, (2, 20000), np.float32)
    try:
        # a prime, a factor 11, beyond the LDS, an odd real length, a real length whose half is below 16
        for mode, n in ((0, 97), (0, 1100), (0, 10000), (2, 625), (2, 30)):
            assert lib.impdar_fft_rows_any_dev(ctx, mode, 0, n, 2, d.ptr, d.ptr, 1.0) != 0, (mode, n)
        assert lib.impdar_fft_rows_dev(ctx, 0, 0, 48, 2, d.ptr, d.ptr, 1.0) != 0         # (the power-of-two entry stays what it was)
    finally:
        d.free()
