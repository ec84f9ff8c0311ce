"""The seven-pass form of the Stolt path on power-of-two sizes (csrc/stolt.hip, its stretch in csrc/stolt_kernels.h; round 6) restated in NumPy (CPU): the transform over the
TRACES first, the wavenumbers k >= 0 with ALL frequencies, the stretch along each row for both signs of the frequency -- the negative
half by the same interpolation, with the same weights, between the mirrored knots of the same row -- and a real inverse transform over the
traces at the end.  Held to the oracle's restatement of mig_python.py:126-208 (rfft2 / irfft2: the frequencies w >= 0 of all
wavenumbers).  The kernel itself is held to the oracle by tests/test_stolt_gpu.py."""
import numpy as np
import pytest

from oracle import mig_oracle


def stolt_rows_scheme(data, dt, trace_int, dist, vel, htaper, vtaper):
    snum, tnum = data.shape
    assert snum % 2 == 0 and tnum % 2 == 0
    nz, m = snum // 2, snum // 2 + 1
    tap = mig_oracle._apply_taper(data, htaper, vtaper).astype(data.dtype)          # (data * H) * V, cast back (:157)
    B = np.fft.fft(np.fft.rfft(tap.astype(np.float64), axis=1), axis=0)             # [w in FFT order][k = 0 .. tnum/2]
    ws = 2. * np.pi * np.fft.rfftfreq(snum, d=dt)
    kx = mig_oracle._kx(tnum, trace_int, dist)[:tnum // 2 + 1]
    kz = 2. * ws / vel
    dw = ws[1] - ws[0]
    H = np.zeros_like(B)
    for k in range(tnum // 2 + 1):
        kk = np.sqrt(kz[:nz] ** 2 + kx[k] ** 2)
        wq = np.minimum(vel / 2. * kk, ws[-1])
        i0 = np.clip(np.floor(wq / dw).astype(int), 0, m - 2)
        i0 = np.where(ws[i0] > wq, i0 - 1, i0)
        i0 = np.where(ws[np.minimum(i0 + 1, m - 1)] <= wq, np.minimum(i0 + 1, m - 2), i0)
        i0 = np.clip(i0, 0, m - 2)
        w = (wq - ws[i0]) / (ws[i0 + 1] - ws[i0])
        with np.errstate(invalid='ignore', divide='ignore'):
            sc = kz[:nz] / kk
        row = B[:, k]
        H[:nz, k] = ((1. - w) * row[i0] + w * row[i0 + 1]) * sc                      # w >= 0: as the reference (:171-198)
        mirrored = ((1. - w) * row[(snum - i0) % snum] + w * row[snum - i0 - 1]) * sc
        H[snum - np.arange(1, nz), k] = mirrored[1:]                                # w < 0: conj KK[w][-kx], out of the SAME row
        if k == 0:
            H[0, 0] = 0.                                                            # :200
    # (the zero-frequency row is zero -- kz = 0 scales it away -- and so is the Nyquist row: only KK[:nz] is filled)
    return np.fft.irfft(np.fft.ifft(H, axis=0), n=tnum, axis=1)


@pytest.mark.parametrize('snum,tnum', [(64, 64), (128, 32), (32, 256)])
def test_stretch_along_rows_with_mirrored_knots_is_the_references_stolt(snum, tnum):
    from impdar_amd import synth
    geo = synth.geometry(snum, tnum)
    data = synth.noise_radargram(snum, tnum, seed=snum + tnum)
    want = mig_oracle.stolt(data, geo['dt'], geo['trace_int'], geo['dist'], 1.68e8, 5, 7)
    got = stolt_rows_scheme(data, geo['dt'], geo['trace_int'], geo['dist'], 1.68e8, 5, 7)
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), np.max(np.abs(got - want)) / np.max(np.abs(want))
