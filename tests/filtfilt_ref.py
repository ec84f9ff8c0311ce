"""Test infrastructure for the two filtfilt kernels (csrc/preproc.hip along time, csrc/hpass.hip along traces):
well-conditioned (b, a) designs at every coefficient count they take, and a long-double restatement of
scipy.signal.filtfilt.

At 0.2-0.8 of Nyquist a Butterworth band pass of every order up to 16 is well conditioned as a transfer function,
so SciPy's float64 filtfilt is within 1e-13 of the long-double result (tests/test_filtfilt_cpu.py) and a kernel that
runs SciPy's float64 recurrence can be held to 1e-12 at every count.  The long-double twin is the CPU oracle's
filtfilt run in np.longdouble: same odd extension in the data's dtype, same float64 lfilter_zi (SciPy's solve, which
the kernels receive as an input too), so the comparison measures only the rounding of the recurrence."""
import numpy as np

from oracle import preproc_oracle as po

NCOEF_MIN = 2
VERT_MAX = 33    # FF_MAX_COEF in csrc/preproc.hip
HORIZ_MAX = 17   # HP_MAX_COEF in csrc/hpass.hip

# vertical_band_pass(10, 40 MHz) at dt = 1e-8 (0.2-0.8 of Nyquist): (filttype, order) pairs of 23-33 coefficients that
# test_filtfilt_cpu.py proves well conditioned.  cheby1 (5 dB ripple) stops at order 11: order 12 reaches 1.2e-13 on
# some noise and order 16 3.6e-12.
API_BAND = (10., 40.)
API_DESIGNS = [('butter', n) for n in range(11, 17)] + [('bessel', n) for n in range(11, 17)] + [('cheb', 11)]


def design(ncoef):
    """(b, a), ``ncoef`` coefficients each: butter(N, [0.2, 0.8], 'bandpass') for ncoef = 2N + 1; for ncoef = 2N + 2
    the same design with one more real zero (b * [1, 0.5]) and pole (a * [1, -0.3])."""
    from scipy import signal
    b, a = signal.butter((ncoef - 1) // 2, [0.2, 0.8], 'bandpass')
    if ncoef % 2 == 0:
        b = np.convolve(b, [1.0, 0.5])
        a = np.convolve(a, [1.0, -0.3])
    assert len(b) == len(a) == ncoef, (ncoef, len(b), len(a))
    return b, a


def spec(b, a):
    """(b, a, zi) of one of the designs above as the C ABI takes them: float64 arrays, zi = SciPy's lfilter_zi."""
    from scipy import signal
    return tuple(np.ascontiguousarray(v, dtype=np.float64) for v in (b, a, signal.lfilter_zi(b, a)))


def filtfilt_ld(b, a, x):
    """scipy.signal.filtfilt(b, a, x, axis=0) with both passes in np.longdouble (returned in np.longdouble)."""
    return po.filtfilt(b, a, x, dtype=np.longdouble)


def rel_err(got, want):
    """max |got - want| / max |want|, in long double."""
    want = np.asarray(want, dtype=np.longdouble)
    return float(np.max(np.abs(np.asarray(got, dtype=np.longdouble) - want)) / np.max(np.abs(want)))
