"""NumPy restatements of the three spectra (the reference's ``plot_ft`` / ``plot_hft`` arithmetic and
``scipy.signal.periodogram`` of every trace, ``src/impdar/lib/plot.py:310-312, 346-347, 654-674``) that work in whatever
float dtype the data has -- ``longdouble`` included, which SciPy's periodogram does not take -- and the yardstick the
GPU tests measure errors with.  ``tests/golden/make_golden_spectra.py`` forms the expected ``*_hi`` arrays with these;
``tests/test_spectra_cpu.py`` holds ``periodogram`` to SciPy's own on every fixture.
"""
import glob
import os

import numpy as np

U = 2.0 ** -53
PARAMS = ((None, 'spectrum'), ('hamming', 'density'), ('hann', 'spectrum'))
DT = 1.0e-8          # the sampling step of every fixture: fs = 1 / DT
# 8 x the largest rho_ref / Y of the reference's own float64 results against their longdouble evaluation over all
# fixtures (make_golden_spectra.py prints the table; DESIGN.md 4.13 holds it)
C = 30.0           # 8 x 3.7338 (the horizontal spectrum of the 16384 x 2 flat case) = 29.87


def mean_spectrum(data, axis):
    """``mean(|fft(data, axis)|^2)`` over the other axis, in the dtype of ``data``."""
    return np.mean(np.abs(np.fft.fft(data, axis=axis)) ** 2.0, axis=1 - axis)


def window(name, n):
    from scipy.signal import get_window
    return np.asarray(get_window(name or 'boxcar', n), dtype=np.float64)


def scale_of(w, fs, scaling):
    if scaling == 'density':
        return 1.0 / (fs * (w * w).sum())
    if scaling == 'spectrum':
        return 1.0 / w.sum() ** 2
    raise ValueError('Unknown scaling: %r' % scaling)


def periodogram(data, fs, win=None, scaling='density'):
    """``scipy.signal.periodogram(data[:, t], fs, win, scaling=scaling)[1]`` of every trace as a (snum // 2 + 1, tnum)
    image, in the dtype of ``data``: detrend 'constant', the float64 window widened to that dtype, ``|rfft|^2 * scale``,
    every bin but the first (and, for even snum, the last) doubled."""
    data = np.asarray(data)
    n = data.shape[0]
    w = window(win, n).astype(data.dtype)
    x = (data - data.mean(axis=0)) * w[:, None]
    spec = np.fft.rfft(x, axis=0)
    power = (np.conjugate(spec) * spec).real * scale_of(w, data.dtype.type(fs), scaling)
    if n % 2:
        power[1:] *= 2
    else:
        power[1:-1] *= 2
    return power


def yardstick_mean(data, axis):
    """``Y = u (log2 n + log2 m + 2) n mean_m ||x||^2`` of a mean spectrum along ``axis``: one number for all bins."""
    data = np.asarray(data, dtype=np.float64)
    n, m = data.shape[axis], data.shape[1 - axis]
    return U * (np.log2(n) + np.log2(m) + 2.0) * n * np.mean(np.sum(data * data, axis=axis))


def yardstick_periodogram(data, fs, win, scaling):
    """``Y`` per trace (tnum,): the window-weighted undetrended trace enters, times ``2 scale``; m = 1."""
    data = np.asarray(data, dtype=np.float64)
    n = data.shape[0]
    w = window(win, n)
    x = data * w[:, None]
    return U * (np.log2(n) + 2.0) * n * np.sum(x * x, axis=0) * 2.0 * scale_of(w, fs, scaling)


def load_fixture(golden_dir, name):
    """A fixture is one or more files ``name.npz``, ``name_p1.npz`` ...: every array sits in one of them."""
    out = {}
    for path in sorted(glob.glob(os.path.join(golden_dir, name + '.npz')) + glob.glob(os.path.join(golden_dir, name + '_p[0-9]*.npz'))):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


def fixture_names(golden_dir):
    import re
    names = (os.path.basename(p)[:-4] for p in glob.glob(os.path.join(golden_dir, 'FS[0-9][0-9]_*.npz')))
    return sorted(n for n in names if not re.search(r'_p\d+$', n))
