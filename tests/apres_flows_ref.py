"""NumPy restatement of the kernels behind ``quadpol.find_cpe`` (reference
``src/impdar/lib/ApresData/_QuadPolProcessing.py:225-272, 303-355``), written from its formulas and pinned to its output
by ``test_apres_flows_cpu.py`` on every ``AF_QC*`` fixture.  It is the stand-in for the kernels when the host logic is
tested without a GPU and, in ``longdouble``, what the GPU sweeps are compared with.

The kernels' layout for a complex (n, m) image that goes through the filter is ONE float64 (n, 2 m) array: per row the
m real parts, then the m imaginary parts ("planes").

``row_argmin`` spells NumPy's rule for complex values out instead of calling ``np.argmin``, so that a slip can be
planted in it (``slip=``): the tests show that each of them is caught."""
import numpy as np

U = 2.0 ** -53


def to_planes(z):
    return np.hstack((np.real(z), np.imag(z))).astype(np.float64)


def to_complex(planes):
    m = planes.shape[1] // 2
    out = np.empty((planes.shape[0], m), dtype=np.complex128)
    out.real, out.imag = planes[:, :m], planes[:, m:]
    return out


def power(HV, dtype=np.complex128):
    """``10 log10(HV^2)`` in complex arithmetic."""
    z = np.asarray(HV).astype(dtype)
    with np.errstate(all='ignore'):
        return z.real.dtype.type(10.) * np.log10(z * z)


def power_anomaly(HV, dtype=np.complex128):
    """The power minus its row mean over the elements without a NaN in either part (``np.nanmean``)."""
    import warnings
    P = power(HV, dtype)
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        return P - np.nanmean(P, axis=1)[:, None]


def anomaly_planes(HV):
    return to_planes(power_anomaly(HV))


def lowpass_planes(planes, spec):
    """SciPy's ``filtfilt`` along range of every column of the planes."""
    from scipy.signal import filtfilt
    _, b, a, _ = spec
    return filtfilt(b, a, planes, axis=0)


def row_argmin(planes, c0, c1, slip=None):
    """Per row the column in ``[c0, c1)`` that ``np.argmin`` picks among complex values: the first with a NaN in
    either part, else the least real part, then the least imaginary part, then the lowest column."""
    n, m = planes.shape[0], planes.shape[1] // 2
    stop = c1 + 1 if slip == 'window_end_inclusive' else c1
    out = np.empty((n,), dtype=np.int32)
    for j in range(n):
        best = None
        for c in range(c0, min(stop, m)):
            re, im = planes[j, c], planes[j, m + c]
            if np.isnan(re) or np.isnan(im):
                if slip == 'nan_skipped':
                    continue
                best = (re, im, c)
                break
            if best is None:
                best = (re, im, c)
            elif re < best[0] or (re == best[0] and im < best[1]):
                best = (re, im, c)
            elif slip == 'tie_to_higher_index' and re == best[0] and im == best[1]:
                best = (re, im, c)
        out[j] = c0 if best is None else best[2]
    return out


def find_cpe(HV, spec, c0, c1, filtered=False, slip=None):
    """The three stages: ``(idxs, filtered planes)`` or the indices alone."""
    planes = lowpass_planes(anomaly_planes(HV), spec)
    idxs = row_argmin(planes, c0, c1, slip=slip)
    return (idxs, planes) if filtered else idxs


def gather(image, idx):
    image = np.asarray(image)
    return image[np.arange(image.shape[0]), np.asarray(idx)]


def anomaly_bar(HV):
    """Elementwise bar, real and imaginary planes, for a float64 evaluation of the anomaly against the longdouble one,
    where the latter is finite.  Per element of P: the two parts of HV^2 carry 2 u |HV^2| each, so |HV^2| is off by
    at most 4 u relative (with hypot's own rounding) and the angle by 3 u; 10 log10(e) = 4.35 turns that into 18 u and
    13 u; log and atan2 are good to 2 ulp and two products follow: 4 u |P.re| and (8 + 4) u |P.im| at most.  The mean
    of m elements adds the mean of those bars, a sum of ceil(m / 64) + 6 additions per lane and butterfly, and the
    product with 1 / count: (ceil(m / 64) + 9) u mean|P|."""
    P = power(HV, np.clongdouble)
    ok = ~(np.isnan(P.real) | np.isnan(P.imag))
    m = P.shape[1]
    out = []
    for part, a, b in ((P.real, 18., 4.), (P.imag, 13., 12.)):
        mag = np.where(ok, np.abs(part), 0.).astype(np.float64)
        elem = U * (a + b * mag)
        cnt = np.maximum(ok.sum(axis=1), 1)[:, None]
        mean_elem = np.where(ok, elem, 0.).sum(axis=1)[:, None] / cnt
        mean_mag = mag.sum(axis=1)[:, None] / cnt
        out.append(elem + mean_elem + (np.ceil(m / 64.) + 9.) * U * mean_mag)
    return np.hstack(out)


def kinds(x):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isnan(x), 1, np.where(np.isposinf(x), 2, np.where(np.isneginf(x), 3, 0)))
