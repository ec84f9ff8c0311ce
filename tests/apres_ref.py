"""NumPy restatement of ``csrc/apres.hip``, written from the formulas: what the CPU tests put in the kernels' place and
what pins the fixtures of the reference.

  range conversion   per chirp x of snum samples: y = (x - mean(x)) win, X = DFT of y zero-padded to N = p snum,
                     spec = X mul / div, data = comp spec, Rfine = angle(data) / den (first order: lambdac angle / den);
                     spec and data for the first n bins, Rfine for all nf = N // 2
  stacking           the mean over runs of m consecutive rows
  phase difference   co[i] = S(s1 conj(s2)) / sqrt(S|s1|^2 S|s2|^2) over samples [i step, i step + 2 (win // 2))
"""
import numpy as np

U = 2.0 ** -53


def range_rows(raw, t, chunk=0):
    """``(spec, data, Rfine)`` of (rows, snum) chirps and the tables ``t`` of ``apres.range_tables``."""
    raw = np.asarray(raw, dtype=np.float64)
    N = t.p * raw.shape[1]
    y = (raw - raw.mean(axis=1, keepdims=True)) * t.win
    spec = np.fft.rfft(y, N, axis=1)[:, :t.nf] * t.scale_mul / t.scale_div
    data = t.comp * spec
    phi = np.angle(data)
    rfine = t.lambdac * phi / t.den if t.first_order else phi / t.den
    return np.ascontiguousarray(spec[:, :t.n]), np.ascontiguousarray(data[:, :t.n]), rfine


def dft_exact(y, N, nf):
    """The first nf bins of the length-N DFT of the rows of y, summed directly in long double."""
    y = np.asarray(y, dtype=np.longdouble)
    k = np.arange(nf, dtype=np.int64)[:, None] * np.arange(y.shape[1], dtype=np.int64)[None, :]
    ang = (-8 * np.arctan(np.longdouble(1))) * (k % N).astype(np.longdouble) / np.longdouble(N)
    kernel = np.cos(ang) + 1j * np.sin(ang)
    return np.array([(row[None, :] * kernel).sum(axis=1) for row in y])


def stack(data, groups, m):
    """Means over runs of m rows, summed in row order; NumPy's last step: / m for real, * (1 / m) for complex data."""
    data = np.asarray(data)
    out = np.zeros((groups, data.shape[1]), dtype=data.dtype)
    for g in range(groups):
        for i in range(m):
            out[g] = out[g] + data[g * m + i]
    if np.iscomplexobj(out):
        return out.real * (1.0 / m) + 1j * (out.imag * (1.0 / m))
    return out / m


def phase_diff(s1, s2, win, step):
    s1, s2 = np.asarray(s1, dtype=np.complex128), np.asarray(s2, dtype=np.complex128)
    h = win // 2
    idxs = np.arange(h, len(s1) - h, step).astype(int)
    co = np.empty(len(idxs), dtype=np.complex128)
    with np.errstate(invalid='ignore', divide='ignore'):
        for i, idx in enumerate(idxs):
            a, b = s1[idx - h:idx + h], s2[idx - h:idx + h]
            co[i] = np.sum(a * np.conj(b)) / np.sqrt(np.sum(np.abs(a)**2.) * np.sum(np.abs(b)**2.))
    return co


def spectrum_bar(N, norms):
    """E = 64 u log2(N) ||reference spectrum of the chirp||_2, per chirp: a radix transform's relative 2-norm error
    is below about 6 u log2 N (Higham), a Bluestein route's three transforms of length <= 4 N and three pointwise
    products about 18 u log2 N + 46 u, de-mean, window and scaling a few u more; no bin can be off by more than
    the 2-norm of the error."""
    return 64 * U * np.log2(N) * np.asarray(norms, dtype=np.float64)
