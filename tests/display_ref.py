"""NumPy restatement of what the display unit computes (csrc/display.hip, impdar_amd/display.py), for the tests: the two
order statistics of every percentage from a sort, NumPy's interpolation between them, the flattened image as the
reference's trace loop builds it (src/impdar/lib/plot.py:240-254) and its offsets (:905-917), plus the loader of the FD*
fixtures."""
import glob
import os
import types

import numpy as np

NO_SHIFT = -2 ** 31


def ranks(n, q):
    """(lo, hi, g): the ranks floor((n - 1) q / 100) and min(lo + 1, n - 1) and the fraction between them, in float64 as
    NumPy forms them."""
    v = (n - 1) * np.true_divide(np.asarray(q, dtype=np.float64), 100.0)
    lo = np.floor(v)
    return lo.astype(np.int64), np.minimum(lo + 1, n - 1).astype(np.int64), v - lo


def order_stats(window, q, skip_nan=True):
    """(N, nan_count, vals): vals[2 i], vals[2 i + 1] the values of rank lo, hi of q[i] among the window's values that
    are no NaN, from a full sort; None where there is nothing to rank (n == 0, or a NaN that is not skipped)."""
    flat = np.asarray(window).reshape(-1)
    nan = int(np.isnan(flat).sum())
    n = flat.size - nan
    if n == 0 or (nan and not skip_nan):
        return flat.size, nan, None
    s = np.sort(flat[~np.isnan(flat)])
    lo, hi, _ = ranks(n, np.atleast_1d(q))
    vals = np.empty((2 * lo.size,), dtype=flat.dtype)
    vals[0::2], vals[1::2] = s[lo], s[hi]
    return flat.size, nan, vals


def lerp(a, b, g):
    with np.errstate(invalid='ignore', over='ignore'):
        d = b - a
        low = np.asarray(a + d * g, dtype=np.float64)
        high = np.asarray(b - d * (1.0 - g), dtype=np.float64)
    return np.where(g >= 0.5, high, low)


def percentile(window, q, skip_nan=True):
    """np.percentile(window[~isnan(window)], q) -- or of the window, NaN and all -- from the sort and the lerp."""
    N, nan, vals = order_stats(window, q, skip_nan)
    if N == 0 or (N - nan == 0 and skip_nan):
        raise IndexError('index -1 is out of bounds for axis 0 with size 0')
    qa = np.asarray(q, dtype=np.float64)
    if vals is None:
        out = np.full(np.atleast_1d(qa).shape, np.nan)
    else:
        out = lerp(vals[0::2], vals[1::2], ranks(N - nan, np.atleast_1d(qa))[2])
    return out[0] if qa.ndim == 0 else out


def get_offset(samp2_row):
    """(offset, mask) of the layer whose centre rows are samp2_row."""
    offset = int(np.nanmean(samp2_row)) - samp2_row
    return offset, np.isnan(samp2_row)


def flatten_loop(data, offset):
    """Trace by trace: a NaN offset leaves the trace NaN, int(offset) == 0 copies it, a negative offset moves it up and
    a positive one down, and an offset of snum rows or more leaves nothing."""
    snum = data.shape[0]
    out = np.full_like(data, np.nan)
    for j in range(data.shape[1]):
        if np.isnan(offset[j]):
            continue
        k = int(offset[j])
        if k == 0:
            out[:, j] = data[:, j]
        elif abs(offset[j]) < snum and k < 0:
            out[:k, j] = data[-k:, j]
        elif abs(offset[j]) < snum:
            out[k:, j] = data[:-k, j]
    return out


def shifts(offset, snum):
    off = np.asarray(offset, dtype=np.float64)
    k = np.array([NO_SHIFT if np.isnan(o) else int(max(-snum, min(snum, o))) for o in off], dtype=np.int64)
    return k.astype(np.int32)


def flatten_gather(data, shift):
    """out[i, j] = data[i - shift[j], j] where that row exists, NaN elsewhere: the kernel's statement."""
    snum = data.shape[0]
    out = np.full_like(data, np.nan)
    for j, k in enumerate(shift):
        if k == NO_SHIFT:
            continue
        i = np.arange(snum)
        ok = (i - int(k) >= 0) & (i - int(k) < snum)
        out[i[ok], j] = data[i[ok] - int(k), j]
    return out


def fixture_names(golden_dir):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(golden_dir, 'FD[0-9][0-9]_*.npz')))


def load_fixture(golden_dir, name):
    with np.load(os.path.join(golden_dir, name + '.npz')) as z:
        return {k: z[k] for k in z.files}


def picks_of(g):
    """A stand-in for the Picks object with what the plots read."""
    if 'samp2' not in g:
        return None
    return types.SimpleNamespace(samp1=g['samp1'], samp2=g['samp2'], samp3=g['samp3'], power=g['power'],
                                 picknums=[int(p) for p in g['picknums']])


def fill_dat(d, g, dtype=None):
    """Give a RadarData (or a bare namespace) the attributes of fixture g that the plots read."""
    data = g['data'] if dtype is None else g['data'].astype(dtype)
    d.data = data.copy()
    d.snum, d.tnum = data.shape
    d.travel_time = g['travel_time'].copy()
    d.dist = g['dist'].copy()
    d.nmo_depth = None
    d.long, d.lat = g['long'].copy(), g['lat'].copy()
    d.x_coord = d.y_coord = None
    d.fn = None
    d.picks = picks_of(g)
    return d
