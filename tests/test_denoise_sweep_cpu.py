"""The denoise sweep without a GPU.  ``denoise_sweep.py`` has the cases, the long-double Wiener reference and the bars;
this file runs the sweep on a float64 NumPy restatement of the kernels' order of operations:

  wn_vsum_kernel   strips of ``WN_RS`` rows, the strip's pivot, the first window summed row by row, then the running
                   ``(s - leaving) + entering``; zero-padded rows enter as 0 - p; the count of non-finite values
  wn_hsum_kernel   ``T`` at column 0 (strided partial sums, the butterfly), per tile ``S = (T + Qex) - Pex`` from the
                   thread-local prefixes and the wave scans, the carry ``T += totQ - totP``, the ``n == 1`` shortcut, the
                   padded columns' terms, mean and variance by each dtype's rule, the fixed-order noise
  median           the dispatch by N, the (``MD_TR`` x ``MD_TW``) tile with its reflected halo (held to ``MD_LDS``), the
                   +inf padding to NB, ``md_reflect``, the rank (a sort stands for the bitonic network and the radix
                   select)

That the restatement passes shows that every bar is attainable in float64 on exactly these inputs, and keeps the
references under test where there is no GPU.  Six planted slips must each fail the sweep (``SLIPS``); the case counts
and the seams the cases cross are asserted from the kernels' constants.

The restatement's own margins, worst |diff| / bar and worst noise error / bar per family (``-s`` prints them; a
record of the restatement, not a bar):
  base             0.0016   0.0000
  band             0.0175   0.0179      (66 x 2049 and 2050 x 5 with the band on the pivot row)
  nonfinite        0.0007   (noise given)
  unit window      0.0000   0.0001
  widest window    0.0000   0.0000
With the padded columns entered as z (0 - p) and z p**2, as the kernel had them before this sweep, the widest window
(2 x (2**30 - 1) on 3 x 5, float64) came out at 5.701 of the output bar, here and on the device alike: all but five
columns of every window are padding, and E[(x - p)**2] - E[x - p]**2 cancels to a variance 2e8 times smaller than p**2.
``wn_hsum_kernel`` now takes the variance about the mean of the pivots (p in the array, 0 in the padding).
"""
import numpy as np
import pytest

import denoise_sweep as ds
from denoise_sweep import (MD_LDS, MD_NB, MD_SMALL, MD_TR, MD_TW, WN_BLOCK, WN_PER, WN_RS, WN_TILE)

WN_GROUPS = ds.wiener_groups()
MD_GROUPS = ds.median_groups()
WIDEST = ((3, 5), (2, ds.HOR_WIN_MAX))

SLIPS = ('tile_carry', 'pad_term', 'strip_pivot', 'win_shift', 'rank_low', 'mirror')


# ------------------------------------------------------------------------------------------------ Wiener restated
def pivot(x, t):
    """``wn_pivot``: a finite value of the middle row of the strip that holds row t, else 0."""
    snum, tnum = x.shape
    r = min((t // WN_RS) * WN_RS + WN_RS // 2, snum - 1)
    v = x[r, tnum // 2]
    return float(v) if np.isfinite(v) else 0.0


def vsum(x, m):
    """``wn_vsum_kernel``: V1 = sum (x - p), V2 = sum (x - p)**2 (float32: sum fl32(x * x)), Vc = non-finite count."""
    snum, tnum = x.shape
    lo, hi = m // 2, (m - 1) // 2
    f32 = x.dtype == np.float32
    finite = np.isfinite(x)
    xd = np.where(finite, x, 0).astype(np.float64)
    sq32 = (np.where(finite, x, 0) * np.where(finite, x, 0)).astype(np.float64) if f32 else None
    V1, V2, Vc = np.empty(x.shape), np.empty(x.shape), np.empty(x.shape, dtype=np.int64)
    for s0 in range(0, snum, WN_RS):
        s1 = min(s0 + WN_RS, snum)
        p = pivot(x, s0)

        def term(r):
            if r < 0 or r >= snum:                                  # a zero-padded row
                y = np.full(tnum, 0.0 - p)
                return y, (np.zeros(tnum) if f32 else y * y), np.zeros(tnum, dtype=np.int64)
            y = np.where(finite[r], xd[r] - p, 0.0)
            return y, np.where(finite[r], sq32[r] if f32 else y * y, 0.0), (~finite[r]).astype(np.int64)

        a1, a2, c = np.zeros(tnum), np.zeros(tnum), np.zeros(tnum, dtype=np.int64)
        for r in range(s0 - lo, s0 + hi + 1):
            t1, t2, tc = term(r)
            a1, a2, c = a1 + t1, a2 + t2, c + tc
        for t in range(s0, s1):
            V1[t], V2[t], Vc[t] = a1, a2, c
            if t + 1 < s1:
                l1, l2, lc = term(t - lo)
                e1, e2, ec = term(t + hi + 1)
                a1, a2, c = (a1 - l1) + e1, (a2 - l2) + e2, c + (ec - lc)
    return V1, V2, Vc


def block_sum(v):
    """``wn_block_sum`` of (..., WN_BLOCK): the xor butterfly in each wave, then (w0 + w1) + (w2 + w3)."""
    v = v.reshape(v.shape[:-1] + (WN_BLOCK // 64, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    red = v[..., 0]
    return (red[..., 0] + red[..., 1]) + (red[..., 2] + red[..., 3])


def block_scan(v):
    """``wn_block_scan`` of (..., threads), threads a multiple of 64 (waves beyond hold zeros and change nothing): the
    exclusive prefix of every thread and the total."""
    waves = v.shape[-1] // 64
    inc = v.reshape(v.shape[:-1] + (waves, 64)).copy()
    o = 1
    while o < 64:
        nxt = inc.copy()
        nxt[..., o:] = inc[..., o:] + inc[..., :-o]
        inc, o = nxt, o << 1
    ex = np.zeros_like(inc)
    ex[..., 1:] = inc[..., :-1]
    before = np.zeros(inc.shape[:-1])
    tot = np.zeros(inc.shape[:-2])
    for q in range(waves):
        before[..., q] = tot
        tot = tot + inc[..., q, 63]
    return (ex + before[..., None]).reshape(v.shape), tot


def hsum(x, V, m, n, noise, slip=None):
    """``wn_hsum_kernel`` on the stacked sums ``V`` (3, snum, tnum), every row at once.  ``noise`` None: MODE 0, the
    row sums of lVar; else MODE 1, the output."""
    snum, tnum = x.shape
    f32 = x.dtype == np.float32
    lo, hi = (n // 2, (n - 1) // 2) if slip != 'win_shift' else ((n - 1) // 2, n // 2)
    N = float(m) * float(n)
    rows = np.arange(snum)
    prow = np.minimum(rows + 1, snum - 1) if slip == 'strip_pivot' else rows
    p = np.array([pivot(x, t) for t in prow])[:, None]
    e0 = min(hi, tnum - 1)
    part = np.zeros((3, snum, WN_BLOCK))
    for j in range(0, e0 + 1, WN_BLOCK):
        w = min(WN_BLOCK, e0 + 1 - j)
        part[:, :, :w] = part[:, :, :w] + V[:, :, j:j + w]
    T = block_sum(part)                                             # (3, snum)
    acc = np.zeros((snum, WN_BLOCK))
    out = np.empty((snum, tnum))
    for c0 in range(0, tnum, WN_TILE):
        ncol = min(WN_TILE, tnum - c0)
        threads = -(-ncol // (64 * WN_PER)) * 64
        j = c0 + np.arange(threads * WN_PER, dtype=np.int64)
        a, b = j - lo, j + hi + 1
        ina, inb = (j < tnum) & (a >= 0) & (a < tnum), (j < tnum) & (b < tnum)
        P = np.where(ina, V[:, :, np.clip(a, 0, tnum - 1)], 0.0).reshape(3, snum, threads, WN_PER)
        Q = np.where(inb, V[:, :, np.clip(b, 0, tnum - 1)], 0.0).reshape(3, snum, threads, WN_PER)
        S, tots = [], []
        for X in (P, Q):
            inc = np.cumsum(X, axis=-1)                             # thread-local inclusive prefixes, in order
            ex, tot = block_scan(inc[..., -1])
            own = np.concatenate([np.zeros_like(inc[..., :1]), inc[..., :-1]], axis=-1)
            S.append((ex[..., None] + own).reshape(3, snum, threads * WN_PER)[:, :, :ncol])
            if slip == 'tile_carry':                                # the totals taken one column short
                short = X.copy()
                short[..., -1, -1] = 0.0
                tot = block_scan(np.cumsum(short, axis=-1)[..., -1])[1]
            tots.append(tot)
        s = (T[:, :, None] + S[1]) - S[0]
        if n == 1:
            s = V[:, :, c0:c0 + ncol].astype(np.float64)
        j = j[:ncol]
        npc = np.maximum(lo - j, 0) + np.maximum(j + hi - (tnum - 1), 0)
        s1, s2, sc = s[0], s[1], s[2]
        z = npc.astype(np.float64) * float(m) if slip != 'pad_term' else np.zeros(ncol)
        eu = s1 / N                                                 # about the pivot, in-array columns only
        mean = p + np.where(z > 0, s1 - z * p, s1) / N
        if f32:
            var = s2 / N - mean * mean
        else:
            var = s2 / N - eu * eu
            var = np.where(z > 0, var + z * (p * (2.0 * s1 + p * (N - z))) / (N * N), var)
        mean, var = np.where(sc > 0, np.nan, mean), np.where(sc > 0, np.nan, var)
        if noise is None:
            v4 = np.zeros((snum, threads * WN_PER))
            v4[:, :ncol] = var
            v4 = v4.reshape(snum, threads, WN_PER)
            for u in range(WN_PER):
                acc[:, :threads] = acc[:, :threads] + v4[:, :, u]
        else:
            xv = x[:, c0:c0 + ncol].astype(np.float64)
            with np.errstate(divide='ignore', invalid='ignore'):
                out[:, c0:c0 + ncol] = np.where(var < noise, mean, (xv - mean) * (1.0 - noise / var) + mean)
        T = T + (tots[1] - tots[0])
    return block_sum(acc) if noise is None else out


def wiener_restated(data, m, n, noise=None, slip=None):
    """``wn_run``: ``(out, noise_used)``."""
    x = np.asarray(data)
    snum, tnum = x.shape
    V = np.stack([a.astype(np.float64) for a in vsum(x, m)])
    if noise is None:
        rowsum = hsum(x, V, m, n, None, slip)
        part = np.zeros(WN_BLOCK)
        for t in range(0, snum, WN_BLOCK):                         # wn_noise_kernel
            w = min(WN_BLOCK, snum - t)
            part[:w] = part[:w] + rowsum[t:t + w]
        noise = float(block_sum(part) / float(snum * tnum))
        if noise == 0.0:
            raise ValueError(ds.NOISE_MESSAGE)
    return hsum(x, V, m, n, float(noise), slip), float(noise)


# ------------------------------------------------------------------------------------------------ median restated
def md_reflect(j, L, slip=None):
    """``md_reflect`` (d c b a | a b c d | d c b a); the 'mirror' slip does not repeat the edge sample."""
    if slip == 'mirror':
        if L == 1:
            return np.zeros_like(j)
        j = np.mod(j, 2 * L - 2)
        return np.where(j < L, j, 2 * L - 2 - j)
    j = np.mod(j, 2 * L)
    return np.where(j < L, j, 2 * L - 1 - j)


def median_kernel(m, n):
    """``md_launch``: the register width NB of med_small_kernel, or None for med_radix_kernel."""
    for nb in MD_NB:
        if m * n <= nb:
            return nb
    return None


def median_restated(data, m, n, slip=None, seen=None):
    x = np.asarray(data)
    snum, tnum = x.shape
    N, lo_v, lo_h = m * n, m // 2, n // 2
    kth = (N - 1) // 2 if slip == 'rank_low' else N // 2
    nb = median_kernel(m, n)
    if seen is not None:
        seen.add(nb)
    out = np.empty_like(x)
    if nb is None:                                                  # med_radix_kernel: a window per output
        cols = md_reflect(np.arange(tnum)[:, None] - lo_h + np.arange(n)[None, :], tnum, slip)       # (tnum, n)
        step = max(1, 20000000 // (tnum * N))
        for t0 in range(0, snum, step):
            t = np.arange(t0, min(t0 + step, snum))
            rws = md_reflect(t[:, None] - lo_v + np.arange(m)[None, :], snum, slip)                 # (rows, m)
            w = x[rws[:, None, :, None], cols[None, :, None, :]].reshape(len(t), tnum, N)
            out[t] = np.partition(w, kth, axis=-1)[:, :, kth]
        return out
    LW, LH = MD_TW + n - 1, MD_TR + m - 1
    assert LW * LH <= MD_LDS, 'the halo tile of a %d x %d window does not fit its LDS array' % (m, n)
    for r0 in range(0, snum, MD_TR):
        for c0 in range(0, tnum, MD_TW):
            tile = x[np.ix_(md_reflect(r0 - lo_v + np.arange(LH), snum, slip), md_reflect(c0 - lo_h + np.arange(LW), tnum, slip))]
            w = np.lib.stride_tricks.sliding_window_view(tile, (m, n)).reshape(MD_TR, MD_TW, N)
            v = np.full((MD_TR, MD_TW, nb), np.inf, dtype=x.dtype)
            v[:, :, :N] = w
            r = np.sort(v, axis=-1)[:, :, kth]
            out[r0:r0 + MD_TR, c0:c0 + MD_TW] = r[:min(MD_TR, snum - r0), :min(MD_TW, tnum - c0)]
    return out


# ------------------------------------------------------------------------------------------------ the sweep
RECORD = {}


def _record(family, ratio, nratio=None):
    old = RECORD.get(family, (0.0, 0.0))
    RECORD[family] = (max(old[0], ratio), max(old[1], nratio or 0.0))
    print('%s: worst |diff| = %.4f of the bar, worst noise error = %.4f of the bar' % ((family,) + RECORD[family]))


@pytest.mark.parametrize('key', list(WN_GROUPS))
def test_wiener_sweep(key):
    ratio, nratio = ds.sweep_wiener(wiener_restated, WN_GROUPS[key])
    _record('wiener ' + key.split('-')[0], ratio, nratio)


@pytest.mark.parametrize('shape', ds.WN_SHAPES, ids=[ds.SHAPE_NAMES[s] for s in ds.WN_SHAPES])
def test_wiener_unit_window(shape):
    """The (1, 1) window.  float64: lVar is exactly 0, the reference's error on every shape.  float32: lVar is
    fl32(x * x) - x * x, the rounding error of the float32 square, and its mean is not zero on any of the shapes (1e-13
    to 5e-8 in size, negative on eight of them): the long-double form and the restatement agree that nothing is raised,
    and the output is lMean = x to the bar.  Had a shape only exact squares, both would raise (``check_wiener``)."""
    ratio, nratio = ds.check_wiener_unit_window(wiener_restated, shape)
    _record('wiener unit window', ratio, nratio)


def test_wiener_widest_window():
    """The widest window of the argument check: the restatement's cost does not depend on the window either."""
    shape, win = WIDEST
    cases = [ds.WnCase(shape, win, dt, 'base', None) for dt in ds.DTYPES]
    _record('wiener widest window', *ds.sweep_wiener(wiener_restated, cases))


@pytest.mark.parametrize('key', list(MD_GROUPS))
def test_median_sweep(key):
    seen = set()
    ds.sweep_median(lambda x, m, n: median_restated(x, m, n, seen=seen), MD_GROUPS[key])
    N = MD_GROUPS[key][0].win[0] * MD_GROUPS[key][0].win[1]
    assert seen == {min([nb for nb in MD_NB if N <= nb], default=None)}


@pytest.mark.parametrize('key', list(MD_GROUPS))
def test_median_reference_is_scipys(key):
    """``median_closed`` against SciPy on every case.  SciPy 1.15 returns values that occur nowhere in the input for
    a 65 x 1 window on 2 x 3 (by hand: row 0 of a column is taken 33 times and row 1 32 times, which is what
    ``median_closed`` returns), in either orientation.  Only a result of that kind is set aside: SciPy's filter then
    runs on the array extended by ``numpy.pad(mode='symmetric')``, the same rule, so that no window of a kept output
    reaches SciPy's own boundary."""
    ndimage = pytest.importorskip('scipy.ndimage')
    for case in MD_GROUPS[key]:
        x = ds.median_input(case.shape, case.dtype)
        (snum, tnum), (m, n) = case.shape, case.win
        got = ndimage.median_filter(x, size=case.win, mode='reflect')
        if not np.isin(got, x).all():
            print('%s: scipy.ndimage returns values that are not in the input; extending the array by numpy.pad' % (case,))
            wide = np.pad(x, ((m // 2, (m - 1) // 2), (n // 2, (n - 1) // 2)), mode='symmetric')
            got = ndimage.median_filter(wide, size=case.win, mode='reflect')[m // 2:m // 2 + snum, n // 2:n // 2 + tnum]
        assert got.dtype == x.dtype and np.array_equal(got, ds.median_want(*case)), case


# ------------------------------------------------------------------------------------------------ planted slips
def first_failure(sweep, cases):
    for case in cases:
        try:
            sweep(case)
        except AssertionError as err:
            return case, str(err).strip().splitlines()[0]
    return None


@pytest.mark.parametrize('slip', SLIPS)
def test_planted_slip_is_caught(slip):
    if slip in ('rank_low', 'mirror'):
        found = first_failure(lambda c: ds.check_median(lambda x, m, n: median_restated(x, m, n, slip=slip), c),
                              ds.all_cases(MD_GROUPS))
    else:
        found = first_failure(lambda c: ds.check_wiener(lambda x, m, n, noise: wiener_restated(x, m, n, noise, slip=slip), c),
                              ds.all_cases(WN_GROUPS))
    assert found is not None, 'the sweep passes with the slip %r planted: it lacks a shape' % slip
    print('slip %s caught: %s' % (slip, found[1][:240]))


@pytest.mark.parametrize('slip', ('tile_carry', 'pad_term', 'strip_pivot', 'win_shift'))
@pytest.mark.parametrize('kind', ('base', 'band', 'nonfinite'))
def test_wiener_slip_is_caught_by_every_family_that_can_see_it(slip, kind):
    """Each family of inputs catches each Wiener slip on its own (a pivot slip needs more than one strip, which every
    family has)."""
    cases = ds.all_cases({k: v for k, v in WN_GROUPS.items() if k.startswith(kind)})
    fn = lambda x, m, n, noise: wiener_restated(x, m, n, noise, slip=slip)
    assert first_failure(lambda c: ds.check_wiener(fn, c), cases) is not None


# ------------------------------------------------------------------------------------------------ the cases themselves
def test_case_counts():
    wn, md = ds.all_cases(WN_GROUPS), ds.all_cases(MD_GROUPS)
    assert (len(WN_GROUPS), len(wn)) == (129, 300)                # tests, cases: both dtypes, two bands to a test
    assert (len(MD_GROUPS), len(md)) == (109, 217)                 # both dtypes but for the 65537-row case
    have = {(c.shape, c.win) for c in wn if c.variant == 'base'}
    for dt in ds.DTYPES:
        for shape in ds.FULL_SHAPES:
            for win in ds.WN_WINDOW_NAMES:
                assert ds.WnCase(shape, win, dt, 'base', None) in wn
        for shape in ds.WN_SHAPES:
            for win in ds.EVERY_SHAPE_WINDOWS:
                assert ds.WnCase(shape, win, dt, 'base', None) in wn
        for shape in ds.FULL_SHAPES:
            for win in ds.MD_BOUNDARY_WINDOWS:
                assert ds.MdCase(shape, win, dt) in md
    assert len(have) == 3 * len(ds.WN_WINDOW_NAMES) + 3 * (len(ds.WN_SHAPES) - 3) + 6
    assert ds.MdCase((65537, 3), (5, 13), 'float32') in md and ds.MdCase((65537, 3), (5, 13), 'float64') not in md
    assert sorted(ds.MD_WINDOWS) == sorted(list(MD_NB) + [nb + 1 for nb in MD_NB])
    assert all(m * n == N for N, ws in ds.MD_WINDOWS.items() for m, n in ws)


def test_every_seam_is_crossed():
    hit = ds.seams(ds.all_cases(WN_GROUPS), ds.all_cases(MD_GROUPS), ds.WN_SHAPES, WIDEST)
    for seam, cases in hit.items():
        assert cases, 'no case crosses: ' + seam
        print('%-62s %4d cases, first %s' % (seam, len(cases), tuple(cases[0])))
    assert (MD_TR + MD_SMALL - 1) * MD_TW == MD_LDS >= MD_TR * (MD_TW + MD_SMALL - 1)
    assert WN_TILE == WN_BLOCK * WN_PER


def test_band_rows_and_the_pivot():
    """Rows 28..36 hold the pivot row of strip 0 and leave rows of that strip outside; rows 4..12 do not hold it."""
    pivot_row = WN_RS // 2
    on, off = ds.BAND_ON_PIVOT, ds.BAND_OFF_PIVOT
    assert on[0] <= pivot_row <= on[1] and on[0] > 0 and on[1] < WN_RS - 1
    assert not off[0] <= pivot_row <= off[1] and off[1] < WN_RS
    for shape in ds.WN_SHAPES:
        if shape[0] >= 40:
            for dt in ds.DTYPES:
                x = ds.wiener_input(shape, dt, 'band_on_pivot')
                assert abs(pivot(x, 0)) > 990 and abs(x[0, shape[1] // 2]) < 10 and abs(x[WN_RS - 2, shape[1] // 2]) < 10
                y = ds.wiener_input(shape, dt, 'band_off_pivot')
                assert abs(pivot(y, 0)) < 10 and abs(y[off[0], shape[1] // 2]) > 990


def test_inputs_are_what_the_sweep_says():
    for shape in ds.MD_SHAPES + ((65537, 3),):
        for dt in ds.DTYPES:
            x = ds.median_input(shape, dt)
            assert x.dtype == np.dtype(dt) and not np.isnan(x).any()
            fin = x[np.isfinite(x)]
            assert np.array_equal(fin * 2, np.round(fin * 2))
            if x.size >= 100:
                zeros = x[x == 0]
                assert (fin > 0).any() and (fin < 0).any() and np.signbit(zeros).any() and not np.signbit(zeros).all()
                assert (x == np.inf).any() and (x == -np.inf).any()
    for shape in ds.WN_SHAPES:
        if shape not in ds.DEGENERATE:
            x = ds.wiener_input(shape, 'float64', 'nonfinite')
            pos = ds.nonfinite_positions(shape)
            assert int((~np.isfinite(x)).sum()) == len(pos) >= 2
            assert {c for c in (0, WN_TILE - 1, WN_TILE, shape[1] - 1) if c < shape[1]} <= {p[1] for p in pos}
            assert {r for r in (WN_RS - 1, WN_RS) if r < shape[0]} <= {p[0] for p in pos}
            assert np.isnan(x).any() and (x == np.inf).any()
            assert (x == -np.inf).any() or len(pos) == 2
