"""Cases, seeded inputs, references and the sweeps of the denoise kernels at their smallest breaking shapes
(``test_denoise_sweep_cpu.py`` runs them on a NumPy restatement of the kernels, ``test_denoise_sweep_gpu.py`` on the
device).  Every sweep is a function that takes the implementation under test.

Wiener reference: ``numpy.longdouble``; every window sum is formed from its own terms (over the window's rows, then over
its columns, each window clipped to the image: zero padding adds nothing and the divisor stays N = m n).  No running
sums, no prefix differences, no pivot.  float32 squares are rounded to float32 first; output i covers
i - w/2 .. i + (w-1)/2; an output whose window holds a non-finite value is NaN (the header of ``csrc/denoise.hip``).

Median reference: ``median_closed`` of ``test_denoise_cpu.py`` (explicit reflected gather, ``np.sort``, rank N // 2).

The bars are the project's own (``test_denoise_gpu.py`` holds the 4096 x 10000 runs to them):
  output   NaN where the reference has NaN; elsewhere |got - want| <= 1e-10 max|x| over the finite x, ``want`` the
           long-double form evaluated at the noise the call returned
  noise    |noise_used - noise_ld| <= 1e-9 |noise_ld| where the noise is estimated
  median   equal to the reference (``np.array_equal``: -0.0 == +0.0), dtype kept
"""
import collections
import functools

import numpy as np
import pytest

from test_denoise_cpu import median_closed

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, 'numpy.longdouble is no wider than float64 here: the sweep has no reference'

# The seams of impdar_amd/csrc/denoise.hip (its #defines of the same names; the launch shapes are md_launch's).
WN_BLOCK = 256                  # threads of a workgroup of the Wiener kernels
WN_RS = 64                      # rows per strip of wn_vsum_kernel, one pivot per strip
WN_PER = 4                      # consecutive columns per thread in a tile of wn_hsum_kernel
WN_TILE = WN_BLOCK * WN_PER     # columns per tile of wn_hsum_kernel
WN_MAX_ROW_BLOCKS = 2048        # resident workgroups of wn_hsum_kernel: more rows are looped over
MD_TR, MD_TW = 16, 64           # output tile of med_small_kernel
MD_NB = (16, 32, 64)            # its three register widths; N > 64 goes to med_radix_kernel
MD_SMALL = MD_NB[-1]
MD_LDS = (MD_TR + MD_SMALL - 1) * MD_TW
MD_RADIX_BLOCK = 256            # columns per workgroup of med_radix_kernel
MD_RADIX_ROWS = 65535           # its grid's rows: more rows are looped over
HOR_WIN_MAX = (1 << 30) - 1     # the widest window the argument check admits together with m = 2

OUT_BAR = 1e-10
NOISE_BAR = 1e-9
NOISE_MESSAGE = 'Could not compute variance, specify noise for denoise'
GIVEN_NOISE = 0.05

SHAPE_NAMES = collections.OrderedDict((
    ((1, 1), 'one_sample'), ((1, 7), 'one_row'), ((7, 1), 'one_column'), ((2, 3), 'two_rows'),
    ((63, 255), 'wave_and_block_less_one'), ((64, 256), 'one_strip_one_block'), ((65, 257), 'strip_and_block_plus_one'),
    ((3, 1023), 'tile_less_one'), ((3, 1024), 'one_tile'), ((3, 1025), 'tile_plus_one'),
    ((129, 1023), 'three_strips_ragged'), ((66, 2049), 'three_tiles_ragged'),
    ((2050, 5), 'rows_past_resident_workgroups'), ((65537, 3), 'rows_past_radix_grid')))
DEGENERATE = ((1, 1), (1, 7), (7, 1), (2, 3))
FULL_SHAPES = ((65, 257), (3, 1025), (66, 2049))          # every window occurs with these
WN_SHAPES = tuple(s for s in SHAPE_NAMES if s != (65537, 3))
MD_SHAPES = tuple(s for s in SHAPE_NAMES if s not in ((2050, 5), (65537, 3)))

WN_WINDOW_NAMES = collections.OrderedDict((
    ((1, 2), 'two_columns'), ((2, 1), 'two_rows_no_row_sum'), ((1, 10), 'chain_default'), ((3, 5), 'odd_odd'),
    ((4, 6), 'even_even'), ((64, 3), 'strip_height'), ((65, 3), 'strip_height_plus_one'),
    ((200, 3), 'taller_than_the_image'), ((3, 1023), 'tile_less_one'), ((3, 1024), 'one_tile'),
    ((3, 1025), 'tile_plus_one'), ((3, 2049), 'wider_than_two_tiles'), ((2, 4100), 'wider_than_every_image')))
EVERY_SHAPE_WINDOWS = ((1, 10), (4, 6), (65, 3))          # every shape occurs with these
UNIT_WINDOW = (1, 1)

MD_WINDOWS = collections.OrderedDict((
    (16, ((4, 4), (16, 1), (1, 16))), (17, ((1, 17), (17, 1))), (32, ((4, 8),)), (33, ((3, 11),)),
    (64, ((8, 8), (64, 1), (1, 64))), (65, ((5, 13), (65, 1), (1, 65)))))
MD_BOUNDARY_WINDOWS = tuple(w for ws in MD_WINDOWS.values() for w in ws)
MD_EVERY_SHAPE_WINDOWS = ((4, 4), (1, 17), (4, 8), (3, 11), (8, 8), (5, 13))

WnCase = collections.namedtuple('WnCase', 'shape win dtype variant given')
MdCase = collections.namedtuple('MdCase', 'shape win dtype')
DTYPES = ('float64', 'float32')


# ------------------------------------------------------------------------------------------------ the cases
def _unique(cases):
    return tuple(collections.OrderedDict((c, None) for c in cases))


def wiener_groups():
    """The Wiener sweep as ``{test id: cases}``; the id names the seam of the window and of the shape.  The (1, 1)
    window and the widest window have tests of their own."""
    groups = collections.OrderedDict()

    def add(kind, shape, win, variant, given=None):
        key = '%s-win_%s_%dx%d-on_%s_%dx%d' % ((kind, WN_WINDOW_NAMES[win]) + win + (SHAPE_NAMES[shape],) + shape)
        groups.setdefault(key, [])
        groups[key] += [WnCase(shape, win, dt, variant, given) for dt in DTYPES]

    for shape in FULL_SHAPES:
        for win in WN_WINDOW_NAMES:
            add('base', shape, win, 'base')
    for shape in WN_SHAPES:
        for win in EVERY_SHAPE_WINDOWS:
            add('base', shape, win, 'base')
    for shape in ((3, 1023), (3, 1024)):                          # the window of a tile on the image of a tile
        for win in ((3, 1023), (3, 1024), (3, 1025)):
            add('base', shape, win, 'base')
    for shape in WN_SHAPES:
        if shape[0] >= 40:
            wins = EVERY_SHAPE_WINDOWS + (((64, 3), (3, 1025), (2, 4100)) if shape == (65, 257) else ())
            for win in wins:
                add('band', shape, win, 'band_on_pivot')
                add('band', shape, win, 'band_off_pivot')
    for shape in WN_SHAPES:
        if shape not in DEGENERATE:
            wins = ((1, 10), (4, 6), (65, 3)) + (((3, 1023), (3, 1025)) if shape in FULL_SHAPES else ())
            for win in wins:
                add('nonfinite', shape, win, 'nonfinite', GIVEN_NOISE)
    return collections.OrderedDict((k, _unique(v)) for k, v in groups.items())


def median_groups():
    """The median sweep as ``{test id: cases}``."""
    groups = collections.OrderedDict()

    def add(kind, shape, win, dtypes=DTYPES):
        key = '%s-N_%d_win_%dx%d-on_%s_%dx%d' % ((kind, win[0] * win[1]) + win + (SHAPE_NAMES[shape],) + shape)
        groups.setdefault(key, [])
        groups[key] += [MdCase(shape, win, dt) for dt in dtypes]

    for shape in FULL_SHAPES:
        for win in MD_BOUNDARY_WINDOWS:
            add('dispatch', shape, win)
    for shape in MD_SHAPES:
        for win in MD_EVERY_SHAPE_WINDOWS:
            add('dispatch', shape, win)
    for shape in ((63, 255), (64, 256), (129, 1023)):
        for win in ((64, 1), (1, 64)):
            add('halo', shape, win)
    for shape in DEGENERATE:
        add('periods', shape, (30, 21))
    for shape in ((2, 3), (7, 1)):
        for win in ((1, 65), (65, 1)):
            add('periods', shape, win)
    add('periods', (3, 1025), (2, 4100))
    add('row_loop', (65537, 3), (5, 13), ('float32',))
    return collections.OrderedDict((k, _unique(v)) for k, v in groups.items())


def all_cases(groups):
    return _unique(c for cases in groups.values() for c in cases)


# ------------------------------------------------------------------------------------------------ inputs
def _seed(shape):
    return 7919 * shape[0] + shape[1]


BAND_ON_PIVOT = (28, 36)        # rows, inclusive: holds the pivot row of strip 0 (WN_RS / 2)
BAND_OFF_PIVOT = (4, 12)        # the pivot row of strip 0 is outside


def nonfinite_positions(shape):
    """(row, column, value): NaN, +inf, -inf at columns 0, 1023, 1024 and tnum - 1 and in rows 63 and 64, wherever
    the shape has them, spread so that most windows stay finite."""
    snum, tnum = shape
    values = (np.nan, np.inf, -np.inf)
    cols = sorted({c for c in (0, WN_TILE - 1, WN_TILE, tnum - 1) if c < tnum})
    pos = [((11 * k + 1) % snum, c) for k, c in enumerate(cols)]
    pos += [(r, (tnum // 3 + 5 * r) % tnum) for r in (WN_RS - 1, WN_RS) if r < snum]
    if snum > WN_RS and tnum > WN_TILE:
        pos += [(WN_RS - 1, WN_TILE), (WN_RS, WN_TILE - 1)]
    pos = sorted(set(pos))
    return [(r, c, values[k % 3]) for k, (r, c) in enumerate(pos)]


@functools.lru_cache(maxsize=None)
def wiener_input(shape, dtype, variant):
    """Seeded normal data times the per-row amplitude ``10**(-2 i / snum)``; see the variants above."""
    snum, tnum = shape
    rng = np.random.default_rng(_seed(shape))
    x = rng.standard_normal(shape) * (10. ** (-2. * np.arange(snum) / snum))[:, None]
    if variant in ('band_on_pivot', 'band_off_pivot'):
        assert snum >= 40
        r0, r1 = BAND_ON_PIVOT if variant == 'band_on_pivot' else BAND_OFF_PIVOT
        x[r0:r1 + 1] += 1000.0
    elif variant == 'nonfinite':
        for r, c, v in nonfinite_positions(shape):
            x[r, c] = v
    else:
        assert variant == 'base'
    x = np.ascontiguousarray(x.astype(dtype))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def median_input(shape, dtype):
    """Twice the base data in steps of 0.5, so that ties decide ranks: both signs, both zeros (the weak rows are all
    zeros), a few +-inf, no NaN."""
    snum, tnum = shape
    rng = np.random.default_rng(_seed(shape))
    x = rng.standard_normal(shape) * (10. ** (-2. * np.arange(snum) / snum))[:, None]
    x = np.round(4. * x) / 2.
    k = max(snum * tnum // 97, 1 if snum * tnum > 4 else 0)
    where = rng.choice(snum * tnum, size=k, replace=False)
    x.reshape(-1)[where] = np.where(np.arange(k) % 2 == 0, np.inf, -np.inf)
    x = np.ascontiguousarray(x.astype(dtype))
    x.setflags(write=False)
    return x


# ------------------------------------------------------------------------------------------------ references
def _window_sums(a, w, axis):
    """Output i = the sum of a[i - w // 2 .. i + (w - 1) // 2] along ``axis``, clipped to the array: one ``sum`` per
    output over that window's own terms."""
    a = np.ascontiguousarray(np.moveaxis(a, axis, -1))
    L = a.shape[-1]
    out = np.empty_like(a)
    for i in range(L):
        out[..., i] = a[..., max(i - w // 2, 0):min(i + (w - 1) // 2, L - 1) + 1].sum(axis=-1)
    return np.moveaxis(out, -1, axis)


def _box_ld(a, m, n):
    return _window_sums(_window_sums(a, m, 0), n, 1)


WienerStats = collections.namedtuple('WienerStats', 'mean var bad noise')


@functools.lru_cache(maxsize=None)
def wiener_stats(shape, win, dtype, variant):
    """lMean and lVar (long double), the outputs whose window holds a non-finite value, and noise = mean(lVar)."""
    m, n = win
    x = wiener_input(shape, dtype, variant)
    finite = np.isfinite(x)
    xz = np.where(finite, x, x.dtype.type(0))
    sq = (xz * xz).astype(LD) if x.dtype == np.float32 else xz.astype(LD) * xz.astype(LD)
    N = LD(m) * LD(n)
    bad = _box_ld((~finite).astype(np.int64), m, n) > 0
    mean = _box_ld(xz.astype(LD), m, n) / N
    var = _box_ld(sq, m, n) / N - mean * mean
    mean[bad] = np.nan
    var[bad] = np.nan
    noise = var.sum() / LD(var.size)
    for a in (mean, var, bad):
        a.setflags(write=False)
    return WienerStats(mean, var, bad, noise)


def wiener_out(case, noise):
    """The long-double output for a given noise, rounded to float64."""
    st = wiener_stats(case.shape, case.win, case.dtype, case.variant)
    x = wiener_input(case.shape, case.dtype, case.variant).astype(LD)
    noise = LD(noise)
    with np.errstate(divide='ignore', invalid='ignore'):
        out = np.where(st.var < noise, st.mean, (x - st.mean) * (1 - noise / st.var) + st.mean)
    return out.astype(np.float64)


@functools.lru_cache(maxsize=None)
def median_want(shape, win, dtype):
    want = median_closed(median_input(shape, dtype), *win)
    want = np.ascontiguousarray(want)
    want.setflags(write=False)
    return want


# ------------------------------------------------------------------------------------------------ the sweeps
def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_wiener(fn, case):
    """One case of ``fn(data, m, n, noise) -> (out, noise_used)``.  Returns ``(|diff| / bar, noise error / bar)`` (the
    second is 0 where the noise is given); where the reference's noise is exactly 0, the reference's error is due."""
    x = wiener_input(case.shape, case.dtype, case.variant)
    st = wiener_stats(case.shape, case.win, case.dtype, case.variant)
    if case.given is None and st.noise == 0:
        with pytest.raises(ValueError, match='^%s$' % NOISE_MESSAGE):
            fn(x, case.win[0], case.win[1], None)
        return 0.0, 0.0
    got, used = fn(x, case.win[0], case.win[1], case.given)
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == case.shape, case
    nratio = 0.0
    if case.given is None:
        assert np.isfinite(st.noise), case
        nratio = float(abs(LD(used) - st.noise) / (NOISE_BAR * abs(st.noise)))
        assert nratio <= 1.0, '%s: noise %r, long double %r: %.3f of the bar' % (case, used, st.noise, nratio)
    else:
        assert used == case.given, case
    want = wiener_out(case, used)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=str(case))
    if case.variant == 'nonfinite':
        np.testing.assert_array_equal(np.isnan(want), st.bad, err_msg=str(case))
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0, nratio
    norm = float(np.max(np.abs(x[np.isfinite(x)].astype(np.float64))))
    ratio = float(np.max(np.abs(got[ok] - want[ok]))) / (OUT_BAR * norm)
    assert ratio <= 1.0, '%s: |diff| = %.3f of the bar' % (case, ratio)
    return ratio, nratio


def sweep_wiener(fn, cases):
    """The worst ``(|diff| / bar, noise error / bar)`` over ``cases``."""
    worst = (0.0, 0.0)
    for case in cases:
        r = check_wiener(fn, case)
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    return worst


def check_wiener_unit_window(fn, shape):
    """The (1, 1) window: lVar is x**2 - x**2.  float64: exactly 0 everywhere, so the reference's error.  float32:
    fl32(x * x) - x * x, which the long-double form decides like every other case."""
    x = wiener_input(shape, 'float64', 'base')
    assert wiener_stats(shape, UNIT_WINDOW, 'float64', 'base').noise == 0
    with pytest.raises(ValueError, match='^%s$' % NOISE_MESSAGE):
        fn(x, 1, 1, None)
    return check_wiener(fn, WnCase(shape, UNIT_WINDOW, 'float32', 'base', None))


def check_median(fn, case):
    """One case of ``fn(data, m, n) -> out``."""
    x = median_input(case.shape, case.dtype)
    got = np.asarray(fn(x, *case.win))
    want = median_want(*case)
    assert got.dtype == x.dtype and got.shape == case.shape, case
    assert not np.isnan(want).any()
    assert np.array_equal(got, want), '%s: %d of %d outputs differ, first at %s' % (
        case, int((got != want).sum()), want.size, tuple(np.argwhere(got != want)[0]))


def sweep_median(fn, cases):
    for case in cases:
        check_median(fn, case)
    return len(cases)


# ------------------------------------------------------------------------------------------------ the seams
def seams(wn_cases, md_cases, unit_shapes, widest):
    """Which seam of the kernels each part of the sweep crosses, from the kernels' constants: ``{seam: cases}``.
    ``unit_shapes`` are the shapes of the (1, 1) test, ``widest`` the (shape, window) of the widest-window test."""
    wn = lambda f: [c for c in wn_cases if f(c.shape[0], c.shape[1], c.win[0], c.win[1], c)]
    md = lambda f: [c for c in md_cases if f(c.shape[0], c.shape[1], c.win[0], c.win[1], c)]
    out = collections.OrderedDict()
    out['window wider than a tile on an image wider than a tile'] = wn(lambda s, t, m, n, c: n > WN_TILE < t)
    out['window of exactly a tile on an image of exactly a tile'] = wn(lambda s, t, m, n, c: n == WN_TILE == t)
    out['window taller than a strip on an image of several strips'] = wn(lambda s, t, m, n, c: m > WN_RS and s > WN_RS)
    out['window of exactly a strip'] = wn(lambda s, t, m, n, c: m == WN_RS and s >= WN_RS)
    out['window taller than the image'] = wn(lambda s, t, m, n, c: m // 2 >= s)
    out['window wider than every image'] = wn(lambda s, t, m, n, c: (n - 1) // 2 >= max(x[1] for x in WN_SHAPES))
    out['even windows both ways'] = wn(lambda s, t, m, n, c: m % 2 == 0 and n % 2 == 0)
    out['no horizontal sum (n = 1)'] = wn(lambda s, t, m, n, c: n == 1 and m > 1)
    out['more than two tiles, the last ragged'] = wn(lambda s, t, m, n, c: t > 2 * WN_TILE and t % WN_TILE)
    out['more than two strips, the last ragged'] = wn(lambda s, t, m, n, c: s > 2 * WN_RS and s % WN_RS)
    out['a last row strip of one row'] = wn(lambda s, t, m, n, c: s % WN_RS == 1 and s > WN_RS)
    out['a last tile of one column'] = wn(lambda s, t, m, n, c: t % WN_TILE == 1 and t > WN_TILE)
    out['a last column block of one column (wn_vsum)'] = wn(lambda s, t, m, n, c: t % WN_BLOCK == 1 and t > WN_BLOCK)
    out['more rows than resident workgroups'] = wn(lambda s, t, m, n, c: s > WN_MAX_ROW_BLOCKS)
    out['pivot row inside the flat band'] = wn(
        lambda s, t, m, n, c: c.variant == 'band_on_pivot' and BAND_ON_PIVOT[0] <= min(WN_RS // 2, s - 1) <= BAND_ON_PIVOT[1])
    out['pivot row outside the flat band of its strip'] = wn(
        lambda s, t, m, n, c: c.variant == 'band_off_pivot' and not BAND_OFF_PIVOT[0] <= min(WN_RS // 2, s - 1) <= BAND_OFF_PIVOT[1]
        and BAND_OFF_PIVOT[1] < WN_RS)
    out['non-finite values on both sides of a tile seam'] = wn(
        lambda s, t, m, n, c: c.variant == 'nonfinite' and t > WN_TILE and 1 < n < WN_TILE
        and {WN_TILE - 1, WN_TILE} <= {p[1] for p in nonfinite_positions(c.shape)})
    out['non-finite values on both sides of a strip seam'] = wn(
        lambda s, t, m, n, c: c.variant == 'nonfinite' and s > WN_RS and 1 < m
        and {WN_RS - 1, WN_RS} <= {p[0] for p in nonfinite_positions(c.shape)})
    out['(1, 1) window on every shape'] = [s for s in unit_shapes] if set(unit_shapes) == set(WN_SHAPES) else []
    out['the widest window the argument check admits'] = [widest] if widest[1] == (2, HOR_WIN_MAX) else []
    for nb in MD_NB:
        out['median N = %d, the last of its kernel' % nb] = md(lambda s, t, m, n, c: m * n == nb and s * t > 1)
        out['median N = %d, the first of the next kernel' % (nb + 1)] = md(lambda s, t, m, n, c: m * n == nb + 1 and s * t > 1)
    out['median halo tile m = %d, n = 1' % MD_SMALL] = md(lambda s, t, m, n, c: (m, n) == (MD_SMALL, 1) and s > MD_TR)
    out['median halo tile m = 1, n = %d' % MD_SMALL] = md(lambda s, t, m, n, c: (m, n) == (1, MD_SMALL) and t > MD_TW)
    out['median tiles ragged both ways, more than one'] = md(
        lambda s, t, m, n, c: m * n <= MD_SMALL and s > MD_TR and t > MD_TW and s % MD_TR and t % MD_TW)
    out['float64 radix path beyond its first column block'] = md(
        lambda s, t, m, n, c: m * n > MD_SMALL and c.dtype == 'float64' and t > MD_RADIX_BLOCK)
    out['float32 radix path beyond its first column block'] = md(
        lambda s, t, m, n, c: m * n > MD_SMALL and c.dtype == 'float32' and t > MD_RADIX_BLOCK)
    out['reflection across more than one period, rows'] = md(lambda s, t, m, n, c: m // 2 > 2 * s)
    out['reflection across more than one period, columns'] = md(lambda s, t, m, n, c: n // 2 > 2 * t)
    out['row loop of the radix kernel'] = md(lambda s, t, m, n, c: m * n > MD_SMALL and s > MD_RADIX_ROWS)
    return out
