"""The window search of the attenuation methods 3 and 6b on the MI355X (csrc/attsearch.hip) against ``tests/analysis_ref.py``
and the ``YA_*`` fixtures, through ``impdar_att_search`` and through the public functions.

``C`` is held to the ``longdouble`` evaluation of the same windows: |C_dev - C_hi| <= 8 x max |C_ref - C_hi|, absolute (``C``
lies in [0, 1] and its minimum sits near 0), the right-hand side measured per case from the float64 restatement of the
reference's passes (never from the device); 8 is the margin this project gives a differently ordered float64 sum over the
reference's own rounding.  On the decided fixtures that distance was 5.4e-15 (400 traces) and 1.9e-15 (1000 traces) when
they were written; the device's, on an MI355X, 5.6e-16 and 5.1e-16 (ratios 0.10 and 0.27).

A centre's decision is compared where its margin exceeds twice that tolerance; the centres left out may be at most 1 % of
a case, asserted, so a loose kernel cannot hide behind the exclusion.  On the fixtures the margin is
``analysis_ref.margin``: the smaller of the gap from the minimum ``C`` to its runner-up and of any |C - Cw|, over all
windows a centre visited.  The shape tests start from windows of two to five elements, and two elements have |r| = 1 for
every rate up to rounding, so their gap is nothing in every walk that begins there; these tests take the gap from the last
window alone, the one whose minimum is reported (the minimum of an earlier window enters only through ``Cm < Cw``, which
|C - Cw| covers): that leaves out fewer centres than the fixtures' rule would, never more.  A centre whose last window
has two elements is decided by rounding alone: it is compared only where the restatement's outcome is a value with a
margin, and does not count into the 1 %."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

from conftest import golden

import analysis_ref as ar

pytestmark = pytest.mark.gpu

NS30 = np.arange(30.)
NS30.setflags(write=False)


def margin(w, cw):
    """The margin of the shape tests (above): any |C - Cw|, and the gap to the runner-up in the last window."""
    m = np.inf
    for cs in w['rows']:
        m = min(m, float(np.min(np.abs(cs - cw))))
    if w['rows'] and len(w['rows'][-1]) > 1:
        s = np.sort(w['rows'][-1])
        m = min(m, float(s[1] - s[0]))
    return m


def finite(w):
    return all(np.all(np.isfinite(cs)) for cs in w['rows'])


def rows_ld(w, z, pc, ns):
    return [ar.c_row_ld(z[at], pc[at], ns) for at in w['windows']]


@functools.lru_cache(maxsize=None)
def fixture_walks(name):
    """A decided method 3 fixture: the prepared pick, the call, and the restatement's walk of every trace, computed once."""
    g = golden(name)
    kw = json.loads(str(g['call']))['kwargs']
    z, pc = ar.prepared(g['picks_z'][0], g['picks_corrected_power'][0])
    traces = range(kw['win_init'] // 2, int(g['tnum']) - kw['win_init'] // 2)
    walks = [ar.walk(ar.INDEX, z, pc, g['Ns'], 0.1, 1., kw['win_init'], kw['win_step'], tr) for tr in traces]
    for a in (z, pc):
        a.setflags(write=False)
    return g, kw, z, pc, traces, walks


def held(rows_dev, rows_ref, rows_hi, what):
    """|C_dev - C_hi| <= 8 max |C_ref - C_hi| over the rows; returns (tolerance, ratio of the device's distance to the reference's)."""
    assert len(rows_dev) == len(rows_ref), what
    ref, dev = ar.distance(rows_ref, rows_hi), ar.distance(rows_dev, rows_hi)
    ratio = dev / ref if ref > 0 else (0.0 if dev == 0 else np.inf)
    print('%s: max |C_dev - C_hi| %.3e, max |C_ref - C_hi| %.3e, ratio %.3f' % (what, dev, ref, ratio))
    assert dev <= 8 * ref, (what, dev, ref)
    return 8 * ref, ratio


@pytest.mark.parametrize('name, every', [('YA_m3_400', 4), ('YA_m3_1000', 10)])
def test_decided_fixture_probe_rows_and_decisions(hip, name, every):
    from impdar_amd import attsearch
    g, kw, z, pc, traces, walks = fixture_walks(name)
    ns = g['Ns']
    # the probed centres, one launch of one centre each
    dev_rows, ref_rows, hi_rows = [], [], []
    for b in range(0, len(traces), every):
        idx, win, code, table = attsearch.search_dev(attsearch.INDEX, z, pc, ns, 0.1, 1., kw['win_init'], kw['win_step'], first=traces[b], ncent=1,
                                                     probe=0)
        assert len(table) == len(walks[b]['rows']), (name, traces[b])
        dev_rows += list(table)
        ref_rows += walks[b]['rows']
        hi_rows += rows_ld(walks[b], z, pc, ns)
    tol, _ = held(dev_rows, ref_rows, hi_rows, name)
    # every centre in one launch
    idx, win, code = attsearch.search_dev(attsearch.INDEX, z, pc, ns, 0.1, 1., kw['win_init'], kw['win_step'], first=traces[0], ncent=len(traces))
    left_out = 0
    for b, tr in enumerate(traces):
        if ar.margin(walks[b]['rows'], 0.1) > 2 * tol:
            assert code[b] == attsearch.VALUE and ns[idx[b]] == g['out0'][tr] and win[b] == g['out1'][tr], (name, tr)
        else:
            left_out += 1
    print('%s: %d of %d centres left out by their margin' % (name, left_out, len(traces)))
    assert left_out <= 0.01 * len(traces)


@pytest.mark.parametrize('name', ['YA_m3_400', 'YA_m3_1000', 'YA_m3_nan', 'YA_m3_odd', 'YA_m3_step1', 'YA_m6b_km', 'YA_m6b_m', 'YA_m6b_flat'])
def test_public_functions_on_the_device(hip, name):
    from impdar_amd.lib.analysis import attenuation
    g = golden(name)
    lib, ctx = hip.load(), hip.context()
    got = ar.run_call({'att': attenuation}, g)
    assert 'impdar_att_search' in metrics(hip, lib, ctx)
    for k in ('out0', 'out1', 'after_picks_z', 'after@Ns') + (('after@att_ds',) if 'att_ds' in g else ()):
        assert np.array_equal(got[k], g[k], equal_nan=True), (name, k)


def metrics(hip, lib, ctx):
    buf = C.create_string_buffer(4096)
    hip.check(lib.impdar_ctx_last_metrics(ctx, buf, len(buf)), 'impdar_ctx_last_metrics')
    return buf.value.decode()


# ---- smallest breaking shapes, against the restatement

def rates(nn):
    """``nn`` rates, one of them 0 (the second, where there are two or more)."""
    return np.array([0.]) if nn == 1 else (np.arange(nn, dtype=np.float64) - 1.) * (29. / nn)


def compare_index(hip, z, pc, ns, wi, ws, first, ncent, nh_target=1., probes=(), what=''):
    """One launch over the centres first .. first + ncent - 1 against the restatement's walks; returns (codes, walks)."""
    from impdar_amd import attsearch
    walks = [ar.walk(ar.INDEX, z, pc, ns, 0.1, nh_target, wi, ws, first + b) for b in range(ncent)]
    ref = [r for w in walks for r in w['rows']]
    hi = [r for w in walks for r in rows_ld(w, z, pc, ns)]
    good = [k for k, r in enumerate(ref) if np.all(np.isfinite(r))]
    tol = 8 * ar.distance([ref[k] for k in good], [hi[k] for k in good])
    idx, win, code = attsearch.search_dev(attsearch.INDEX, z, pc, ns, 0.1, nh_target, wi, ws, first=first, ncent=ncent)
    counted = left_out = 0
    for b, w in enumerate(walks):
        tr = first + b
        if not w['rows']:
            assert code[b] == attsearch.NOT_ENTERED and idx[b] == -1 and win[b] == wi, (what, tr)
            continue
        if not finite(w):
            assert code[b] == attsearch.NONFINITE, (what, tr)
            continue
        tiny = len(w['windows'][-1]) <= 2
        counted += not tiny
        if margin(w, 0.1) > 2 * tol:
            assert code[b] == attsearch.VALUE and w['nm'].size == 1 and ns[idx[b]] == w['nm'][0] and win[b] == w['win'], (what, tr)
        else:
            left_out += not tiny
    assert left_out <= 0.01 * counted, (what, left_out, counted)
    for b in probes:
        if finite(walks[b]) and walks[b]['rows']:
            table = attsearch.search_dev(attsearch.INDEX, z, pc, ns, 0.1, nh_target, wi, ws, first=first + b, ncent=1, probe=0)[3]
            assert len(table) == len(walks[b]['rows']), (what, b)
            for r_dev, r_ref, r_hi in zip(table, walks[b]['rows'], rows_ld(walks[b], z, pc, ns)):
                assert float(np.max(np.abs(r_dev.astype(ar.LD) - r_hi))) <= tol, (what, b)
    return code, walks


@pytest.mark.parametrize('nn', [1, 2, 30, 63, 64, 65, 130])
def test_rate_counts(hip, nn):
    z, pc = ar.synthetic(150, 5)
    compare_index(hip, z, pc, rates(nn), 8, 6, 4, 142, probes=(0, 70, 141), what='nn %d' % nn)


def test_window_sizes_across_64_256_1024(hip):
    """Every window is visited (Nh_target -1): 60, 250, ... 2150 elements around the middle traces -- across a wave, the
    workgroup and the LDS tile, the last windows two and three tiles long."""
    z, pc = ar.synthetic(2300, 6)
    code, walks = compare_index(hip, z, pc, NS30, 60, 190, 1148, 5, nh_target=-1., probes=(2,), what='sizes')
    sizes = sorted({len(at) for w in walks for at in w['windows']})
    assert sizes[0] == 60 and sizes[-1] >= 2048 and any(64 < s <= 256 for s in sizes) and any(256 < s <= 1024 for s in sizes)
    assert any(1024 < s <= 2048 for s in sizes)


@pytest.mark.parametrize('ws', [1, 2, 7])
@pytest.mark.parametrize('wi', [2, 3, 4, 5])
def test_small_widths_and_steps(hip, wi, ws):
    """All centres of a 40-trace pick, the first (tr = win_init // 2) and the last included; among them centres that meet
    win // 2 == tr and win // 2 == n - tr exactly on their way."""
    n = 40
    z, pc = ar.synthetic(n, 7 + wi)
    first, ncent = wi // 2, n - 2 * (wi // 2)
    code, walks = compare_index(hip, z, pc, NS30, wi, ws, first, ncent, nh_target=-1., probes=(0, ncent // 2, ncent - 1), what='wi %d ws %d' % (wi, ws))
    halves = [[len(at) // 2 for at in w['windows']] for w in walks]
    assert any(h and h[-1] == first + b for b, h in enumerate(halves)) and any(h and h[-1] == n - (first + b) for b, h in enumerate(halves))
    assert halves[0] and halves[0][0] == first


def test_record_shorter_than_tnum_and_a_single_centre(hip):
    """15 NaN traces dropped: the 14 centres past n - win_init // 2 visit no window (one of them sits at n itself)."""
    from impdar_amd import attsearch
    z, pc = ar.synthetic(85, 8)
    tnum, wi, ws = 100, 10, 4
    code, walks = compare_index(hip, z, pc, NS30, wi, ws, wi // 2, tnum - 2 * (wi // 2), what='short')
    assert list(code[-14:]) == [attsearch.NOT_ENTERED] * 14 and code[-15] != attsearch.NOT_ENTERED
    compare_index(hip, z, pc, NS30, wi, ws, 40, 1, probes=(0,), what='single')


def depth_case():
    z, pc = ar.synthetic(500, 9)
    z[np.argmin(z)], z[np.argmax(z)] = 1.0, 2.0
    z[[10, 20, 30]] = 1.5                                     # equal depths, different powers
    order = np.argsort(z, kind='stable')
    return z, pc, order


@pytest.mark.parametrize('wi, ws', [(0.25, 0.1), (0.0625, 0.1), (0.5, 0.25)])
def test_depth_windows(hip, wi, ws):
    """The first window of the first depth touches min Z (entered; the next is outside), the second depth lies a rounding
    below it (outside); likewise at max Z, where the depth one rounding above is still entered because d + win/2 rounds
    to max Z, and the next one is outside; equal depths in Z; a step that is no binary fraction, so the width is the
    repeated sum."""
    from impdar_amd import attsearch
    z, pc, order = depth_case()
    depths = np.array([1.0 + wi / 2, np.nextafter(1.0 + wi / 2, 0.), 1.3, 1.5, 1.5, 1.7, 2.0 - wi / 2, np.nextafter(2.0 - wi / 2, 3.),
                       2.0 - wi / 2 + np.spacing(2.0)])
    walks = [ar.walk(ar.DEPTH, z, pc, NS30, 0.1, -1., wi, ws, d) for d in depths]
    assert [len(walks[b]['rows']) for b in (0, 1, -3, -2, -1)] == [1, 0, 1, 1, 0]
    ref = [r for w in walks if finite(w) for r in w['rows']]
    hi = [r for w in walks if finite(w) for r in rows_ld(w, z, pc, NS30)]
    tol = 8 * ar.distance(ref, hi)
    idx, win, code = attsearch.search_dev(attsearch.DEPTH, z[order], pc[order], NS30, 0.1, -1., wi, ws, centres=depths)
    for b, w in enumerate(walks):
        if not w['rows']:
            assert code[b] == attsearch.NOT_ENTERED and win[b] == wi, b
            continue
        if not finite(w):
            # an empty window (the narrow one at min Z holds min Z alone, on its edge): the walk stopped there for NumPy
            assert code[b] == attsearch.NONFINITE, b
            continue
        assert margin(w, 0.1) > 2 * tol, 'depth %d is not decided: margin %.3e' % (b, margin(w, 0.1))
        assert code[b] == attsearch.VALUE and NS30[idx[b]] == w['nm'][0], b
        assert win[b] == w['win'], b                          # the repeated float64 sum, bit for bit
    if ws == 0.1:
        assert any(w['win'] != wi + len(w['rows']) * ws for w in walks)
    for b in (0, 3, 5):
        if not finite(walks[b]):
            continue
        table = attsearch.search_dev(attsearch.DEPTH, z[order], pc[order], NS30, 0.1, -1., wi, ws, centres=depths[b:b + 1], probe=0)[3]
        assert len(table) == len(walks[b]['rows'])
        for r_dev, r_hi in zip(table, rows_ld(walks[b], z, pc, NS30)):
            assert float(np.max(np.abs(r_dev.astype(ar.LD) - r_hi))) <= tol, b


def test_two_calls_same_bits(hip):
    from impdar_amd import attsearch
    z, pc = ar.synthetic(700, 10)
    runs = [attsearch.search_dev(attsearch.INDEX, z, pc, NS30, 0.1, -1., 20, 30, first=10, ncent=680, probe=340) for _ in range(2)]
    bare = attsearch.search_dev(attsearch.INDEX, z, pc, NS30, 0.1, -1., 20, 30, first=10, ncent=680)
    assert len(runs[0][3]) > 10
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(bare, runs[0]):
        assert a.tobytes() == b.tobytes()
    zd, pd, order = depth_case()
    depths = np.linspace(1.2, 1.8, 9)
    runs = [attsearch.search_dev(attsearch.DEPTH, zd[order], pd[order], NS30, 0.1, -1., 0.1, 0.1, centres=depths, probe=4) for _ in range(2)]
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()


def test_outcome_codes_become_the_reference_s_exceptions_and_carry(hip):
    from impdar_amd import attsearch
    z, pc = ar.synthetic(85, 8)
    # a tie: a rate listed twice
    dup = np.array([0., 6., 12., 12., 18.])
    out = attsearch.search_dev(attsearch.INDEX, z, pc, dup, 0.1, 1., 10, 4, first=5, ncent=75)
    ties = [ar.walk(ar.INDEX, z, pc, dup, 0.1, 1., 10, 4, tr)['nm'].size > 1 for tr in range(5, 80)]
    assert any(ties) and [c == attsearch.TIE for c in out[2]] == ties
    with pytest.raises(ValueError):
        attsearch.settle(dup, *out)
    # the stale carry and the first centre without a window
    out = attsearch.search_dev(attsearch.INDEX, z, pc, NS30, 0.1, 1., 10, 4, first=5, ncent=90)
    got, widths = attsearch.settle(NS30, *out)
    want = ar.search(ar.INDEX, z, pc, NS30, 0.1, 1., 10, 4, range(5, 95), count=100)
    assert np.array_equal(got, want[0][5:95]) and np.array_equal(widths, want[1][5:95])
    assert np.all(got[-10:] == got[-11]) and np.all(widths[-10:] == 10)
    with pytest.raises(UnboundLocalError):
        attsearch.settle(NS30, *attsearch.search_dev(attsearch.INDEX, z, pc, NS30, 0.1, 1., 10, 4, first=81, ncent=9))
    # a window of constant depth: non-finite C, the centre is handed to NumPy, which raises as the reference does
    flat = np.full(85, 1.5)
    out = attsearch.search_dev(attsearch.INDEX, flat, pc, NS30, 0.1, 1., 10, 4, first=5, ncent=75)
    assert np.all(out[2] == attsearch.NONFINITE)
    with pytest.raises(ValueError):
        attsearch.settle(NS30, *attsearch.search(attsearch.INDEX, flat, pc, NS30, 0.1, 1., 10, 4, range(5, 80)))
    # the flat-layer fixture of method 6b meets such windows on its way and still ends on values
    g = golden('YA_m6b_flat')
    zf, pf = ar.prepared(g['picks_z'].flatten(), g['picks_corrected_power'].flatten())
    order = np.argsort(zf, kind='stable')
    out = attsearch.search_dev(attsearch.DEPTH, zf[order], pf[order], NS30, 0.1, 1., 0.1, 0.1, centres=g['att_ds'])
    assert np.any(out[2] == attsearch.NONFINITE)


def test_rejected_descriptor_launches_nothing(hip):
    from impdar_amd import attsearch
    z, pc = ar.synthetic(85, 8)
    attsearch.search_dev(attsearch.INDEX, z, pc, NS30, 0.1, 1., 10, 4, first=5, ncent=75)
    lib, ctx = hip.load(), hip.context()

    def kernel_ms():
        ms = C.c_float()
        hip.check(lib.impdar_ctx_last_kernel_ms(ctx, C.byref(ms)), 'impdar_ctx_last_kernel_ms')
        return ms.value

    before = kernel_ms()
    base = dict(flavour=attsearch.INDEX, z=z, pc=pc, ns=NS30, wi=10, ws=4, first=5, ncent=75, centres=None, probe=None)
    zs = np.sort(z)
    bad = [dict(z=z[:0], pc=pc[:0]), dict(ncent=0), dict(ncent=-3), dict(wi=1), dict(ws=0), dict(wi=2.5), dict(first=-1), dict(probe=75),
           dict(ns=np.arange(1., 9.)), dict(ns=np.zeros(0)), dict(ns=np.array([0., 0., 5.])), dict(flavour=7),
           dict(flavour=attsearch.DEPTH, centres=np.array([1.5]), wi=0.1, ws=0.1),                     # z is not sorted
           dict(flavour=attsearch.DEPTH, z=zs, centres=np.array([1.5]), wi=0.0, ws=0.1),
           dict(flavour=attsearch.DEPTH, z=zs, centres=np.array([1.5]), wi=0.1, ws=float('nan')),
           dict(flavour=attsearch.DEPTH, z=zs, centres=np.zeros(0), wi=0.1, ws=0.1),
           # depth walks that could not end: a step the width absorbs, too many steps across the picks, an infinite depth
           dict(flavour=attsearch.DEPTH, z=zs, centres=np.array([1.5]), wi=0.2, ws=1e-17),
           dict(flavour=attsearch.DEPTH, z=zs, centres=np.array([1.5]), wi=0.2, ws=1e-9),
           dict(flavour=attsearch.DEPTH, z=np.append(zs[:-1], np.inf), centres=np.array([1.5]), wi=0.2, ws=0.1),
           dict(flavour=attsearch.DEPTH, z=zs, centres=np.array([1.5]), wi=0.2, ws=1e-5, probe=0)]      # a probe table of more than 2^16 rows
    for change in bad:
        k = dict(base, **change)
        with pytest.raises(ValueError):
            attsearch.search_dev(k['flavour'], k['z'], k['pc'], k['ns'], 0.1, 1., k['wi'], k['ws'], centres=k['centres'], first=k['first'],
                                 ncent=k['ncent'], probe=k['probe'])
        assert kernel_ms() == before, change
    nbytes = C.c_longlong()
    assert lib.impdar_att_search_plan(0, 85, 30, 75, 10., 4., -1, 0, C.byref(nbytes)) == 0 and nbytes.value >= 8 * (2 * 85 + 30 + 77 * 30)
    assert lib.impdar_att_search_plan(0, 85, 0, 75, 10., 4., -1, 0, C.byref(nbytes)) == hip.ERR_ARG
    assert lib.impdar_att_search_plan(0, 1 << 62, 30, 75, 10., 4., -1, 0, C.byref(nbytes)) == hip.ERR_ARG
