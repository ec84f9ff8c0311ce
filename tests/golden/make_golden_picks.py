#!/usr/bin/env python3
"""Generate the ``PK*`` golden vectors (layer picking, continuity index) by running the REFERENCE's
``picklib.auto_pick`` / ``pick`` / ``packet_pick`` (``src/impdar/lib/picklib.py:16-199``), ``PickParameters``,
``Picks`` and ``analysis/continuity_index.py`` -- loaded by file path, never copied -- on small synthetic
radargrams (``tests/picking_ref.synthetic``).  Inputs are stored as float32; the float64 cases are the same values
widened.  Every file stores the input, the parameters and either the reference's picks for both dtypes or the text
of the error it raised, with the seed and trace where the NumPy restatement places it.  The script asserts the
outcome kind each case is meant to have, so a fixture cannot silently turn into an all-errors set, and that
``tests/picking_ref.py`` agrees with the reference on every case it writes.  ``PK_ref_saved_picked.mat`` is a
small picked file written by the reference's ``save()``.

Only runs where the reference is installed; the committed files are what travels.

Usage:  python tests/golden/make_golden_picks.py REFERENCE_SRC            (the directory that holds impdar/)
        python tests/golden/make_golden_picks.py REFERENCE_SRC --load FILE   print the picks the reference loads
"""
import contextlib
import importlib
import io
import os
import sys
import types
import warnings

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import picking_ref as ref          # noqa: E402

DT = 1.0e-8
VERS = dict(numpy_version=np.__version__, scipy_version=scipy.__version__)
KINDS = {'picks': 0, 'short': 1, 'argmax': 2, 'argmin': 3}
TEXT = {1: 'Your choice of frequency is too high', 2: 'attempt to get argmax of an empty sequence',
        3: 'attempt to get argmin of an empty sequence'}


def load_reference(src):
    """The reference's lib package under a private name, so that nothing of this project shadows it."""
    pkg = types.ModuleType('ref_impdar_lib')
    pkg.__path__ = [os.path.join(src, 'impdar', 'lib')]
    sys.modules['ref_impdar_lib'] = pkg
    mods = {}
    for name in ('picklib', 'PickParameters', 'Picks', 'NoInitRadarData', 'RadarData', 'analysis.continuity_index'):
        mods[name.split('.')[-1]] = importlib.import_module('ref_impdar_lib.' + name)
    return types.SimpleNamespace(**mods)


def ref_dat(R, data, freq=None, pol=1):
    d = R.NoInitRadarData.NoInitRadarData(big=True)
    d.data = data.copy()
    d.snum, d.tnum = data.shape
    d.dt = DT
    d.travel_time = np.arange(d.snum) * DT * 1.0e6
    n = d.tnum
    d.dist, d.long, d.lat = np.arange(n) * 1., np.arange(n) * 3., np.arange(n) * 2.
    d.trace_num, d.decday = np.arange(n) + 1., np.arange(n).astype(float)
    d.trig, d.pressure, d.elevation = np.zeros(n), np.zeros(n), np.zeros(n)
    d.picks = R.Picks.Picks(d)
    if freq is not None:
        with contextlib.redirect_stdout(io.StringIO()):
            d.picks.pickparams.freq_update(freq)
    d.picks.pickparams.pol = pol
    return d


def save(name, **arrs):
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **arrs, **VERS)
    size = os.path.getsize(path)
    print('wrote', path, size, 'bytes')
    assert size < 512 * 1024, size


def run(fn):
    """``(outcome code, result or None, message or None)`` of a reference call."""
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            return 0, fn(), None
    except ValueError as e:
        msg = str(e)
        for code, text in TEXT.items():
            if text in msg:
                return code, None, msg
        raise


def check_picks(got, want, dtype, what):
    """The restatement against the reference: rows 0-2 equal, row 3 NaN, power within the bar."""
    assert np.array_equal(got[..., :3, :], want[..., :3, :], equal_nan=True), what
    assert np.all(np.isnan(got[..., 3, :])) and np.all(np.isnan(want[..., 3, :])), what
    p, q = got[..., 4, :], want[..., 4, :]
    assert np.array_equal(np.isnan(p), np.isnan(q)), what
    n = want[..., 2, :] - want[..., 0, :] + 1
    ok = np.isnan(q) | (np.abs(p - q) <= ref.power_bar(n, dtype, q))
    assert np.all(ok), (what, float(np.nanmax(np.abs(p - q) / ref.power_bar(n, dtype, q))))


def ref_chains(R, d, snums, tnums):
    """Every seed's chain on its own, trace by trace through the reference's ``packet_pick``, as far as it gets:
    ``(picks, outcome per seed, trace it stopped at or -1)``.  What a failing ``auto_pick`` had picked before it
    raised is not returned by the reference; this recovers it, and the walks of the seeds it never reached."""
    pp = d.picks.pickparams
    out = np.full((len(snums), 5, d.tnum), np.nan)
    codes, traces = np.zeros(len(snums), dtype=np.int64), np.full(len(snums), -1, dtype=np.int64)
    for k, (s, t0) in enumerate(zip(snums, tnums)):
        mid = s
        for j in list(range(t0, -1, -1)) + list(range(t0 + 1, d.tnum)):
            if j == t0 + 1:
                mid = (out[k, 0, t0] + out[k, 2, t0]) // 2
            code, pick, _ = run(lambda: R.picklib.packet_pick(d.data[:, j], pp, mid))
            if code != 0:
                codes[k], traces[k] = code, j
                break
            out[k, :, j] = pick
            mid = (pick[0] + pick[2]) // 2
    return out, codes, traces


def auto_case(R, name, data32, freq, pol, snums, tnums, kind, partial=False, windows=None):
    arrs = dict(kind='auto', expect=kind, data=data32, dt=DT, freq=freq, pol=pol, snums=np.array(snums), tnums=np.array(tnums))
    for dtype, tag in ((np.float32, '32'), (np.float64, '64')):
        d = ref_dat(R, data32.astype(dtype), freq, pol)
        pp = d.picks.pickparams
        if windows is not None:         # window sizes no frequency gives: set as a loaded struct could hold them
            pp.plength, pp.FWW, pp.scst = windows
        else:
            assert (pp.plength, pp.FWW, pp.scst) == ref.freq_params(freq, DT, d.snum)
        prm = (pp.plength, pp.FWW, pp.scst)
        code, out, msg = run(lambda: R.picklib.auto_pick(d, snums, tnums))
        assert code == KINDS[kind], (name, tag, code, msg)
        mine, (mcode, mseed, mtrace) = ref.auto_pick(d.data, snums, tnums, *prm, pol)
        assert mcode == code, (name, mcode, code)
        arrs.update(plength=prm[0], FWW=prm[1], scst=prm[2], code=code)
        if code == 0:
            check_picks(mine, out, dtype, name + tag)
            arrs['out' + tag] = out
        else:
            arrs.update(message=msg, fail_seed=mseed, fail_trace=mtrace)
        if partial:
            part, codes, traces = ref_chains(R, d, snums, tnums)
            for k in range(len(snums)):
                mine, (mcode, _, mtrace) = ref.auto_pick(d.data, snums[k:k + 1], tnums[k:k + 1], *prm, pol)
                assert (mcode, mtrace) == (codes[k], traces[k]), (name, k)
                check_picks(mine[0], part[k], dtype, name + tag)
            reached = int(np.sum(~np.isnan(part[:, 0])))
            print(name + tag, 'the chains pick', reached, 'traces before they leave the data')
            assert reached >= 6 * len(snums), 'the chains reach too few traces'
            arrs['partial' + tag] = part
            arrs.update(seed_codes=codes, seed_traces=traces)
    save(name, **arrs)


def guided_case(R, name, data32, freq, pol, t0, n, snum_start, snum_end):
    arrs = dict(kind='guided', expect='picks', data=data32, dt=DT, freq=freq, pol=pol, t0=t0, n=n, snum_start=snum_start,
                snum_end=snum_end)
    for dtype, tag in ((np.float32, '32'), (np.float64, '64')):
        d = ref_dat(R, data32.astype(dtype), freq, pol)
        pp = d.picks.pickparams
        code, out, msg = run(lambda: R.picklib.pick(d.data[:, t0:t0 + n], snum_start, snum_end, pp))
        assert code == 0, (name, msg)
        mid = R.picklib._midpoint(n, snum_start, snum_end)
        mine, first = ref.pick_guided(d.data, t0, mid, pp.plength, pp.FWW, pp.scst, pol)
        assert first[0] == 0
        check_picks(mine, out, dtype, name + tag)
        arrs.update(plength=pp.plength, FWW=pp.FWW, scst=pp.scst, mid=mid)
        arrs['out' + tag] = out
    save(name, **arrs)


def sweep_trace(rng, n):
    flavour = rng.integers(0, 3)
    if flavour == 0:
        x = rng.standard_normal(n)
    else:
        x = rng.integers(-2, 3, n).astype(np.float64)
        if flavour == 2:
            x[rng.integers(0, n, max(1, n // 16))] = np.nan
    return x.astype(np.float32)


# no walk over pure random integers stays inside 64 rows for 70 traces (none of 22400 tried does): the reference ends
# these cases in its 'short' error, and the fixtures keep what every seed's chain had picked until then
TIE_SEEDS = (list(range(20, 44, 2)), [0, 40, 69, 20, 55, 10, 30, 60, 5, 45, 25, 65])
FREQS = [50, 34, 25, 20, 15, 12, 8, 4, 2, 1]


def sweep_cases(R):
    """2000 single packets, and lines of 63 / 64 / 65 traces that share length and parameters."""
    rng = np.random.default_rng(1)
    N, LMAX = 2000, 80
    traces = np.full((N, LMAX), np.nan, dtype=np.float32)
    lens, freqs, pols, mids = (np.zeros(N, dtype=np.int64) for _ in range(4))
    prms = np.zeros((N, 3), dtype=np.int64)
    codes = {t: np.zeros(N, dtype=np.int64) for t in ('32', '64')}
    outs = {t: np.full((N, 5), np.nan) for t in ('32', '64')}

    def one(x32, freq, pol, mid, dtype):
        x = x32.astype(dtype)
        d = ref_dat(R, x[:, None], freq, pol)
        pp = d.picks.pickparams
        code, out, msg = run(lambda: R.picklib.packet_pick(x, pp, mid))
        mcode, mine = ref.packet_pick(x, mid, pp.plength, pp.FWW, pp.scst, pol)
        assert mcode == code, (mcode, code, msg)
        if code == 0:
            check_picks(np.array(mine, dtype=np.float64)[:, None], np.array(out, dtype=np.float64)[:, None], dtype, 'sweep')
        return code, out, (pp.plength, pp.FWW, pp.scst)

    for k in range(N):
        n = int(rng.integers(3, LMAX + 1))
        x = sweep_trace(rng, n)
        traces[k, :n] = x
        lens[k], freqs[k], pols[k] = n, FREQS[rng.integers(0, len(FREQS))], rng.choice([1, -1])
        mids[k] = rng.integers(-5, n + 5)
        for dtype, tag in ((np.float32, '32'), (np.float64, '64')):
            code, out, prms[k] = one(x, int(freqs[k]), int(pols[k]), int(mids[k]), dtype)
            codes[tag][k] = code
            if code == 0:
                outs[tag][k] = out
    share = [float(np.mean(codes['32'] == c)) for c in range(4)]
    print('sweep outcome shares (picked, short, argmax, argmin):', share)
    assert share[0] >= 0.40 and share[1] > 0.2 and share[2] > 0 and share[3] > 0, share
    assert np.array_equal(codes['32'], codes['64'])
    save('PK20_sweep', kind='sweep', traces=traces, lens=lens, freqs=freqs, pols=pols, mids=mids, prms=prms, dt=DT,
         codes=codes['32'], out32=outs['32'], out64=outs['64'])

    G, NMAX = 30, 65
    data = np.full((G, LMAX, NMAX), np.nan, dtype=np.float32)
    snum, ns, gfreq, gpol = (np.zeros(G, dtype=np.int64) for _ in range(4))
    gprm = np.zeros((G, 3), dtype=np.int64)
    gmid = np.zeros((G, NMAX), dtype=np.int64)
    gcodes = np.zeros((G, NMAX), dtype=np.int64)
    gout = {t: np.full((G, 5, NMAX), np.nan) for t in ('32', '64')}
    for g in range(G):
        ns[g], snum[g] = (63, 64, 65)[g % 3], int(rng.integers(3, LMAX + 1))
        gfreq[g], gpol[g] = FREQS[rng.integers(0, len(FREQS))], rng.choice([1, -1])
        for i in range(ns[g]):
            x = sweep_trace(rng, snum[g])
            data[g, :snum[g], i] = x
            gmid[g, i] = rng.integers(-5, snum[g] + 5)
            for dtype, tag in ((np.float32, '32'), (np.float64, '64')):
                code, out, gprm[g] = one(x, int(gfreq[g]), int(gpol[g]), int(gmid[g, i]), dtype)
                gcodes[g, i] = code
                if code == 0:
                    gout[tag][g, :, i] = out
    assert np.mean(gcodes[:, :63] == 0) > 0.3
    save('PK21_sweep_lines', kind='sweep_lines', data=data, snum=snum, n=ns, freqs=gfreq, pols=gpol, prms=gprm, mids=gmid,
         dt=DT, codes=gcodes, out32=gout['32'], out64=gout['64'])


def continuity_case(R, name, data32, spick, bpick, ratios):
    """The reference's index for float32 and float64 input, and how far its float32 result is from its float64 one
    in units of the bar 16 u max(1, max|P|)."""
    arrs = dict(kind='continuity', data=data32, spick=np.array(np.nan) if spick is None else spick, bpick=bpick, ratios=np.array([np.nan if r is None else r for r in ratios]))
    worst = 0.
    for k, ratio in enumerate(ratios):
        res = {}
        for dtype, tag in ((np.float32, '32'), (np.float64, '64')):
            d = ref_dat(R, data32.astype(dtype))
            d.picks.samp1 = np.vstack((spick, bpick)) if spick is not None else np.vstack((bpick, bpick))
            with warnings.catch_warnings(), np.errstate(all='ignore'):
                warnings.simplefilter('ignore')
                R.continuity_index.continuity_index(d, 1, 0 if spick is not None else None, ratio)
            res[tag] = np.array(d.continuity_index, dtype=np.float64)
            arrs['out%s_%d' % (tag, k)] = res[tag]
        s, b = bounds(np.zeros_like(bpick) if spick is None else spick, bpick, data32.shape[0])
        for dtype, tag in ((np.float32, '32'), (np.float64, '64')):
            mine = ref.continuity(data32.astype(dtype), s, b, ratio)
            assert np.array_equal(np.isnan(mine), np.isnan(res[tag])), (name, ratio, tag)
            bar = 16 * ref.unit_roundoff(dtype) * ref.continuity_pmax(data32.astype(dtype), s, b, ratio)
            if not np.all(np.isnan(mine)):
                assert np.nanmax(np.abs(mine - res[tag])) <= bar, (name, ratio, tag, np.nanmax(np.abs(mine - res[tag])) / bar)
        assert np.array_equal(np.isnan(res['32']), np.isnan(res['64']))
        if not np.all(np.isnan(res['64'])):
            bar32 = 16 * ref.unit_roundoff(np.float32) * ref.continuity_pmax(data32, s, b, ratio)
            worst = max(worst, float(np.nanmax(np.abs(res['32'] - res['64']))) / bar32)
    arrs['ref32_vs_ref64_over_bar'] = worst
    print(name, 'reference float32 against its float64, over the bar: %.3f' % worst)
    save(name, **arrs)
    return worst


def bounds(spick, bpick, snum):
    s = np.full(len(bpick), -1, dtype=np.int32)
    b = np.full(len(bpick), -1, dtype=np.int32)
    for j in range(len(bpick)):
        if not (np.isnan(spick[j]) or np.isnan(bpick[j])):
            s[j], b[j], _ = slice(int(spick[j]), int(bpick[j])).indices(snum)
    return s, b


def saved_file(R):
    """A picked file as the reference writes it: two layers of the basic radargram."""
    data = ref.synthetic(96, 70, [(30, 0.15, 1), (60, -0.2, -0.8)]).astype(np.float32)
    d = ref_dat(R, data, 4, 1)
    out = R.picklib.auto_pick(d, [30, 35], [0, 35])
    for k, num in enumerate((1, 2)):
        d.picks.add_pick(num)
        d.picks.update_pick(num, out[k])
    path = os.path.join(HERE, 'PK_ref_saved_picked.mat')
    d.save(path)
    print('wrote', path, os.path.getsize(path), 'bytes')
    back = R.RadarData.RadarData(path)
    assert np.array_equal(back.picks.samp2, out[:, 1]) and back.picks.picknums == [1, 2]


def load_check(R, path):
    d = R.RadarData.RadarData(path)
    print(d.picks)
    print('picknums', d.picks.picknums, 'samp2 shape', None if d.picks.samp2 is None else d.picks.samp2.shape)
    pp = d.picks.pickparams
    print('freq', pp.freq, 'plength', pp.plength, 'FWW', pp.FWW, 'scst', pp.scst, 'pol', pp.pol)
    if d.picks.samp2 is not None:
        print('samp2[:, :8]', d.picks.samp2[:, :8])


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    R = load_reference(sys.argv[1])
    if len(sys.argv) >= 4 and sys.argv[2] == '--load':
        return load_check(R, sys.argv[3])
    two = [(30, 0.15, 1), (60, -0.2, -0.8)]
    basic = ref.synthetic(96, 70, two).astype(np.float32)
    seeds = ([30, 35, 50, 60, 35], [0, 35, 69, 0, 35])
    auto_case(R, 'PK01_basic_pos', basic, 4, 1, *seeds, 'picks')
    auto_case(R, 'PK02_basic_neg', basic, 4, -1, [50, 60, 50], [69, 0, 69], 'picks')
    d = ref_dat(R, basic, 4, 1)
    out = R.picklib.auto_pick(d, [30, 35], [0, 35])
    assert np.array_equal(out[0, :3], out[1, :3]), 'the seeds (30, 0) and (35, 35) follow the same layer'
    auto_case(R, 'PK03_band_edge', ref.synthetic(96, 130, two).astype(np.float32), 8, 1, [30, 58, 40], [0, 129, 77], 'picks')
    one = ref.synthetic(96, 70, [(30, 0.15, 1)]).astype(np.float32)
    auto_case(R, 'PK04_smallest_f25', one, 25, 1, [30], [10], 'picks')
    auto_case(R, 'PK05_smallest_f34', one, 34, 1, [30], [10], 'argmin')
    auto_case(R, 'PK06_smallest_f50', one, 50, 1, [30], [10], 'argmax')
    auto_case(R, 'PK07_long_window', ref.synthetic(600, 70, [(300, 0.4, 1)], w=40.).astype(np.float32), 0.5, 1, [300], [69], 'picks')
    auto_case(R, 'PK08_direct', ref.synthetic(3000, 24, [(1500, 0.4, 1)], w=200.).astype(np.float32), 0.1, 1, [1500], [12],
              'picks')
    for slope, name in ((3, 'PK09_steep3'), (8, 'PK10_steep8')):
        data = ref.synthetic(800, 70, [(40, slope, 1)], noise=0.01).astype(np.float32)
        auto_case(R, name, data, 4, 1, [40], [0], 'picks')
        d = ref_dat(R, data, 4, 1)
        out = R.picklib.auto_pick(d, [40], [0])
        j = np.arange(70)
        off = np.max(np.abs(out[0, 1] - (40 + slope * j + 2 * np.sin(j / 9.))))
        print(name, 'the reference follows the layer to within %.2f rows' % off)
        assert off <= 1.3, off
    auto_case(R, 'PK11_bottom', ref.synthetic(96, 70, [(70, 0.5, 1)]).astype(np.float32), 4, 1, [70], [0], 'short')
    auto_case(R, 'PK12_top', ref.synthetic(300, 70, [(30, 0.15, 1)]).astype(np.float32), 1, 1, [30], [0], 'short')
    rng = np.random.default_rng(3)
    ties = rng.integers(-2, 3, (64, 70)).astype(np.float32)
    auto_case(R, 'PK13_ties', ties, 8, 1, TIE_SEEDS[0], TIE_SEEDS[1], 'short', partial=True)
    for j in range(70):
        ties[rng.integers(0, 64, 3), j] = np.nan
    auto_case(R, 'PK14_nan', ties, 8, -1, TIE_SEEDS[0], TIE_SEEDS[1], 'short', partial=True)
    # either side of the longest window that csrc/pick.hip walks out of LDS (PK_STAGE_MAX = 190)
    edge = ref.synthetic(420, 40, [(210, 0.4, 1)], w=30.).astype(np.float32)
    auto_case(R, 'PK16_staged_190', edge, 1, 1, [210], [20], 'picks', windows=(190, 63, 63))
    auto_case(R, 'PK17_direct_191', edge, 1, 1, [210], [20], 'picks', windows=(191, 63, 64))
    auto_case(R, 'PK15_one_trace', ref.synthetic(96, 1, [(30, 0.15, 1)]).astype(np.float32), 4, 1, [30], [0], 'picks')

    wide = ref.synthetic(96, 130, two).astype(np.float32)
    guided_case(R, 'PK30_guided_line', basic, 4, 1, 0, 70, 30, 42)
    guided_case(R, 'PK31_guided_flat', basic, 4, 1, 0, 70, -9999, 40)
    guided_case(R, 'PK32_guided_sub', wide, 4, 1, 17, 47, 30, 42)
    guided_case(R, 'PK33_guided_wide', wide, 4, -1, 0, 130, 60, 36)
    sweep_cases(R)

    worst = 0.
    for name, shape in (('PK40_continuity_small', (96, 70)), ('PK41_continuity_wide', (300, 130))):
        snum, tnum = shape
        data = ref.synthetic(snum, tnum, [(30, 0.15, 1), (int(0.6 * snum), -0.2, -0.8)]).astype(np.float32)
        d = ref_dat(R, data, 4, 1)
        lay = R.picklib.auto_pick(d, [30, int(0.6 * snum)], [0, 0])
        spick, bpick = lay[0, 0].copy(), lay[1, 0].copy()
        bpick[3] = np.nan                       # a NaN pick
        spick[5] = np.nan
        data[int(bpick[7]) - 4, 7] = 0.         # a zero sample inside a window: P = -inf
        bpick[9], bpick[10] = spick[9] + 9, spick[10] + 10      # windows of 9 and of 10 rows
        worst = max(worst, continuity_case(R, name + '_s', data, spick, bpick, [None, 0.1, 0.001]))
        bpick[9], bpick[10] = 9, 10
        worst = max(worst, continuity_case(R, name + '_0', data, None, bpick, [None, 0.1, 0.001]))
    print('continuity: the reference float32 result is at most %.3f of the bar from its float64 one' % worst)
    saved_file(R)


if __name__ == '__main__':
    main()
