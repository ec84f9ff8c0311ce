"""The host-side route of the Kirchhoff plan (csrc/kirch_route.h, compiled here by itself with g++: no GPU, no HIP): the
analysis of the axes, the choice between the six kernels with their tile widths, ring sizes and table shifts, and the host
tables the plan uploads.

Where the expected values come from.  model() and the table formulas below are NumPy restatements of the rules of
impdar_kirch_plan_create as it stood at the commit before the route was split out of it (source (a)), written from that
function's text; the header is held to them on every case of tests/kirch_route_cases.py.  In addition
tests/kirch_route_recorded.json holds (source (b)) what that commit's library reported on the GPU for the cases marked gpu
-- impdar_kirch_plan_kernel, _mode, _tnum_pad and _xnoise of a plan created through the C ABI -- and tile maps dumped from
that commit's build_tilemap, compiled into a scratch program with its loop as it stood."""
import json
import math

import numpy as np
import pytest

import kirch_route_cases as KC
from kirch_route_cases import AUTO, EXACT, FAST

KQ_GS, TH, KF_W = 1056, 256, 512


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return KC.probe(str(tmp_path_factory.mktemp('kirchroute')))


def rows(sa, xb, nh, S):
    return (TH + math.ceil(sa * (xb * nh + S - 2)) + 8 + 31) // 32 * 32


def kq_piece(xb, lk=0):
    return (((xb + 15 + 7) // 8 + lk) * KQ_GS + 255) // 256 * 256


def kd_piece(xb):
    return (((xb + 7 + 3) // 4) * KQ_GS + 255) // 256 * 256


def geometry(c):
    dist, tt = KC.axes(c)
    snum, tnum = c['snum'], c['tnum']
    g = dict(tmax=tt.max() if c['tmax'] is None else c['tmax'], increasing=bool(np.all(np.diff(tt) > 0)))
    dt = (tt[-1] - tt[0]) / (snum - 1)
    dev_t = np.abs(tt - (tt[0] + np.arange(snum) * dt))
    g['uni_t'], g['uni_t11'] = bool(dt > 0 and np.all(dev_t <= 1e-9 * dt)), bool(dt > 0 and np.all(dev_t <= 1e-11 * dt))
    dx = (dist[-1] - dist[0]) / (tnum - 1) if tnum >= 2 else 1.0
    dev_x = np.abs(dist - (dist[0] + np.arange(tnum) * dx))
    g['uni_x'] = bool(dx > 0 and np.all(dev_x <= 1e-9 * dx))
    g['dist_sorted'] = bool(np.all(np.diff(dist) >= 0))
    g['xnoise'] = max(4.5e-16 * tnum, (2.0 * dev_x.max() + 4.5e-16 * np.abs(dist).max()) / (dx if dx > 0 else 1.0))
    g.update(dt=dt, dx=dx, sa=2.0 * dx / (KC.VEL * dt))
    g['alpha'] = g['sa'] * g['sa']
    g['hest'] = min(abs(g['tmax'] / dt) / g['sa'] + 2.0, tnum + 128.0)
    ext = max(dist[min(j + 31, tnum - 1)] - dist[j] for j in range(tnum))
    g['gen_need'] = 264.0 + math.ceil(ext * 2.0 / (KC.VEL * dt))
    return g


def model(c, g):
    """impdar_kirch_plan_create's choice of kernel up to its first HIP call, restated."""
    env = {k[len('IMPDAR_KIRCH_'):]: v for k, v in c['env'].items()}
    f32, snum, tnum, nranks, near, sa = c['dtype'] == 'float32', c['snum'], c['tnum'], c['nranks'], c['nearfield'], g['sa']
    uniform = g['uni_t'] and g['uni_x']
    r = dict(tnum_pad=(tnum + 8 * nranks - 1) // (8 * nranks) * 8 * nranks)

    def ring(xb, nh, lk=0):
        return rows(sa, xb, nh, 8) // 32 * kq_piece(xb, lk)
    xbq = 24
    if env.get('XB') in ('24', '32', '40'):
        xbq = int(env['XB'])
    elif ring(40, 1) <= 80 * 1024:
        xbq = 40
    pair32 = 'XB' not in env and 'NH' not in env and not near and xbq == 40 and tnum >= 8000 * nranks and 65535 < ring(32, 2) <= 80 * 1024
    if pair32:
        xbq = 32
    want = int(env['NH']) if 'NH' in env else (2 if pair32 else 1)
    nhq = want if (want in (2, 3) and (xbq == 40 or (xbq == 32 and want == 2)) and not near and ('NH' in env or pair32)
                   and 65535 < ring(xbq, want) <= 160 * 1024) else 1
    wq = rows(sa, xbq, nhq, 8)
    lkq = int(int(env.get('LK', 0)) == 1 and nhq >= 2 and wq // 32 >= 4 * nhq and ring(xbq, nhq, 1) <= 160 * 1024)
    quad_ok = ring(xbq, nhq, lkq) <= (160 if nhq > 1 else 80) * 1024
    tab_ok = TH + sa * 15 + 8.0 <= KF_W
    aperture_ok = snum < 65536 and abs(g['tmax'] / g['dt']) / sa < 65000.0
    fast_ok = f32 and uniform and (quad_ok or tab_ok) and aperture_ok and (2.0 * g['hest'] + 400.0) / 8.0 * snum * 32.0 < 2 ** 31
    gen_ok = (f32 and g['uni_t11'] and g['dist_sorted'] and tnum >= 2 and 4 <= snum < (1 << 22) and c['tmax'] is None and
              tnum * snum * 4.0 < 2 ** 31 and g['gen_need'] <= 1024.0)
    gen_w = max((int(g['gen_need']) + 255) // 256 * 256, 512) if gen_ok else 0
    mode = c['mode']
    gen = gen_ok and mode != EXACT and (env.get('IMPL') == 'gen' or not fast_ok)
    if mode == AUTO:
        mode = FAST if (fast_ok or gen) else EXACT
    if mode == FAST and not fast_ok and not gen:
        return dict(status=KC.UNSUPPORTED, err_sa=sa, err_limit=(KF_W - TH - 8.0) / 15.0)
    parts = int(env['PARTS']) if 'PARTS' in env else (4 if nranks >= 8 else 2 if nranks >= 4 else 1)
    quad = mode == FAST and not gen and quad_ok and not (env.get('IMPL') == 'tab' and tab_ok)
    r.update(status=0, mode=mode, gen=int(gen and mode == FAST), genW=gen_w, walk_parts_log2={4: 2, 2: 1}.get(parts, 0), nh=nhq, lk=lkq,
             quadW=wq, quadSH=0 if ring(xbq, nhq, lkq) <= 65535 else 4, quad=int(quad), xb=32 if gen else (xbq if quad else 16), dquad=0)
    if (mode == EXACT and not f32 and uniform and aperture_ok and (2.0 * g['hest'] + 400.0) / 4.0 * snum * 32.0 < 2 ** 31 and
            'EXACT_IMPL' not in env and not c['caller_tables']):
        def fits(xb, nh):
            b = rows(sa, xb, nh, 4) // 32 * kd_piece(xb)
            return b <= 80 * 1024 and (nh == 1 or b > 65535)
        nhd = int(env['NHD']) if 'NHD' in env else (2 if ('XBD' not in env and fits(20, 2) and tnum >= 8000 * nranks) else 1)
        if nhd != 2 or near:
            nhd = 1
        xbd = int(env['XBD']) if env.get('XBD') in ('16', '20') else (16 if (nhd == 2 and 'NHD' in env) else 20)
        if nhd == 2 and not fits(xbd, 2):
            nhd = 1
        if not fits(xbd, nhd):
            xbd = 16
        if fits(xbd, nhd):
            w = rows(sa, xbd, nhd, 4)
            r.update(dquad=1, xb=xbd, nh=nhd, quadW=w, quadSH=0 if w // 32 * kd_piece(xbd) <= 65535 else 4)
    pair = env.get('EXACT_IMPL') == 'pair'
    r['want_tie_scan'] = int(uniform and not r['gen'] and not c['caller_tables'] and (mode == FAST or bool(r['dquad']) or not pair))
    r['xtab_off'] = int(c['caller_tables'])
    if r['gen']:
        r['kernel'] = 'GEN'
    elif mode == FAST:
        r['kernel'] = 'QUAD' if quad else 'TAB'
    elif r['dquad']:
        r['kernel'] = 'DQUAD'
    else:
        r['kernel'] = 'EXACT_TAB' if (uniform and not r['xtab_off'] and not pair) else 'EXACT_PAIR'
    return r


@pytest.mark.parametrize('c', KC.CASES, ids=KC.IDS)
def test_route_is_what_plan_create_decided(lib, c):
    got, g = KC.route(lib, c), geometry(c)
    for k in ('increasing', 'uni_t', 'uni_t11', 'uni_x', 'dist_sorted'):
        assert bool(got[k]) == g[k], k
    if not g['increasing']:
        return                                                  # the argument error: nothing else is looked at
    for k in ('tmax', 'dt', 'dx', 'xnoise', 'sa', 'alpha', 'hest', 'gen_need'):
        assert got[k] == g[k], k                                # the same float64 operations in the same order: bit for bit
    want = model(c, g)
    if c['caller_tables']:
        # (the commit before rewrote four fields of a finished plan here; what its ring would have been is not part of the result)
        want = {k: want[k] for k in ('status', 'mode', 'kernel', 'tnum_pad', 'dquad', 'xtab_off', 'want_tie_scan', 'gen', 'quad')}
    assert {k: got[k] for k in want} == want


def test_every_branch_is_reached(lib):
    """The preconditions the cases stand for (so that a change of a threshold cannot quietly empty a case)."""
    r = {c['id']: KC.route(lib, c) for c in KC.CASES}

    def ring(i):
        return (r[i]['kernel'], r[i]['xb'], r[i]['nh'], r[i]['lk'], r[i]['quadSH'])
    assert ring('f32-sa1.2') == ('QUAD', 40, 1, 0, 4) and ring('f32-sa4') == ('QUAD', 24, 1, 0, 0) and ring('f32-sa5') == ('QUAD', 24, 1, 0, 4)
    assert ring('f32-XB=24') == ('QUAD', 24, 1, 0, 0) and ring('f32-XB=32') == ('QUAD', 32, 1, 0, 0)
    assert r['f32-sa10']['kernel'] == 'TAB' and r['f32-sa20']['kernel'] == 'GEN' and r['f32-sa20']['genW'] == 1024
    assert r['f32-sa30-fast']['status'] == KC.UNSUPPORTED and r['f32-sa30-auto']['kernel'] == 'EXACT_TAB'
    assert r['f32-sa1.2-exact']['kernel'] == 'EXACT_TAB' and r['f32-exact-EXACT_IMPL=pair']['kernel'] == 'EXACT_PAIR'
    assert ring('f32-pair-r1') == ('QUAD', 32, 2, 0, 4) and r['f32-pair-r1']['walk_parts_log2'] == 0
    assert [(ring('f32-pair-r%d' % n)[1:3], r['f32-pair-r%d' % n]['walk_parts_log2']) for n in (2, 4, 8)] == [((40, 1), 0), ((40, 1), 1), ((40, 1), 2)]
    assert ring('f32-pair-sa0.5')[1:3] == (40, 1) and ring('f32-near-pair')[1:3] == (40, 1) and ring('f32-pair-XB=7')[1:3] == (40, 1)
    assert ring('f32-XB=32')[1] == 32 and ring('f32-XB=7')[1] == 40
    assert ring('f32-NH=2')[1:4] == (40, 2, 0) and ring('f32-NH=3')[1:4] == (40, 3, 0) and ring('f32-NH=2-LK=1')[1:4] == (40, 2, 1)
    assert ring('f32-LK=1')[2:4] == (1, 0) and ring('f32-sa4-NH=2')[1:3] == (24, 1)
    assert r['f32-IMPL=tab']['kernel'] == 'TAB' and r['f32-IMPL=gen']['kernel'] == 'GEN' and r['f32-sa20-IMPL=tab']['kernel'] == 'GEN'
    assert r['f32-PARTS=2']['walk_parts_log2'] == 1 and r['f32-PARTS=4']['walk_parts_log2'] == 2
    assert ring('f64-pair') == ('DQUAD', 20, 2, 0, 4) and ring('f64-pair-r2')[1:3] == (20, 1)
    assert [ring(i)[:3] for i in ('f64-sa1.2', 'f64-sa3', 'f64-sa5')] == [('DQUAD', 20, 1), ('DQUAD', 20, 1), ('DQUAD', 16, 1)]
    assert r['f64-sa8']['kernel'] == 'EXACT_TAB' and r['f64-auto']['kernel'] == 'DQUAD' and r['f64-fast']['status'] == KC.UNSUPPORTED
    assert ring('f64-XBD=16')[1:3] == (16, 1) and ring('f64-XBD=20')[1:3] == (20, 1) and ring('f64-NHD=2')[1:3] == (16, 2)
    assert ring('f64-NHD=2-XBD=20')[1:3] == (20, 2) and ring('f64-sa1.2-NHD=2')[1:3] == (16, 1) and ring('f64-near-NHD=2')[1:3] == (20, 1)
    assert r['f64-EXACT_IMPL=tab']['kernel'] == 'EXACT_TAB' and r['f64-EXACT_IMPL=pair']['kernel'] == 'EXACT_PAIR'
    assert r['f64-EXACT_IMPL=tab']['want_tie_scan'] and not r['f64-EXACT_IMPL=pair']['want_tie_scan']
    assert [r[i]['kernel'] for i in ('32-jitter', '32-zigzag', '64-jitter', '64-zigzag')] == ['GEN', 'EXACT_PAIR', 'EXACT_PAIR', 'EXACT_PAIR']
    assert r['f32-zigzag-fast']['status'] == KC.UNSUPPORTED and r['f32-jitter-exact']['kernel'] == 'EXACT_PAIR'
    assert r['f32-tt-e-10']['uni_t'] and not r['f32-tt-e-10']['uni_t11'] and not r['f32-tt-e-8']['uni_t']
    assert [r['f32-' + i]['kernel'] for i in ('tt-e-10', 'jitter-tt-e-10', 'tt-e-8', 'jitter-tt-e-8')] == ['QUAD', 'EXACT_PAIR', 'EXACT_PAIR', 'EXACT_PAIR']
    assert r['f64-tt-e-10']['kernel'] == 'DQUAD' and r['f64-tt-e-8']['kernel'] == 'EXACT_PAIR' and not r['f32-tt-flat']['increasing']
    for lim in ('snum65536', 'aperture', 'span'):
        # (tens of thousands of samples of 1e-8 s through the unit conversions are a grid to 1e-9 dt but not to 1e-11 dt: no gen kernel either)
        assert r['32-' + lim]['kernel'] == ('GEN' if r['32-' + lim]['uni_t11'] else 'EXACT_TAB') and r['64-' + lim]['kernel'] == 'EXACT_TAB', lim
    assert r['f32-tnum1']['kernel'] == 'QUAD'
    assert r['f64-hook-standard']['kernel'] == 'DQUAD' and r['f64-hook-standard']['tmax'] == float(np.float32(299 * KC.DT))
    own = r['f64-hook-own']
    assert own['kernel'] == 'EXACT_PAIR' and own['xtab_off'] and not own['dquad'] and not own['want_tie_scan'] and own['tmax'] == 0.9 * r['f64-hook-standard']['tmax']


@pytest.mark.parametrize('cid,mode', [('f32-sa1.2', AUTO), ('f32-sa1.2-fast', FAST), ('f32-sa10', AUTO), ('f64-sa1.2', EXACT), ('f64-EXACT_IMPL=tab', EXACT),
                                      ('f32-TIEFIX=0', AUTO)])
def test_route_after_ties(lib, cid, mode):
    """The tie scan's count against the list's capacity: 0 and in range keep the route (in range: the list is kept); over the cap
    -- or any tie with the correction off -- an AUTO request falls back to EXACT per pair, an explicit FAST keeps its ring, the
    float64 ring and the tabulated kernel are dropped."""
    c = KC.CASES[KC.IDS.index(cid)]
    assert c['mode'] == mode
    base, cap = KC.route(lib, c), 1 << 20
    nofix = c['env'].get('IMPDAR_KIRCH_TIEFIX') == '0'
    for count in (0, 1, cap, cap + 1):
        r = KC.route(lib, c, ties=count, cap=cap)
        ambiguous = count > cap or (count > 0 and nofix)
        assert r['tie_ambiguous'] == ambiguous and r['want_tie_groups'] == (0 < count <= cap and not nofix)
        if not ambiguous:
            assert {k: r[k] for k in base if k not in ('want_tie_groups',)} == {k: base[k] for k in base if k not in ('want_tie_groups',)}
            continue
        assert r['xtab_off'] and not r['dquad']
        if base['mode'] == FAST and mode == AUTO:
            assert (r['mode'], r['quad'], r['xb'], r['kernel']) == (EXACT, 0, 16, 'EXACT_PAIR')
        elif base['mode'] == FAST:
            assert (r['mode'], r['quad'], r['xb'], r['kernel']) == (FAST, base['quad'], base['xb'], base['kernel'])
        else:
            assert r['mode'] == EXACT and r['kernel'] == 'EXACT_PAIR'


# ---- the host tables against NumPy: snum 300 (two chunks, the second ragged), tnum 96, tt[0] before, at and after the trigger
TABLE_CASES = [KC.case('tab-%s-%s' % (d[-2:], n), d, t0_us=t0, mode=m, env=e)
               for d, m, e in (('float32', AUTO, {}), ('float32', AUTO, {'IMPDAR_KIRCH_NH': '2'}), ('float32', AUTO, {'IMPDAR_KIRCH_IMPL': 'tab'}),
                               ('float64', EXACT, {}))
               for n, t0 in (('before', -0.03), ('at', 0.0), ('after', 0.05))]


@pytest.mark.parametrize('c', TABLE_CASES, ids=['%s-%s' % (c['id'], '-'.join(c['env'].values())) for c in TABLE_CASES])
def test_tables_against_numpy(lib, c):
    r, g, T = KC.route(lib, c), geometry(c), KC.tables(lib, c)
    _, tt = KC.axes(c)
    snum, tnum, dt, alpha, vel = c['snum'], c['tnum'], g['dt'], g['alpha'], KC.VEL
    a, um = tt / dt, g['tmax'] / dt
    rem = um * um - a * a
    h_half = np.where(rem < 0, -1, np.floor(np.sqrt(np.maximum(rem, 0) / alpha) + 1e-12)).astype(np.int64)
    assert np.array_equal(T['h_half'], h_half)
    # per-sample factors: float64 from zs = v t / 2, float32 from a = t / dt; a sample at t = 0 gets zeros
    zs = vel * tt / 2.0
    with np.errstate(divide='ignore', invalid='ignore'):
        want64 = np.where(zs == 0, 0.0, [np.minimum((g['dx'] / zs) * (g['dx'] / zs), 1e300), np.minimum(vel / (zs * zs), 1e300),
                                         np.sign(zs) / (2.0 * np.pi * vel)])
        half = vel * dt / 2.0
        want32 = np.where(a == 0, 0.0, [np.minimum(alpha / (a * a), 1e30), np.minimum(vel / (half * half * a * a), 1e30),
                                        np.sign(a) / (2.0 * np.pi * vel)]).astype(np.float32)
    assert np.array_equal(T['c64'], want64) and np.array_equal(T['c32'].view(np.uint32), want32.view(np.uint32))
    assert (c['t0_us'] == 0.0) == bool(np.any(T['c64'][2] == 0)) and (c['t0_us'] < 0) == bool(np.any(T['c64'][2] < 0))
    # per-chunk tables
    S = 4 if r['dquad'] else 8
    nch = 2
    chunks = [slice(0, 256), slice(256, snum)]
    hglob = min(max(h_half.max() + 1, 0), tnum + 128)
    hmax = [min(max(h_half[s].max() + 1, 0), hglob) for s in chunks]
    assert T['nchunks'] == nch and T['hmax'].tolist() == hmax and not T['refused']
    assert (T['nb'], T['ntab'], T['mrow0'], T['nrows']) == (hglob + 64, hglob + 1, hglob // S + 8, 2 * (hglob // S) + 64)
    n = np.arange(T['nb'], dtype=np.float64)
    u0 = tt[0] / dt
    for ci, s in enumerate(chunks):
        cmin, cmax = (a[s] * a[s]).min(), (a[s] * a[s]).max()
        klo = np.maximum(0, np.floor(np.sqrt(cmin + alpha * n * n) - u0).astype(np.int64) - 1)
        khi = np.minimum(snum - 1, np.ceil(np.sqrt(cmax + alpha * n * n) - u0).astype(np.int64) + 1)
        assert np.array_equal(T['klo'][ci], klo) and np.array_equal(T['khi'][ci], khi)
        if r['kernel'] == 'TAB':
            assert T['win'] is None
            continue
        # the window of step block row: the offsets its S traces are read at, by every tile of the workgroup
        rr = np.arange(T['nrows'])
        nz = S * (rr - T['mrow0']) + 1 + r['xb'] + S - 2
        na = S * (rr - T['mrow0']) + 1 - (r['nh'] - 1) * r['xb']
        lo = np.where((na <= 0) & (nz >= 0), 0, np.minimum(np.abs(na), np.abs(nz)))
        hi = np.maximum(np.abs(na), np.abs(nz))
        kmin, kmax = klo[np.minimum(lo, T['nb'] - 1)], khi[np.minimum(hi, T['nb'] - 1)]
        assert np.array_equal(T['win'][ci, :, 0], kmin | ((kmin % r['quadW']) << 16)) and np.array_equal(T['win'][ci, :, 1], kmax)
    assert r['kernel'] == {'float64': 'DQUAD'}.get(c['dtype'], 'TAB' if c['env'].get('IMPDAR_KIRCH_IMPL') else 'QUAD')


def test_tie_grouping(lib):
    pairs = [(7, 3), (2, 9), (7, 1), (2, 4), (299, 0), (7, 2)]
    assert KC.group_ties(lib, pairs) == ([2, 7, 299], [0, 2, 5, 6], [4, 9, 1, 2, 3, 0])
    assert KC.group_ties(lib, [(5, 5)]) == ([5], [0, 1], [5])


def _tilemap_args(m):
    return (m['hmax'], m['tnum'], m['xlo'], m['xhi'], m['tile_w'], m['align_mask'], m['ring_blocks'], m['step_block'], m['G'], m['tiles_per_xcd'])


def test_tilemap(lib):
    """Every tile once per chunk, no XCD over its share, and the map the commit before built (tests/kirch_route_recorded.json)."""
    with open(KC.RECORDED) as f:
        maps = json.load(f)['tilemaps']
    assert len(maps) >= 4
    for m in maps:
        got = KC.tilemap(lib, *_tilemap_args(m))
        x00 = m['xlo'] & ~m['align_mask']
        nxt = (m['xhi'] - x00 + m['tile_w'] - 1) // m['tile_w']
        assert got is not None and got.shape == (len(m['hmax']), m['tiles_per_xcd'], 8)
        for c in range(len(m['hmax'])):
            assert sorted(got[c][got[c] >= 0].tolist()) == list(range(nxt))
            assert all((got[c][:, x] >= 0).sum() <= m['tiles_per_xcd'] for x in range(8))
            # groups of G adjacent tiles stay on one XCD, in adjacent slots
            for q in range(0, m['tiles_per_xcd'], m['G']):
                for x in range(8):
                    grp = got[c][q:q + m['G'], x]
                    assert grp[0] < 0 or (grp[0] % m['G'] == 0 and all(t in (-1, grp[0] + i) for i, t in enumerate(grp)))
        assert got.ravel().tolist() == m['map']
    # more tiles than a 16-bit entry holds: the arithmetic rule
    assert KC.tilemap(lib, [10], 40000 * 24, 0, 40000 * 24, 24, 7, 5, 8, 4, 40000 // 8) is None


@pytest.mark.parametrize('tnum,halo,two,cut,need', [
    (4100, 2000, False, [0, 408, 1640, 2864, 4100], [2408, 3640, 4100, 4100]),
    (4100, 2050, False, [0, 2560, 4100], None),          # 1640 + 2050 is not below 3690: the two-block form
    (4100, 2000, True, [0, 2560, 4100], [4100, 4100]),
    (10000, 500, False, [0, 1000, 4000, 7000, 10000], None),
])
def test_oneshot_cuts_where_the_rule_turns(lib, tnum, halo, two, cut, need):
    """The cut planner of the one-shot entry point (default KOS_PCT) at the values where it changes form."""
    got_cut, got_need = KC.oneshot_cuts(lib, tnum, halo, two)
    assert got_cut == cut
    assert len(got_need) == len(cut) - 1
    if need is not None:
        assert got_need == need


def test_oneshot_cuts_properties(lib):
    """Over a sweep of (tnum, halo): cuts strictly increase from 0 to tnum, interior cuts are multiples of 8, and what a block
    needs on the device never shrinks, covers the block's right edge and stays inside the radargram."""
    for tnum in (4096, 4097, 4100, 4103, 5000, 8191, 10000, 12345, 65536, 100001):
        for halo in (16, 17, 100, tnum // 10, tnum // 4, tnum // 2 - 1, tnum // 2, tnum // 2 + 1, tnum, 3 * tnum):
            for two in (False, True):
                cut, need = KC.oneshot_cuts(lib, tnum, halo, two)
                assert len(cut) in (3, 5) and len(need) == len(cut) - 1, (tnum, halo, two)
                assert cut[0] == 0 and cut[-1] == tnum and all(a < b for a, b in zip(cut, cut[1:])), (tnum, halo, two, cut)
                assert all(c % 8 == 0 for c in cut[1:-1]), (tnum, halo, two, cut)
                assert all(a <= b for a, b in zip(need, need[1:])), (tnum, halo, two, need)
                assert all(cut[i + 1] <= need[i] <= tnum for i in range(len(need))), (tnum, halo, two, cut, need)


def test_route_agrees_with_what_the_library_reported(lib):
    """tests/kirch_route_recorded.json: impdar_kirch_plan_kernel / _mode / _tnum_pad / _xnoise of the gpu cases from a GPU run of
    the commit before kirch_route.h."""
    with open(KC.RECORDED) as f:
        rec = json.load(f)['cases']
    assert sorted(rec) == sorted(c['id'] for c in KC.GPU_CASES)
    for c in KC.GPU_CASES:
        r, m = KC.route(lib, c, ties=0), rec[c['id']]          # (no profile of these sizes has more ties than the list holds)
        assert (r['kernel'], r['mode'], r['tnum_pad'], r['xnoise']) == (m['kernel'], m['mode'], m['tnum_pad'], m['xnoise']), c['id']


def test_knobs_from_env(tmp_path):
    """KirchKnobs::from_env: one read per knob, "set" apart from the value, and equality as the plan caches use it."""
    import os
    import subprocess
    src, exe = str(tmp_path / 'knobs.cpp'), str(tmp_path / 'knobs')
    with open(src, 'w') as f:
        f.write('#include "kirch_route.h"\n#include <cstdio>\nint main() { const KirchKnobs K = KirchKnobs::from_env();\n'
                'printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\\n", K.xb_set, K.xb, K.nh_set, K.nh, K.lk_set, K.lk, K.parts_set, K.parts,'
                ' K.nhd_set, K.nhd, K.xbd_set, K.xbd, K.impl, K.exact_impl, K.tiefix_off, K == KirchKnobs()); return 0; }\n')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(root, 'impdar_amd', 'csrc'), src, '-o', exe])
    clean = {k: v for k, v in os.environ.items() if not k.startswith('IMPDAR_KIRCH_')}

    def read(env):
        out = subprocess.run([exe], env=dict(clean, **env), capture_output=True, text=True, check=True).stdout.split()
        return [int(v) for v in out]
    assert read({}) == [0] * 15 + [1]
    assert read({'IMPDAR_KIRCH_MODE': 'fast', 'IMPDAR_KIRCH_RESERVE': '8'})[-1] == 1          # no plan knobs of the C side
    for env in ({'IMPDAR_KIRCH_XB': 'x'}, {'IMPDAR_KIRCH_XB': '24', 'IMPDAR_KIRCH_NH': '3', 'IMPDAR_KIRCH_LK': '1', 'IMPDAR_KIRCH_PARTS': '4'},
                {'IMPDAR_KIRCH_NHD': '2', 'IMPDAR_KIRCH_XBD': '16'}, {'IMPDAR_KIRCH_IMPL': 'tab'}, {'IMPDAR_KIRCH_IMPL': 'gen'},
                {'IMPDAR_KIRCH_IMPL': 'other'}, {'IMPDAR_KIRCH_EXACT_IMPL': 'tab'}, {'IMPDAR_KIRCH_EXACT_IMPL': 'pair'},
                {'IMPDAR_KIRCH_EXACT_IMPL': ''}, {'IMPDAR_KIRCH_TIEFIX': '0'}, {'IMPDAR_KIRCH_TIEFIX': '1'}):
        got = read(env)
        assert got[:15] == KC.knob_array(env).tolist(), env
        assert got[15] == int(env in ({'IMPDAR_KIRCH_IMPL': 'other'}, {'IMPDAR_KIRCH_TIEFIX': '1'})), env
