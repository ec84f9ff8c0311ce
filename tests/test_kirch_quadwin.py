"""The quad-aligned output window of kirch_quad_kernel (KIRCH_WINDOW_QUAD, csrc/kirch_route.h) without a GPU: the cover of a
launch restated on the host from the functions the kernel itself steps by (kq_win_first_quad, kq_win_acc, kirch_walk_range,
kirch_tile_origin / kirch_tile_count), driven through the header's probe (compiled here by itself with g++).  Per step: which
ring slots are read, which output each component feeds, and whether the slot's ring group holds that trace at that moment.
The same probe runs as a stand-alone program under AddressSanitizer and UBSan (tests/san/kirch_quadwin_fuzz.cpp)."""
import ctypes as C

import numpy as np
import pytest

import kirch_route_cases as KC

SLIDE, QUAD = 0, 1
_ip, _lp = C.POINTER(C.c_int), C.POINTER(C.c_longlong)
STATS = ('tiles', 'steps', 'reads', 'unused', 'unstaged', 'wrong_slot', 'acc_max', 'fixed_up')


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return KC.probe(str(tmp_path_factory.mktemp('kirchquadwin')))


def cover(lib, tnum, xlo, xhi, xb, nh, lk, hmax, parts_log2, window):
    count = np.zeros((xhi - xlo, 2 * hmax + 1), dtype=np.int32)
    written = np.zeros(xhi - xlo, dtype=np.int32)
    stats = np.zeros(8, dtype=np.int64)
    rc = lib.impdar_kirch_quadwin_cover_probe(tnum, xlo, xhi, xb, nh, lk, hmax, parts_log2, window, count.ctypes.data_as(_ip),
                                              written.ctypes.data_as(_ip), stats.ctypes.data_as(_lp))
    assert rc == 0
    return count, written, dict(zip(STATS, (int(v) for v in stats)))


def valid_pairs(tnum, xlo, xhi, hmax):
    """(output, offset) pairs of the block whose input trace lies in the profile."""
    x = np.arange(xlo, xhi)[:, None]
    n = np.arange(-hmax, hmax + 1)[None, :]
    return (x + n >= 0) & (x + n < tnum)


# a full profile each of 64, 128 and 300 traces, and two blocks of the 300: one that starts and ends off every tile start, one
# whose last column is the last of a tile for every width here (the tile right of it then only holds left-edge sums -- of real
# neighbouring traces)
BLOCKS = [(64, 0, 64), (128, 0, 128), (300, 0, 300), (300, 13, 141), (300, 0, 64)]
# apertures: a few traces, the 520-sample test geometry's, wider than every profile here
HMAX = (3, 38, 400)


@pytest.mark.parametrize('xb', (24, 32, 40))
@pytest.mark.parametrize('nh', (1, 2, 3))
def test_every_pair_is_taken_exactly_once(lib, xb, nh):
    for tnum, xlo, xhi in BLOCKS:
        for hmax in HMAX:
            for lk in (0, 1):
                for pl2 in ((0, 1, 2) if nh == 1 else (0,)):
                    count, written, s = cover(lib, tnum, xlo, xhi, xb, nh, lk, hmax, pl2, QUAD)
                    key = (tnum, xlo, xhi, xb, nh, lk, hmax, pl2)
                    valid = valid_pairs(tnum, xlo, xhi, hmax)
                    assert np.all(count[valid] == 1), (key, np.argwhere(valid & (count != 1))[:4])
                    assert np.all(count <= 1), key                    # (pairs off the profile meet zero rows; still no tile twice)
                    # no read off a staged group, every component on the slot of its pair, none without an accumulator
                    assert s['unstaged'] == 0 and s['wrong_slot'] == 0 and s['unused'] == 0, (key, s)
                    assert s['reads'] == s['steps'] * (xb // 4) and s['acc_max'] == xb + 2, (key, s)
                    # tiles start at multiples of the workgroup tile and reach the column right of the block
                    x00 = (xlo // (xb * nh)) * (xb * nh)
                    nxt = -(-(xhi + 3 - x00) // (xb * nh))
                    assert s['fixed_up'] == nxt * nh - 1, (key, s)
                    assert s['tiles'] <= nxt << pl2 and (pl2 or s['tiles'] == nxt), (key, s)
                    assert np.all(written == 1) if pl2 == 0 else (np.all(written >= 1) and np.all(written <= 1 << pl2)), (key, written)


def test_a_block_that_ends_on_a_tile_gets_the_tile_right_of_it(lib):
    """[0, 64) of 300 traces in tiles of 32: two tiles hold the columns, the third one the rest of columns 61 .. 63."""
    _, _, q = cover(lib, 300, 0, 64, 32, 1, 0, 38, 0, QUAD)
    _, _, s = cover(lib, 300, 0, 64, 32, 1, 0, 38, 0, SLIDE)
    assert (q['tiles'], s['tiles']) == (3, 2)
    # ... and without it the pairs of those three columns at the offsets n & 3 > 0 would have no taker: one tile fewer
    count, _, _ = cover(lib, 300, 0, 61, 32, 1, 0, 38, 0, QUAD)          # (a block that needs two tiles only)
    assert np.all(count[valid_pairs(300, 0, 61, 38)] == 1)


@pytest.mark.parametrize('xb', (24, 32, 40))
def test_the_sliding_window_by_the_same_model(lib, xb):
    """The model reproduces what is known of the sliding form: every pair once, XB/4 + 0.75 quad reads per step, 3 components in
    every 4 steps without an accumulator (profiles/r04_edge_quads.txt)."""
    for tnum, xlo, xhi in BLOCKS:
        count, written, s = cover(lib, tnum, xlo, xhi, xb, 1, 0, 38, 0, SLIDE)
        assert np.all(count[valid_pairs(tnum, xlo, xhi, 38)] == 1) and np.all(count <= 1) and np.all(written == 1)
        assert s['unstaged'] == 0 and s['wrong_slot'] == 0 and s['fixed_up'] == 0
        assert 4 * s['reads'] == s['steps'] * (xb + 3) and s['unused'] == 3 * s['steps'], s


def _route_window(lib, c, window, tables=True):
    """(route ints incl. the window kind, tables) of a case under the probe's window kind (1 slide, 2 quad)."""
    assert lib.impdar_kirch_window_probe(window) == 0
    try:
        dist, tt = KC.axes(c)
        ints, dbls = np.zeros(32, dtype=np.int32), np.zeros(16)
        _dp = C.POINTER(C.c_double)
        lib.impdar_kirch_route_probe.argtypes = [C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                 _ip, C.c_longlong, C.c_longlong, _ip, _dp]
        assert lib.impdar_kirch_route_probe(0, c['snum'], c['tnum'], dist.ctypes.data_as(_dp), tt.ctypes.data_as(_dp), KC.VEL, 0, c['mode'],
                                            c['nranks'], None, 0, KC.knob_array(c['env']).ctypes.data_as(_ip), -1, 1 << 20,
                                            ints.ctypes.data_as(_ip), dbls.ctypes.data_as(_dp)) == 0
        r = {k: int(v) for k, v in zip(KC.INTS, ints)}
        r['window'] = int(ints[25])
        return r, (KC.tables(lib, c) if tables and r['quad'] else None)
    finally:
        lib.impdar_kirch_window_probe(1)


def _ring_rows(sa, xb, nh, extra=0):
    return (256 + int(np.ceil(sa * (xb * nh + 6 + extra))) + 8 + 31) // 32 * 32


def _check_windows(r, T):
    """Every staging window fits the ring's rows: every chunk, every table row."""
    kmin, kmax = T['win'][:, :, 0] & 0xffff, T['win'][:, :, 1]
    assert np.all(kmax - kmin + 1 <= r['quadW']), (r, int((kmax - kmin + 1).max()))
    return int((kmax - kmin + 1).max())


def test_staging_windows_fit_the_ring_at_config3(lib):
    """4096 x 10000 at the benchmark's moveout: two tiles of 32, the ring's rows are 352 with and without the 3 further traces
    (347 and 351 before rounding to whole pieces), so the aligned window is routed; every window of its table fits."""
    c = KC.case('config3', snum=4096, tnum=10000, sa=2.0 / (KC.VEL * KC.DT))
    rs, Ts = _route_window(lib, c, 1)
    rq, Tq = _route_window(lib, c, 2)
    assert (rq['xb'], rq['nh'], rq['quadW'], rq['window']) == (32, 2, 352, QUAD) and rs['window'] == SLIDE
    assert {k: v for k, v in rq.items() if k != 'window'} == {k: v for k, v in rs.items() if k != 'window'}       # nothing else of the route moves
    wq, ws = _check_windows(rq, Tq), _check_windows(rs, Ts)
    print('config 3: widest staging window %d rows (sliding %d) of %d' % (wq, ws, rq['quadW']))
    assert wq >= ws


@pytest.mark.parametrize('xb,nh', [(24, 1), (32, 1), (40, 1), (32, 2), (40, 2), (40, 3)])
def test_staging_windows_fit_the_ring_at_the_steepest_routed_moveout(lib, xb, nh):
    """Per tile width: the steepest moveout (in steps of 0.01 samples per trace) at which the route still takes the aligned
    window -- the last one before the 3 further traces would need another piece of ring rows, or before the width itself is no
    longer routed.  One step steeper the plan keeps the sliding window (or another kernel) with the slot size it had."""
    env = {'IMPDAR_KIRCH_XB': str(xb), 'IMPDAR_KIRCH_NH': str(nh)}
    best = None
    for sa100 in range(30, 1200):
        sa = sa100 / 100.0
        c = KC.case('steep', snum=520, tnum=300, sa=sa, mode=KC.FAST, env=env)
        dist, tt = KC.axes(c)
        r, _ = _route_window(lib, c, 2, tables=False)
        if r['status'] != 0 or not r['quad'] or (r['xb'], r['nh']) != (xb, nh):
            continue
        rs, _ = _route_window(lib, c, 1, tables=False)
        assert r['quadW'] == rs['quadW'] and r['quadSH'] == rs['quadSH']            # the slot size is never the window kind's
        sa_ = 2.0 * (dist[1] - dist[0]) / (KC.VEL * KC.DT)
        # (for one, two and three tiles per workgroup alike: the window kind is the geometry's and the tile width's)
        def holds(s):
            return _ring_rows(s, xb, nh, 3) == r['quadW'] and all(_ring_rows(s, xb, k, 3) == _ring_rows(s, xb, k) for k in (1, 2, 3))
        # (a moveout times a trace count that is a whole number rounds either way: judged only where both neighbours agree)
        if holds(sa_ * (1 - 1e-12)) == holds(sa_ * (1 + 1e-12)):
            assert (r['window'] == QUAD) == holds(sa_), (sa, r)
        if r['window'] == QUAD:
            best = c
    assert best is not None
    r, T = _route_window(lib, best, 2)
    widest = _check_windows(r, T)
    print('XB %d NH %d: aligned window routed up to sa = %.2f, ring rows %d, widest staging window %d' % (xb, nh, best['sa'], r['quadW'], widest))
