"""The queue lists of the persistent Kirchhoff ring kernels (kirch_gangmap, csrc/kirch_route.h; compiled here by itself with g++: no
GPU, no HIP): gangs of G adjacent tiles of a chunk whole on one XCD in consecutive positions, and the packed order -- all gangs
of all chunks longest first by the tile map's cost model, each dealt to the XCD with the least cost so far -- beside the chunk
order (the tile map's own, chunk by chunk).

The replay at the end runs both orders through the cost model as the kernel would pull them: 64 workgroup slots per XCD, each
taking the next item of its own XCD's list and, once that is empty, the next unread item of the other XCDs' lists in turn
(kirch_ring_queue_item).  An item costs what the tile map charges for it, in step blocks."""
import ctypes as C
import heapq

import numpy as np
import pytest

import kirch_route_cases as KC

CHUNK, PACKED = 0, 1
SA = 2.0 / 1.69            # samples of moveout per trace: dx = 1 m, dt = 10 ns, v = 1.69e8 m/s


def hmax_of(snum, tnum, sa=SA):
    """Aperture half widths per 256-sample chunk (+ 1), as kirch_half_widths / kirch_ring_tables give them for tt = k dt."""
    k = np.arange(snum, dtype=np.float64)
    h = np.floor(np.sqrt(np.maximum((snum - 1.0) ** 2 - k * k, 0.0) / (sa * sa)) + 1e-12).astype(np.int64)
    hm = [int(h[c:c + 256].max()) + 1 for c in range(0, snum, 256)]
    return [min(v, min(max(hm), tnum + 128)) for v in hm]


# name: hmax per chunk, tnum, xlo, xhi, tile width, alignment mask, ring blocks, step block
SHAPES = {
    # bench.py's radargram: 16 chunks, 157 workgroup tiles of 2 x 32 traces
    'config3': (hmax_of(4096, 10000), 10000, 0, 10000, 64, 7, 6, 8),
    # an output block of a rank of an 8-rank plan on the 40000-trace radargram: 63 tiles of 40 traces
    'rank_block': (hmax_of(4096, 40000), 40000, 5000, 7500, 40, 7, 7, 8),
    # a ragged block of a 300-trace profile, 3 chunks (the last of 8 samples)
    'ragged': (hmax_of(520, 300), 300, 13, 141, 40, 7, 7, 8),
}


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return KC.probe(str(tmp_path_factory.mktemp('kirchgang')))


def gangmap(lib, shape, G, order):
    """The eight lists of (chunk, tile) of a launch."""
    hmax, tnum, xlo, xhi, tile_w, mask, ring_blocks, step_block = shape
    hm = np.ascontiguousarray(hmax, dtype=np.int32)
    nxt = (xhi - (xlo & ~mask) + tile_w - 1) // tile_w
    lens, items = np.zeros(8, dtype=np.int32), np.full(len(hm) * nxt + 8, -1, dtype=np.int32)
    ip = C.POINTER(C.c_int)
    n = lib.impdar_kirch_gangmap_probe(hm.ctypes.data_as(ip), len(hm), tnum, xlo, xhi, tile_w, mask, ring_blocks, step_block, G, order,
                                       lens.ctypes.data_as(ip), items.ctypes.data_as(ip))
    assert n == int(lens.sum()) <= len(hm) * nxt
    ends = np.cumsum(lens)
    return [[(int(it) >> 16, int(it) & 0xffff) for it in items[e - l:e]] for l, e in zip(lens, ends)]


def tile_cost(shape, c, t):
    """What kirch_tilemap charges for tile t of chunk c: its walk in step blocks, whole ring revolutions, plus a prologue's worth."""
    hmax, tnum, xlo, _, tile_w, mask, ring_blocks, step_block = shape
    x0 = (xlo & ~mask) + t * tile_w
    nlo, nhi = max(-hmax[c], -(x0 + tile_w - 1)), min(hmax[c], tnum - 1 - x0)
    blocks = max(0, nhi - nlo + step_block) // step_block
    return (blocks + ring_blocks - 1) // ring_blocks * ring_blocks + 8


def gangs_of(lst, G):
    """A list cut into its gangs: runs of one chunk that start at a multiple of G and stay inside that gang."""
    out = []
    for c, t in lst:
        if out and out[-1][0] == c and t // G == out[-1][1][0] // G:
            out[-1][1].append(t)
        else:
            out.append((c, [t]))
    return out


@pytest.mark.parametrize('G', [1, 2, 4])
@pytest.mark.parametrize('name', list(SHAPES))
def test_packed_lists(lib, name, G):
    shape = SHAPES[name]
    hmax, _, xlo, xhi, tile_w, mask = shape[:6]
    nxt = (xhi - (xlo & ~mask) + tile_w - 1) // tile_w
    lists = gangmap(lib, shape, G, PACKED)
    # every (chunk, tile) exactly once over the eight lists -- in the chunk order of the same G too
    want = sorted((c, t) for c in range(len(hmax)) for t in range(nxt))
    assert sorted(it for lst in lists for it in lst) == want
    assert sorted(it for lst in gangmap(lib, shape, G, CHUNK) for it in lst) == want
    loads, largest = [], 0
    for lst in lists:
        gangs = gangs_of(lst, G)
        for c, tiles in gangs:
            # a gang: adjacent tiles from a multiple of G, whole (but for the profile's last) -- so on one XCD, in consecutive positions
            assert tiles[0] % G == 0 and tiles == list(range(tiles[0], min(tiles[0] + G, nxt)))
        # a gang's tiles run side by side: it is as long as its longest tile, and weighs their sum on its XCD's list
        costs = [[tile_cost(shape, c, t) for t in tiles] for c, tiles in gangs]
        assert all(max(a) >= max(b) for a, b in zip(costs, costs[1:])), 'costs rise along a list'
        loads.append(sum(sum(g) for g in costs))
        largest = max([largest] + [sum(g) for g in costs])
    assert max(loads) - min(loads) <= largest


def test_chunk_order_is_the_tile_map(lib):
    """The chunk order is kirch_tilemap's map read slot by slot (what the queue pulled before it read lists)."""
    hmax, tnum, xlo, xhi, tile_w, mask, ring_blocks, step_block = SHAPES['config3']
    m = KC.tilemap(lib, hmax, tnum, xlo, xhi, tile_w, mask, ring_blocks, step_block, 1, 20)
    lists = gangmap(lib, SHAPES['config3'], 1, CHUNK)
    for x in range(8):
        assert lists[x] == [(c, int(t)) for c in range(len(hmax)) for t in m[c, :, x] if t >= 0]


def test_gang_size_rule(lib):
    """G = 0 asks for the rule: the chunk order keeps the tile map's (4 from 256 tiles); the packed order gangs where every XCD
    still gets 4 gangs per chunk.  Order -1 leaves the order to the launch too: packed where it gets gangs (from 128 tiles), the
    chunk order as it always was below (the blocks of many-rank plans measured no gain or a loss with the packed order)."""
    for name, G_packed in (('config3', 4), ('rank_block', 1), ('ragged', 1)):
        assert gangmap(lib, SHAPES[name], 0, PACKED) == gangmap(lib, SHAPES[name], G_packed, PACKED)
        assert gangmap(lib, SHAPES[name], 0, CHUNK) == gangmap(lib, SHAPES[name], 1, CHUNK)
        assert gangmap(lib, SHAPES[name], 0, -1) == (gangmap(lib, SHAPES[name], 4, PACKED) if name == 'config3' else gangmap(lib, SHAPES[name], 1, CHUNK))
    edge = list(SHAPES['config3'])
    for tiles, packed in ((127, False), (128, True)):
        edge[3] = tiles * 64
        assert (gangmap(lib, edge, 0, -1) == gangmap(lib, edge, 4, PACKED)) == packed
        assert gangmap(lib, edge, 0, -1) == (gangmap(lib, edge, 4, PACKED) if packed else gangmap(lib, edge, 1, CHUNK))


def replay(shape, lists, slots_per_xcd=64):
    """(idle share of the slot time up to the last item's end, when the first slot runs dry as a share of the span)."""
    pos = [0] * 8
    heap = [(0, s) for s in range(8 * slots_per_xcd)]       # (free at, slot); slot s runs on XCD s & 7
    heapq.heapify(heap)
    busy, end, first_dry = 0, 0, None
    while heap:
        t, s = heapq.heappop(heap)
        for v in range(8):
            x = ((s & 7) + v) & 7
            if pos[x] < len(lists[x]):
                c, tile = lists[x][pos[x]]
                pos[x] += 1
                w = tile_cost(shape, c, tile)
                busy += w
                end = max(end, t + w)
                heapq.heappush(heap, (t + w, s))
                break
        else:
            first_dry = t if first_dry is None else first_dry
    return 1.0 - busy / (8.0 * slots_per_xcd * end), first_dry / end


@pytest.mark.parametrize('name', list(SHAPES))
def test_packed_order_leaves_no_more_idle_time(lib, name):
    """By the cost model the packed order ends no later than the chunk order: at every G against the chunk order of that G, and
    against the chunk order as launches had it (no gangs at these tile counts)."""
    shape = SHAPES[name]
    old = replay(shape, gangmap(lib, shape, 1, CHUNK))[0]
    for G in (1, 2, 4):
        new, same_g = replay(shape, gangmap(lib, shape, G, PACKED))[0], replay(shape, gangmap(lib, shape, G, CHUNK))[0]
        print('%s G=%d: idle share packed %.4f, chunk %.4f (chunk, no gangs: %.4f)' % (name, G, new, same_g, old))
        assert new <= same_g + 1e-12 and new <= old + 1e-12
    if name == 'config3':
        assert abs(old - 0.045) < 0.005 and abs(replay(shape, gangmap(lib, shape, 1, PACKED))[0] - 0.033) < 0.005


def test_queue_policy_takes_only_its_values(monkeypatch):
    """impdar_kirch_queue_policy (the library reads no environment variable for the two settings; the Python side hands them
    over): orders 0..2 and gangs 0, 1, 2, 4, anything else is an argument error and changes nothing."""
    from impdar_amd import _hip
    lib = _hip.load()
    try:
        for order, gang, ok in ((2, 4, True), (1, 1, True), (0, 0, True), (3, 0, False), (-1, 0, False), (0, 3, False), (2, 8, False)):
            assert (lib.impdar_kirch_queue_policy(order, gang) == 0) == ok, (order, gang)
        for order, gang in (('packed', '2'), ('chunk', '4'), ('else', '3')):
            monkeypatch.setenv('IMPDAR_KIRCH_ORDER', order)
            monkeypatch.setenv('IMPDAR_KIRCH_G', gang)
            _hip.apply_queue_policy()            # (what is no value of a knob is the library's own choice, not an error)
    finally:
        lib.impdar_kirch_queue_policy(0, 0)
