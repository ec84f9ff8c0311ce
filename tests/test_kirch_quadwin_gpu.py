"""The quad-aligned output window of kirch_quad_kernel on the GPU (IMPDAR_KIRCH_WINDOW = slide | quad, handed to the library
when KirchhoffPlan creates the plan: impdar_kirch_window_policy).  Under `quad` a tile reads whole LDS quads only and the three
columns left of every tile start are the sum of two tiles' partial sums (kirch_fixup_kernel): those columns differ from the
sliding window's by float32 rounding -- their judge is the float64 oracle -- and no other bit of the image moves."""
import numpy as np
import pytest

from conftest import rel_l2, rel_max
from test_kirchhoff_gpu import FAST_L2

pytestmark = pytest.mark.gpu

DX = 0.9        # 1.07 samples of moveout per trace: every instantiation below holds the window's 3 further traces in the ring rows it has
# (XB, NH, LK) the library has a far-field instantiation for
COMBOS = [(24, 1, 0), (32, 1, 0), (40, 1, 0), (32, 2, 0), (40, 2, 0), (40, 2, 1), (40, 3, 0), (40, 3, 1)]
# snum, tnum, xlo, xhi, nranks
SHAPES = {
    'block-13-141': (520, 300, 13, 141, 1),            # fewer items than workgroup slots: one item per block, no queue
    'full-128': (520, 128, 0, 128, 1),                 # the block ends on a tile start of the 32- and 64-trace tiles: the tile right of it only holds side sums
    'full-64': (520, 64, 0, 64, 1),
    'block-0-64': (520, 300, 0, 64, 1),                # ... over real neighbouring traces
    'queue-12800': (520, 12800, 0, 12800, 1),          # more items than resident workgroups: the ring image persists across items
    'pieces-341': (1300, 341, 0, 341, 4),              # a 4-rank plan: every walk as two queue items with side sums of their own
}
CASES = [(name, c) for name in SHAPES for c in COMBOS if SHAPES[name][4] == 1 or c[1] == 1]

_inputs = {}


def _input(name):
    """The noise radargram and the geometry of a shape, made once."""
    if name not in _inputs:
        from impdar_amd import synth
        snum, tnum = SHAPES[name][:2]
        _inputs[name] = (synth.noise_radargram(snum, tnum, seed=59).astype(np.float32), synth.geometry(snum, tnum, dx=DX, t0_us=-0.02 if snum > 1000 else 0.0))
    return _inputs[name]


def _images(hip, monkeypatch, name, window):
    from impdar_amd import _hip
    from impdar_amd.kirchhoff import KirchhoffPlan
    snum, tnum, xlo, xhi, nranks = SHAPES[name]
    x, geo = _input(name)
    ctx = hip.context()
    monkeypatch.setenv('IMPDAR_KIRCH_WINDOW', window)
    plan = KirchhoffPlan(ctx, np.float32, snum, tnum, geo['dist'], geo['travel_time'], mode='fast', nranks=nranks)
    assert plan.kernel == 'kirch_quad_kernel' and plan.window == window, (plan.kernel, plan.window)
    d_in = _hip.DeviceArray.from_host(ctx, x)
    plan.prep(d_in, tnum, 0, tnum)
    res = []
    for _ in range(2):
        d_out = _hip.DeviceArray(ctx, (snum, xhi - xlo), np.float32)
        plan.migrate(d_out, xlo, xhi)
        plan.sync()
        res.append(d_out.to_host())
        d_out.free()
    plan.destroy()
    d_in.free()
    return res


@pytest.mark.parametrize('name,combo', CASES, ids=['%s-xb%d-nh%d-lk%d' % ((n,) + c) for n, c in CASES])
def test_quad_window_against_the_sliding_one_and_the_oracle(hip, monkeypatch, name, combo):
    from oracle import c_oracle
    xb, nh, lk = combo
    snum, tnum, xlo, xhi, nranks = SHAPES[name]
    monkeypatch.setenv('IMPDAR_KIRCH_XB', str(xb))
    monkeypatch.setenv('IMPDAR_KIRCH_NH', str(nh))
    monkeypatch.setenv('IMPDAR_KIRCH_LK', str(lk))
    slide = _images(hip, monkeypatch, name, 'slide')
    quad = _images(hip, monkeypatch, name, 'quad')
    assert np.array_equal(slide[0], slide[1]) and np.array_equal(quad[0], quad[1])       # run to run
    # tiles start at multiples of XB from trace 0: the three columns left of each are two tiles' sums
    cols_all = np.arange(xlo, xhi)
    boundary = cols_all % xb >= xb - 3
    assert boundary.any() and np.array_equal(quad[0][:, ~boundary], slide[0][:, ~boundary])
    # the oracle on a tile start's neighbourhood (the three shared columns, and the whole columns on both sides of them and of
    # the start), on the block's last three columns (shared ones where the block ends on a tile start) and across the block
    edge = (xlo + 4 + xb - 1) // xb * xb
    assert edge + 1 < xhi
    cols = np.unique(np.concatenate([np.arange(edge - 4, edge + 2), np.arange(xhi - 3, xhi), np.linspace(xlo, xhi - 1, 5).astype(int)]))
    assert len(cols) >= 8 and np.sum(cols % xb >= xb - 3) >= 3
    x, geo = _input(name)
    want = c_oracle.kirchhoff(x, geo['travel_time'], geo['dist'], 1.69e8, False, traces=cols)
    bnd = cols % xb >= xb - 3
    for label, img in (('quad', quad[0]), ('slide', slide[0])):
        got = img[:, cols - xlo]
        print('%s %s: rel L2 against the oracle on %d columns %.3e; on the %d shared columns %.3e (max %.3e), on the others %.3e'
              % (name, label, len(cols), rel_l2(got, want), bnd.sum(), rel_l2(got[:, bnd], want[:, bnd]), rel_max(got[:, bnd], want[:, bnd]),
                 rel_l2(got[:, ~bnd], want[:, ~bnd])))
    got = quad[0][:, cols - xlo]
    assert rel_l2(got, want) < FAST_L2 and rel_l2(got[:, bnd], want[:, bnd]) < FAST_L2, (rel_l2(got, want), rel_l2(got[:, bnd], want[:, bnd]))


def test_window_policy_takes_only_its_values(hip):
    lib = hip.load()
    try:
        for w in range(-1, 5):
            assert (lib.impdar_kirch_window_policy(w) == 0) == (w in (0, 1, 2)), w
    finally:
        lib.impdar_kirch_window_policy(0)
