"""The queue lists of the persistent Kirchhoff ring kernels on the GPU (kirch_gangmap, kirch_ring_queue_item): which workgroup
takes which (chunk, tile) item, on which XCD and when, changes no bit of the image.  IMPDAR_KIRCH_ORDER = chunk | packed and
IMPDAR_KIRCH_G = 1 | 2 | 4 are handed to the library when KirchhoffPlan creates the plan (impdar_kirch_queue_policy)."""
import numpy as np
import pytest

from conftest import rel_l2, rel_max
from test_kirchhoff_gpu import FAST_L2

pytestmark = pytest.mark.gpu

COMBOS = [(order, g) for order in ('chunk', 'packed') for g in ('1', '2', '4')]
KINDS = [(np.float32, 'fast', FAST_L2), (np.float64, 'exact', 1e-12)]


def _six_images(hip, monkeypatch, dtype, mode, snum, tnum, xlo, xhi, nranks=1, seed=47, t0_us=0.0):
    """The block [xlo, xhi) under the six settings, twice each; (images by setting, the radargram, its geometry)."""
    from impdar_amd import _hip, synth
    from impdar_amd.kirchhoff import KirchhoffPlan
    ctx = hip.context()
    geo = synth.geometry(snum, tnum, t0_us=t0_us)
    x = synth.noise_radargram(snum, tnum, seed=seed).astype(dtype)
    d_in = _hip.DeviceArray.from_host(ctx, x)
    outs = {}
    for order, g in COMBOS:
        monkeypatch.setenv('IMPDAR_KIRCH_ORDER', order)
        monkeypatch.setenv('IMPDAR_KIRCH_G', g)
        plan = KirchhoffPlan(ctx, dtype, snum, tnum, geo['dist'], geo['travel_time'], mode=mode, nranks=nranks)
        assert plan.kernel == ('kirch_quad_kernel' if dtype == np.float32 else 'kirch_dquad_kernel')
        plan.prep(d_in, tnum, 0, tnum)
        res = []
        for _ in range(2):
            d_out = _hip.DeviceArray(ctx, (snum, xhi - xlo), dtype)
            plan.migrate(d_out, xlo, xhi)
            plan.sync()
            res.append(d_out.to_host())
            d_out.free()
        plan.destroy()
        outs[order, g] = res
    d_in.free()
    return outs, x, geo


def _check(outs, x, geo, xlo, xhi, tol):
    from oracle import c_oracle
    first = outs[COMBOS[0]][0]
    for key in COMBOS:
        assert np.array_equal(outs[key][0], outs[key][1]), ('run to run', key)
        assert np.array_equal(outs[key][0], first), ('against chunk, G = 1', key)
    cols = np.unique(np.linspace(xlo, xhi - 1, 8).astype(int))
    want = c_oracle.kirchhoff(x, geo['travel_time'], geo['dist'], 1.69e8, False, traces=cols)
    err, emax = rel_l2(first[:, cols - xlo], want), rel_max(first[:, cols - xlo], want)
    print('against the oracle on %d columns: rel L2 %.3e, max %.3e (bar %.0e)' % (len(cols), err, emax, tol))
    # (float32: the bar is on the L2 norm; float64: on the largest difference too, as everywhere in the suite)
    assert err < tol and (first.dtype == np.float32 or emax < tol), (err, emax)


@pytest.mark.parametrize('dtype,mode,tol', KINDS)
def test_more_items_than_resident_workgroups(hip, monkeypatch, dtype, mode, tol):
    """520 samples (chunks of 256, 256 and 8) by 12800 traces: 600 items of two 32-trace tiles in float32 (walks of ~110 step
    blocks), more in float64 -- more than the 512 workgroups that are resident, so workgroups take several items and steal."""
    monkeypatch.setenv('IMPDAR_KIRCH_XB', '32')
    monkeypatch.setenv('IMPDAR_KIRCH_NH', '2')
    snum, tnum = 520, 12800
    outs, x, geo = _six_images(hip, monkeypatch, dtype, mode, snum, tnum, 0, tnum)
    _check(outs, x, geo, 0, tnum, tol)


@pytest.mark.parametrize('dtype,mode,tol', KINDS)
def test_an_output_block_without_the_queue(hip, monkeypatch, dtype, mode, tol):
    """Output traces [13, 141) of a 300-trace profile: fewer items than workgroup slots, one item per block, no queue."""
    monkeypatch.setenv('IMPDAR_KIRCH_XB', '32')
    monkeypatch.setenv('IMPDAR_KIRCH_NH', '2')
    outs, x, geo = _six_images(hip, monkeypatch, dtype, mode, 520, 300, 13, 141)
    _check(outs, x, geo, 13, 141, tol)


@pytest.mark.parametrize('dtype,mode,tol', KINDS)
def test_walk_pieces_of_a_four_rank_plan(hip, monkeypatch, dtype, mode, tol):
    """A 4-rank plan hands every walk out as two queue items with partial images of their own (kirch_ring_walk): the queue is
    used at any item count, and the piece comes from the counter, not from the list."""
    for k in ('IMPDAR_KIRCH_PARTS', 'IMPDAR_KIRCH_XB', 'IMPDAR_KIRCH_NH'):
        monkeypatch.delenv(k, raising=False)
    snum, tnum = 1300, 341
    outs, x, geo = _six_images(hip, monkeypatch, dtype, mode, snum, tnum, 0, tnum, nranks=4, seed=43, t0_us=-0.02)
    _check(outs, x, geo, 0, tnum, tol)
