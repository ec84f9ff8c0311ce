"""The gpu cases of tests/kirch_route_cases.py through the C ABI: the plan reports what the host-only route (csrc/kirch_route.h,
through its probe) says and what the library reported at the commit before the route was split out
(tests/kirch_route_recorded.json), and one prep + migrate of each meets the suite's bars against the C oracle."""
import json

import numpy as np
import pytest

import kirch_route_cases as KC
from conftest import rel_l2, rel_max
from test_kirchhoff_gpu import EXACT_TOL, FAST_L2, FAST_MAX

pytestmark = pytest.mark.gpu

NAMES = {'kirch_exact_kernel': 'EXACT_PAIR', 'kirch_exact_tab_kernel': 'EXACT_TAB', 'kirch_dquad_kernel': 'DQUAD', 'kirch_quad_kernel': 'QUAD',
         'kirch_tab_kernel': 'TAB', 'kirch_gen_kernel': 'GEN'}
MODES = {'auto': KC.AUTO, 'exact': KC.EXACT, 'fast': KC.FAST}


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
    return KC.probe(str(tmp_path_factory.mktemp('kirchroute')))


@pytest.fixture(scope='module')
def recorded():
    with open(KC.RECORDED) as f:
        return json.load(f)['cases']


@pytest.mark.parametrize('c', KC.GPU_CASES, ids=[c['id'] for c in KC.GPU_CASES])
def test_plan_follows_the_route(hip, monkeypatch, probe, recorded, c):
    from oracle import c_oracle
    assert c['snum'] <= 300 and (96 <= c['tnum'] <= 512 or (c['snum'], c['tnum']) == (64, 8192))
    rep, x, img = KC.run(hip, c, monkeypatch)
    got = (NAMES[rep['kernel']], MODES[rep['mode']], rep['tnum_pad'], rep['xnoise'])
    r, m = KC.route(probe, c, ties=0), recorded[c['id']]
    assert got == (r['kernel'], r['mode'], r['tnum_pad'], r['xnoise'])
    assert got == (m['kernel'], m['mode'], m['tnum_pad'], m['xnoise'])
    dist, tt = KC.axes(c)
    want = c_oracle.kirchhoff(x, tt * 1.0e6, dist / 1.0e3, KC.VEL, bool(c['nearfield']))
    if c['dtype'] == 'float32':
        assert rel_l2(img, want) < FAST_L2 and rel_max(img, want) < FAST_MAX, (rel_l2(img, want), rel_max(img, want))
    else:
        assert rel_max(img, want) < EXACT_TOL, rel_max(img, want)


def test_plan_keeps_the_knobs_it_was_created_under(hip, monkeypatch):
    """A plan runs under the IMPDAR_KIRCH_EXACT_IMPL it was created under -- the value its tie list was built, or not built,
    for -- whatever the environment says at migrate."""
    from impdar_amd.kirchhoff import KirchhoffPlan
    c = KC.CASES[KC.IDS.index('f64-EXACT_IMPL=pair')]
    dist, tt = KC.axes(c)
    for k in KC.KNOBS:
        monkeypatch.delenv('IMPDAR_KIRCH_' + k, raising=False)
    ctx = hip.context()
    x = np.random.default_rng(1).standard_normal((c['snum'], c['tnum']))
    d_in, d_out = hip.DeviceArray.from_host(ctx, x), hip.DeviceArray(ctx, x.shape, x.dtype)
    imgs = {}
    for created, run in (('pair', None), ('pair', 'pair'), (None, 'pair')):
        if created:
            monkeypatch.setenv('IMPDAR_KIRCH_EXACT_IMPL', created)
        else:
            monkeypatch.delenv('IMPDAR_KIRCH_EXACT_IMPL', raising=False)
        plan = KirchhoffPlan(ctx, x.dtype, c['snum'], c['tnum'], dist / 1.0e3, tt * 1.0e6, KC.VEL, False, 'exact')
        if run:
            monkeypatch.setenv('IMPDAR_KIRCH_EXACT_IMPL', run)
        else:
            monkeypatch.delenv('IMPDAR_KIRCH_EXACT_IMPL', raising=False)
        assert plan.lib.impdar_kirch_plan_kernel(plan.h) == (0 if created else 2)        # EXACT_PAIR / DQUAD, as at creation
        plan.prep(d_in, c['tnum'], 0, c['tnum'])
        plan.migrate(d_out, 0, c['tnum'])
        plan.sync()
        imgs[(created, run)] = d_out.to_host()
        plan.destroy()
    d_in.free()
    d_out.free()
    assert np.array_equal(imgs[('pair', None)], imgs[('pair', 'pair')])
    assert rel_max(imgs[(None, 'pair')], imgs[('pair', 'pair')]) < EXACT_TOL
