"""The host-side planners of the phase shift's path runners (csrc/ps_path_plan.h, compiled here by itself with g++: no GPU, no
HIP -- the compile is the check that the header is host-only): runs of constant velocity -> the pieces of the transform path
(pn_plan), the runs and stages of the many-runs matrix-core path (pr_plan), the row blocks of the matrix-core path (pm_plan), with
every rule by which a path declines.  (a) Each plan is held, field by field and bit by bit, to what the planning code produced
while it still lived inside the runners of phaseshift.hip (tests/ps_path_plan_recorded.json: a digest per plan, made from those blocks
copied verbatim into a scratch program at the commit before they moved); (b) the invariants the kernels rely on, on the same cases and
on seeded random run lists; (c) the window's correction table against the scheme test's own quadrature."""
import json
import random

import numpy as np
import pytest

import ps_path_plan_cases as PP
from test_nufft_scheme import correction


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return PP.probe(str(tmp_path_factory.mktemp('pspathplan')))


@pytest.fixture(scope='module')
def recorded():
    with open(PP.RECORDED) as f:
        return json.load(f)


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == PP.IDS
    taken = {p: sum(r[p] is not None for r in recorded.values()) for p in ('pn', 'pr', 'pm')}
    assert all(0 < n < len(PP.IDS) for n in taken.values()), taken           # every planner both takes and declines


@pytest.mark.parametrize('name', PP.IDS)
def test_plans_are_those_of_the_runners_before_the_split(lib, recorded, name):
    got, want = PP.plans(lib, PP.CASES[name]), recorded[name]
    for p in ('pn', 'pr', 'pm'):
        assert PP.digest(got[p]) == want[p], (p, got[p])          # (the digest covers every field: see ps_path_plan_cases.digest)


def check_invariants(c, plans):
    runs = PP.runs_of(c)
    end = runs[-1][0] + runs[-1][1]                  # the last finite step + 1
    vz = c['vz']
    pn, pr, pm = plans['pn'], plans['pr'], plans['pm']
    if pn is not None:
        lmax = (2048 if c['pairs'] else 1024) if c['dtype'] == 'float64' else 4096
        at, logs = 0, set()
        for start, length, kind, loglp, _v, _vs in pn['pieces']:
            assert start == at and length >= 1
            at += length
            if kind == 0:
                assert length <= lmax
                assert loglp >= 4 and (1 << loglp) >= length and (loglp == 4 or (1 << (loglp - 1)) < length)
                logs.add(loglp)
            else:
                assert kind == 1 and vz and length <= PP.PN_SHORT
        assert at == end
        assert pn['need'] == sorted(logs)
        assert pn['gmax'] == 2 << max(logs | {4})
        assert pn['nshort_steps'] == sum(p[1] for p in pn['pieces'] if p[2] == 1) <= 128 and len(pn['pieces']) <= 256
        assert pn['e1_len'] == (c['snum'] if c['dtype'] == 'float64' and vz else 0)
    if pr is not None:
        at = 0
        for start, length, kind, _slot, _v in pr['runs']:
            assert start == at and 1 <= length <= (PP.PR_LONG_MAX if kind == 0 else PP.PR_SHORT_LEN)
            at += length
        assert at == end
        assert pr['nparts'] == -(-c['nf'] // PP.PR_PART)
        nxt = 0
        for st in pr['stages']:
            run0, nruns, nshort, short_wave = st[:4]
            long_run, long_nblk, short_tau = st[4:8], st[8:12], st[12:24]
            assert run0 == nxt and 1 <= nruns <= PP.PR_STAGE_RUNS             # every run in one stage, in order
            nxt += nruns
            mine = pr['runs'][run0:run0 + nruns]
            longs = [run0 + i for i, r in enumerate(mine) if r[2] == 0]
            assert len(longs) <= PP.PR_LONGS and long_run == longs + [-1] * (PP.PR_LONGS - len(longs))
            assert [pr['runs'][i][3] for i in longs] == list(range(len(longs)))
            nblk = [-(-(-(-pr['runs'][i][1] // PP.PR_TT)) // PP.PR_ROWS) for i in longs]
            assert long_nblk == nblk + [0] * (PP.PR_LONGS - len(longs)) and all(1 <= n <= 4 for n in nblk)
            taus, rows = [], []
            for r in mine:
                if r[2] == 1:
                    rows.append(len(taus))
                    taus += list(range(r[0], r[0] + r[1]))
            assert nshort == len(taus) <= PP.PR_SROWS and short_tau[:nshort] == taus
            assert [r[3] for r in mine if r[2] == 1] == rows
            assert short_wave == long_nblk.index(min(long_nblk))             # the first wave with the fewest blocks
        assert nxt == len(pr['runs'])
    if pm is not None:
        long_runs = [i for i, (_s, n) in enumerate(runs) if not (vz and n <= PP.PM_SHORT)]
        assert pm['nlong'] == len(long_runs) <= 16 and len(runs) <= PP.PM_MAX_RUNS
        assert pm['long_of'] == [long_runs.index(i) if i in long_runs else -1 for i in range(long_runs[-1] + 1)]
        blocks = []
        for g in range(pm['ngroups']):
            grp = pm['table'][g * PP.PM_NRB:(g + 1) * PP.PM_NRB]
            n = sum(b[0] >= 0 for b in grp)
            assert 1 <= n <= PP.PM_NRB and all(b == [-1, 0] for b in grp[n:])
            blocks += grp[:n]
        assert blocks == [[i, a0] for i in long_runs for a0 in range(0, -(-runs[i][1] // 64), 32)]      # every tile of every long run, in blocks of 32


@pytest.mark.parametrize('name', PP.IDS)
def test_invariants_of_the_recorded_cases(lib, name):
    c = PP.CASES[name]
    check_invariants(c, PP.plans(lib, c))


def test_invariants_of_random_run_lists(lib):
    rnd = random.Random(20251019)
    taken = dict(pn=0, pr=0, pm=0)
    for it in range(300):
        lens = []
        for _ in range(rnd.choice((1, 2, 3, 5, 9, 17, 40, 90, 120))):
            lens.append(rnd.choice((1, 1, 2, 3, 8, 9, 60, 64, 65, 127, 128, 129, 500, 512, 513, 700, 1024, 1025, 2100, 4100)))
        if sum(lens) > 12000:
            lens = lens[:1 + len(lens) // 8]
        v = PP.steps(lens)
        if it % 10 == 9:
            v[rnd.randrange(len(v))] = rnd.choice((np.nan, np.inf, 0.0))
        for dtype, pairs in (('float32', 0), ('float64', it % 2)):
            c = dict(dtype=dtype, pairs=pairs, nf=rnd.choice((64, 256, 1024, 2080, 4096, 6144)), herm=1, vel=v, vz=1, snum=len(v))
            plans = PP.plans(lib, c)
            check_invariants(c, plans)
            for p in taken:
                taken[p] += plans[p] is not None
    assert all(n >= 20 for n in taken.values()), taken


# Largest relative difference measured with the real function over l = 4 .. 12: 2.62e-15 at W = 8, 3.39e-15 at W = 14 (the
# rounding of the rotation recurrence between its re-seeds; the test prints it).  The bar is ten times the larger, far below the
# 5e-12 bar of the scheme at W = 14.
CORR_BAR = 3.4e-14


@pytest.mark.parametrize('W', [8, 14])
def test_correction_table_against_the_scheme(lib, W):
    worst = 0.0
    for l in range(4, 13):
        lp = 1 << l
        got, want = PP.corr(lib, W, l), correction(lp, W)                    # n = 0 .. lp/2; n = -lp/2 .. lp/2 - 1
        ref = np.concatenate([want[lp // 2:], want[:1]])                     # (psihat is even: n = lp/2 from n = -lp/2)
        worst = max(worst, float(np.max(np.abs(got - ref) / np.abs(ref))))
    print('W = %d: largest relative difference %.2e' % (W, worst))
    assert worst < CORR_BAR
