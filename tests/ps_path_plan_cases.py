"""The cases of the phase shift's path planners (test infrastructure of tests/test_ps_path_plan.py): velocity profiles that reach
every cut, merge, packing and decline rule of csrc/ps_path_plan.h, the probe of that header compiled by itself, and each plan as
plain data.  What the planning code inside the path runners produced for each case at the commit before it moved into the header
is in tests/ps_path_plan_recorded.json: per plan what it counts and a SHA-256 over every field of it (integers as they are, doubles
as float.hex(), the first-order table as the SHA-256 of its bytes) -- equal digests are equal plans, bit for bit."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

from ps_route_cases import DT, velocity

RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ps_path_plan_recorded.json')
PN_SHORT, PM_SHORT, PM_NRB, PM_MAX_RUNS = 8, 8, 5, 96
PR_TT, PR_ROWS, PR_LONGS, PR_LONG_MAX, PR_SHORT_LEN, PR_SROWS, PR_STAGE_RUNS, PR_PART = 8, 16, 4, 512, 2, 12, 16, 1024


def steps(lens, v0=1.6e8, dv=0.01e8):
    """A profile whose runs of constant velocity have these lengths: run r at v0 + dv (r % 40) -- neighbours always differ."""
    return np.ascontiguousarray(np.concatenate([np.full(n, v0 + dv * (r % 40)) for r, n in enumerate(lens)]))


def layer_table(kind, snum, dt=DT):
    """The (v, z) tables of test_many_runs_matrix_core_path_..., as the per-step profile getVelocityProfile makes of them."""
    from oracle import mig_oracle
    tt_us = np.arange(snum) * dt * 1.0e6
    Rp = 1.9e8 * tt_us[-1] * 1e-6 / 2.
    lin = lambda n, v0, v1: np.stack([np.linspace(v0, v1, n), np.linspace(0., 1.3 * Rp, n)], axis=1)
    tab = {'layers13': lin(13, 1.69e8, 2.1e8), 'layers40': lin(40, 1.68e8, 1.9e8),
           'uneven': np.array([[1.6e8, 0.], [1.6e8, 0.02 * Rp], [1.66e8, 0.05 * Rp], [1.75e8, 0.61 * Rp], [1.78e8, 0.63 * Rp],
                               [1.82e8, 0.83 * Rp], [1.86e8, 0.9 * Rp], [1.9e8, 1.3 * Rp]]),
           'boundary': np.concatenate([[[1.68e8, 0.]], lin(9, 1.68e8, 1.95e8) + [[0., 0.3 * Rp]] * 9])[:, :],
           'thick': np.array([[1.69e8, 0.], [1.69e8, 0.5 * Rp], [1.9e8, 1.3 * Rp]])}[kind]
    return np.ascontiguousarray(mig_oracle.get_velocity_profile(tt_us, tab), dtype=np.float64)


def noisy(lens):
    """Runs that carry ~4e-13 of relative noise (what 2 * gradient(z(t)) leaves inside a layer): below the cut at 1e-11, so the
    runs stay whole and the float64 transform path takes the noise as its first-order term.  Integer arithmetic: the same bits anywhere."""
    v = steps(lens)
    i = np.arange(len(v), dtype=np.int64)
    return np.ascontiguousarray(v * (1.0 + 4e-13 * (((i * 2654435761) % 1024 - 512) / 512.0)))


def _cut(v, at, value):
    v = v.copy()
    v[at] = value
    return v


def _cases():
    out = {}

    def add(name, vel, nf=1024, dtypes=('float32', 'float64'), herm=1):
        v = vel() if callable(vel) else vel
        for dtype in dtypes:
            for pairs in ((0, 1) if dtype == 'float64' else (0,)):         # (pairs change the piece length of float64 only)
                out['%s-%s-p%d' % (name, dtype, pairs)] = dict(dtype=dtype, pairs=pairs, nf=nf, herm=herm, vel=v, vz=1, snum=len(v))

    def const(name, snum, nf=1024):
        for dtype in ('float32', 'float64'):
            for pairs in ((0, 1) if dtype == 'float64' else (0,)):
                out['%s-%s-p%d' % (name, dtype, pairs)] = dict(dtype=dtype, pairs=pairs, nf=nf, herm=1, vel=1.69e8, vz=0, snum=snum)

    for snum in (64, 1024, 1025, 2048, 2049, 4096, 4097, 8192):               # the piece cuts at 1024, 2048 and 4096
        const('const-s%d' % snum, snum)
    for kind in ('tab3', 'tab6', 'many', 'gradient'):
        for snum in (128, 520, 2100, 4200):
            add('%s-s%d' % (kind, snum), velocity(kind, snum))
    for kind in ('layers13', 'layers40', 'uneven', 'boundary', 'thick'):
        for snum in (520, 2100):
            add('%s-s%d' % (kind, snum), layer_table(kind, snum))
    add('noise', noisy([700, 3, 1500, 4, 2300]), dtypes=('float64',))
    # short runs: a boundary smeared over n single steps between long runs; two boundaries back to back (the merge up to PN_SHORT steps)
    for n in (1, 2, 3, 8, 9):
        add('smear%d' % n, steps([300] + [1] * n + [300]))
    add('merge-3+3', steps([300, 3, 3, 300]))
    add('merge-4+4', steps([300, 4, 4, 300]))
    add('merge-5+5', steps([300, 5, 5, 300]))
    add('merge-1x5+4', steps([300] + [1] * 5 + [4, 300]))
    # decline edges, one case each side
    for n in (128, 129):
        add('pn-short%d' % n, steps([200] + [1] * n + [200]))
    for n in (256, 257):
        add('pn-pieces%d' % n, steps([9] * n))
    add('pr-quarter', steps([1] * 100 + [300]))                               # nshort_total == snum / 4
    add('pr-quarter+1', steps([1] * 101 + [299]))
    add('pr-noblocks', _cut(steps([1, 1, 200]), 2, np.nan))                   # the runs end at the step that is not finite: single steps only
    add('pr-blocks', _cut(steps([1, 200, 100]), 201, np.inf))
    for n in (16, 17):
        add('pm-long%d' % n, steps([700] * n))
    add('pm-short200', steps([1100] + [8] * 25 + [1100]))
    add('pm-short201', steps([1100] + [8] * 25 + [1, 1100]))
    add('pm-pad-at', steps([512] * 4))                                        # 4 x 2048 == 3 snum + 2048
    add('pm-pad-over', steps([512, 512, 512, 511]))
    for n in (96, 97):
        add('pm-runs%d' % n, steps([300] + [1] * (n - 2) + [300]))
    for nf in (32, 63, 64, 224, 255, 256, 4096, 4128, 6144, 6176):
        const('nf%d' % nf, 512, nf=nf)
        add('nf%d-tab' % nf, steps([250, 3, 259]), nf=nf)
    for snum in (63, 64, 255, 256):
        const('snum%d' % snum, snum)
        add('snum%d-tab' % snum, steps([snum // 2, snum - snum // 2]))
    add('complex-walk', steps([300, 300]), herm=0)
    # stage packing of the many-runs path
    for n in (4, 5):
        add('stage-long%d' % n, steps([100] * n))
    for n in (12, 13):
        add('stage-rows%d' % n, steps([1] * n + [100]))
    add('stage-rows-2s', steps([2] * 6 + [100, 2, 100]))
    add('stage-runs16', steps([1, 1, 1, 100] * 4))
    add('stage-runs17', steps([1, 1, 1, 100] * 4 + [1, 1, 1, 100]))
    for n in (512, 513, 1024, 1025):
        add('long%d' % n, steps([n, 100]))
    return out


CASES = _cases()
IDS = sorted(CASES)


def probe(tmpdir):
    """csrc/ps_path_plan.h compiled by itself with g++: the header needs nothing of HIP."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, lib = os.path.join(tmpdir, 'ps_path_plan_probe.cpp'), os.path.join(tmpdir, 'libpspathplan.so')
    with open(src, 'w') as f:
        f.write('#define PS_PATH_PLAN_PROBE 1\n#include "ps_path_plan.h"\n')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(root, 'impdar_amd', 'csrc'), src, '-o', lib])
    return C.CDLL(lib)


def _hex(a):
    return [float(x).hex() for x in a]


def plans(lib, c):
    """The three plans of a case as plain data: None where the planner declines."""
    dbl, snum, nf, vel = int(c['dtype'] == 'float64'), c['snum'], c['nf'], c['vel']
    vm = None if np.ndim(vel) == 0 else np.ascontiguousarray(vel, dtype=np.float64)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    vc, vp = C.c_double(0.0 if vm is not None else float(vel)), vm.ctypes.data_as(dp) if vm is not None else None
    cap = snum + 16
    out = {}
    ints, pi, pv, pvs, e1 = np.zeros(8, np.int32), np.zeros(4 * cap, np.int32), np.zeros(cap), np.zeros(PN_SHORT * cap), np.zeros(snum)
    rc = lib.impdar_pn_plan_probe(dbl, snum, nf, c['pairs'], c['vz'], c['herm'], vc, vp, cap, ints.ctypes.data_as(ip), pi.ctypes.data_as(ip),
                                  pv.ctypes.data_as(dp), pvs.ctypes.data_as(dp), e1.ctypes.data_as(dp))
    assert rc == 0, rc
    out['pn'] = None
    if ints[0]:
        n, ne = int(ints[1]), int(ints[5])
        pieces = []
        for i in range(n):
            vs = pvs[PN_SHORT * i:PN_SHORT * (i + 1)]
            assert pi[4 * i + 2] == 1 or not vs.any()              # (a transform piece has no step velocities)
            pieces.append([int(x) for x in pi[4 * i:4 * i + 4]] + [float(pv[i]).hex()] + [_hex(vs) if pi[4 * i + 2] == 1 else []])
        out['pn'] = dict(pieces=pieces, nshort_steps=int(ints[2]), gmax=int(ints[3]), need=[l for l in range(13) if ints[4] >> l & 1],
                         e1_len=ne, e1_sha256=hashlib.sha256(e1[:ne].tobytes()).hexdigest() if ne else None,
                         e1_absmax=float(np.abs(e1[:ne]).max()).hex() if ne else None)
    ints, ri, rv, si = np.zeros(4, np.int32), np.zeros(4 * cap, np.int32), np.zeros(cap), np.zeros(24 * cap, np.int32)
    rc = lib.impdar_pr_plan_probe(dbl, snum, nf, vc, vp, cap, ints.ctypes.data_as(ip), ri.ctypes.data_as(ip), rv.ctypes.data_as(dp), si.ctypes.data_as(ip))
    assert rc == 0, rc
    out['pr'] = None
    if ints[0]:
        n, ns = int(ints[1]), int(ints[2])
        out['pr'] = dict(runs=[[int(x) for x in ri[4 * i:4 * i + 4]] + [float(rv[i]).hex()] for i in range(n)],
                         stages=[[int(x) for x in si[24 * i:24 * i + 24]] for i in range(ns)], nparts=int(ints[3]))
    ints, tab, lo = np.zeros(3, np.int32), np.zeros(2 * cap, np.int32), np.zeros(PM_MAX_RUNS, np.int32)
    rc = lib.impdar_pm_plan_probe(dbl, snum, nf, c['vz'], vc, vp, cap, ints.ctypes.data_as(ip), tab.ctypes.data_as(ip), lo.ctypes.data_as(ip))
    assert rc == 0, rc
    out['pm'] = None
    if ints[0]:
        ng = int(ints[1])
        out['pm'] = dict(ngroups=ng, nlong=int(ints[2]), table=[[int(tab[2 * i]), int(tab[2 * i + 1])] for i in range(ng * PM_NRB)],
                         long_of=[int(x) for x in lo[:max(np.flatnonzero(lo >= 0)) + 1]])      # (-1 from there on)
    return out


def runs_of(c):
    """ps_route_runs in NumPy: (start, len) of the runs of a case's profile, cut at the first velocity that is not finite."""
    v, snum = c['vel'], c['snum']
    if np.ndim(v) == 0:
        return [(0, snum)]
    vtol = 1e-11 if c['dtype'] == 'float64' else 1e-10
    runs, vrun = [], -1.0
    for i in range(snum):
        if i == 0 or abs(v[i] - vrun) > vtol * abs(v[i]):
            runs.append([i, 0])
            vrun = v[i]
        runs[-1][1] += 1
        if not (np.isfinite(v[i]) and v[i] != 0.0):
            break
    return [tuple(r) for r in runs]


def corr(lib, W, l):
    out = np.zeros((1 << l) // 2 + 1)
    n = lib.impdar_pn_corr_probe(W, l, out.ctypes.data_as(C.POINTER(C.c_double)))
    assert n == len(out)
    return out


def digest(plan):
    """A plan as it is recorded: what it counts (gmax, nshort_steps, pieces / nparts, runs, stages / ngroups, nlong), then the SHA-256
    (first 16 hex digits) of all of its fields as JSON."""
    if plan is None:
        return None
    counts = [len(v) if isinstance(v, list) else v for k, v in sorted(plan.items()) if k in ('pieces', 'nshort_steps', 'gmax', 'runs', 'stages', 'nparts', 'ngroups', 'nlong')]
    return counts + [hashlib.sha256(json.dumps(plan, sort_keys=True, separators=(',', ':')).encode()).hexdigest()[:16]]


def record(lib, path=RECORDED):
    with open(path, 'w') as f:
        f.write('{\n' + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps({p: digest(v) for p, v in plans(lib, CASES[k]).items()}, sort_keys=True, separators=(',', ':')))
                                   for k in IDS) + '\n}\n')
