"""The host-side route of the phase shift (csrc/ps_route.h, compiled here by itself with g++: no GPU, no HIP): the Hermitian
verdict, the runs of constant velocity, which layout of the spectrum, the ORDER in which the frequency-sum kernels are tried,
and the launch order of the runs kernels.  The expected values were read off ps_run as it stood before the route was split out
of it (a NumPy restatement of its run rule and its estimate is below); what that build reported on the GPU for the cases of
tests/ps_route_cases.py is in tests/ps_route_recorded.json, and the route is held to it here."""
import json
import os

import numpy as np
import pytest

import ps_route_cases as PC

SNUM, TNUM, NT, DT = 128, 64, 256, PC.DT
F32, F64 = np.float32, np.float64


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return PC.probe(str(tmp_path_factory.mktemp('psroute')))


def layers(lens, v0=1.69e8, dv=0.1e8):
    return np.concatenate([np.full(n, v0 + dv * i) for i, n in enumerate(lens)])


GRADIENT = 1.69e8 + 0.5e8 * np.linspace(0., 1., SNUM)
THREE, FOUR = layers([40, 40, 48]), layers([32, 32, 32, 32])
MANY = np.concatenate([1.69e8 + 0.4e8 * np.arange(70) / 70., np.full(256 - 70, 1.69e8 + 0.4e8 * 69 / 70.)])      # 70 runs in 256 steps


def model(v, dbl, nf):
    """ps_run's own rules, restated: the runs (a step starts one when it differs from the run's first by more than vtol), whether
    the schedule is used (share of 16-step tiles that hold a start), the long runs (> 8 steps) and the float32 estimate."""
    vtol, starts, vrun = (1e-11 if dbl else 1e-10), [], None
    for i, x in enumerate(v):
        if i == 0 or abs(x - vrun) > vtol * abs(x):
            starts.append(i)
            vrun = x
    lens = np.diff(starts + [len(v)])
    ntile = (len(v) + 15) // 16
    sched = len(set(s // 16 for s in starts)) <= (0.9 if dbl else 0.5) * ntile or len(v) <= 64
    lmax = 2048 if dbl else 4096
    pieces, nshort, fq = sum(-(-n // lmax) for n in lens if n > 8), sum(n for n in lens if n <= 8), nf / 4096.
    nlong = int((lens > 8).sum())
    first = nlong <= (24 if nf >= 2048 else 16) if dbl else \
        nshort <= 128 and (0.135 + 0.06 * fq) * (pieces + nshort / 3.) <= 1.2 + 8.5 * fq * (len(v) / 8192.) + 0.05 * len(lens) * fq
    return dict(runs=len(lens), long_runs=nlong, use_sched=bool(sched), nufft_first=bool(first))


def go(lib, dtype, vel, snum=SNUM, tnum=TNUM, nt=NT, kx=None, ws=None, **kw):
    kx0, ws0 = PC.axes(tnum, nt)
    return PC.route(lib, dtype, snum, kx0 if kx is None else kx, ws0 if ws is None else ws, vel, **kw)


def test_hermitian_verdict(lib):
    kx, ws = PC.axes(TNUM, NT)
    for dtype, vel in ((F32, 1.69e8), (F64, THREE)):
        r = go(lib, dtype, vel)
        assert r['herm'] and (r['nf'], r['fstride'], r['k_zero']) == (NT // 2, NT // 2 + 1, [0])
        assert r['w'][0] == ws[NT // 2] and np.array_equal(r['w'][1:], ws[1:NT // 2])          # slot order: Nyquist in slot 0

    def off(**kw):
        r = go(lib, F32, kw.pop('vel', 1.69e8), **kw)
        assert not r['herm'] and (r['nf'], r['fstride']) == (len(r['w']), len(r['w'])) and not r['half_front'] and not r['use_own']
        return r
    assert off(nt=192)['nf'] == 192                                                        # not a power of two
    for i, x in ((0, 1.0), (NT - 5, ws[NT - 5] * (1 + 1e-15))):                             # ws[0] != 0; one ws[nt - i] != -ws[i]
        w2 = ws.copy()
        w2[i] = x
        assert off(ws=w2)['nf'] == NT
    k2 = kx.copy()
    k2[TNUM - 3] *= 1 + 1e-15                                                               # one kx[tnum - k] != -kx[k]
    off(kx=k2)
    v = THREE.copy()
    v[17] = np.inf
    off(vel=v)
    k5 = kx.copy()
    k5[[1, 2, TNUM - 1, TNUM - 2]] = 0.0                                                    # five zero wavenumbers
    off(kx=k5)
    k4 = kx.copy()
    k4[[1, TNUM - 1]] = 0.0                                                                 # (three: still the half walk)
    assert go(lib, F32, 1.69e8, kx=k4)['k_zero'] == [0, 1, TNUM - 1]
    off(env={'IMPDAR_PS_HERMITIAN': '0'})


@pytest.mark.parametrize('dtype,vel,env,want', [
    (F32, 1.69e8, {}, ['NUFFT', 'MFMA', 'VECTOR']),
    (F32, 1.69e8, {'IMPDAR_PS_MFMA': '0'}, ['VECTOR']),
    (F32, 1.69e8, {'IMPDAR_PS_MFMA': '3'}, ['VECTOR']),                 # (3 and 2 keep the transform path out: it is tried at 1 and 6 only)
    (F32, 1.69e8, {'IMPDAR_PS_MFMA': '2'}, ['MFMA', 'VECTOR']),
    (F32, 1.69e8, {'IMPDAR_PS_MFMA': '6'}, ['NUFFT', 'MFMA', 'VECTOR']),
    (F32, 1.69e8, {'IMPDAR_PS_MFMA': '7'}, ['VECTOR']),
    (F64, 1.69e8, {}, ['NUFFT', 'VECTOR']),
    (F64, 1.69e8, {'IMPDAR_PS_MFMA': '0'}, ['VECTOR']),
    (F32, THREE, {}, ['NUFFT', 'MFMA', 'RUNS', 'VECTOR']),
    (F32, FOUR, {}, ['NUFFT', 'RUNS', 'MFMA', 'VECTOR']),
    (F32, MANY, {}, ['SERIES', 'MFMA', 'RUNS', 'VECTOR']),              # (one long run: not runs_first)
    (F32, GRADIENT, {}, ['SERIES', 'MFMA', 'RUNS', 'SMOOTH', 'VECTOR']),     # (128 runs of one step, none long: not runs_first)
    (F32, GRADIENT, {'IMPDAR_PS_MFMA': '0'}, ['SMOOTH', 'VECTOR']),
    (F32, GRADIENT, {'IMPDAR_PS_MFMA': '7'}, ['SERIES', 'SMOOTH', 'VECTOR']),
    (F32, THREE, {'IMPDAR_PS_MFMA': '7'}, ['SERIES', 'VECTOR']),
    (F64, THREE, {}, ['NUFFT', 'SERIES', 'VECTOR']),
    (F64, THREE, {'IMPDAR_PS_MFMA': '7'}, ['SERIES', 'VECTOR']),
    (F64, GRADIENT, {}, ['SERIES', 'SMOOTH', 'VECTOR']),
    # the test hook: SERIES, NUFFT and RUNS leave every float32 list, MFMA stays (it declines through its own use of the hook); float64 untouched
    (F32, 1.69e8, {'IMPDAR_PS_TEST_EDGE_OVERFLOW': '1'}, ['MFMA', 'VECTOR']),
    (F32, THREE, {'IMPDAR_PS_TEST_EDGE_OVERFLOW': '1'}, ['MFMA', 'VECTOR']),
    (F32, FOUR, {'IMPDAR_PS_TEST_EDGE_OVERFLOW': '1'}, ['MFMA', 'VECTOR']),
    (F32, MANY, {'IMPDAR_PS_TEST_EDGE_OVERFLOW': '1'}, ['MFMA', 'VECTOR']),
    (F32, GRADIENT, {'IMPDAR_PS_TEST_EDGE_OVERFLOW': '1'}, ['MFMA', 'SMOOTH', 'VECTOR']),
    (F64, THREE, {'IMPDAR_PS_TEST_EDGE_OVERFLOW': '1'}, ['NUFFT', 'SERIES', 'VECTOR']),
    (F64, GRADIENT, {'IMPDAR_PS_TEST_EDGE_OVERFLOW': '1'}, ['SERIES', 'SMOOTH', 'VECTOR']),
])
def test_attempt_lists(lib, dtype, vel, env, want):
    dbl, snum = dtype == F64, SNUM if np.ndim(vel) == 0 else len(vel)
    r = go(lib, dtype, vel, snum=snum, env=env)
    assert r['attempts'] == want
    nf = NT // 2
    if np.ndim(vel):
        m = model(vel, dbl, nf)
        assert {k: r[k] for k in m} == m
        # the preconditions the case stands for
        if vel is THREE or vel is FOUR:
            assert m['use_sched'] and m['nufft_first'] and (m['long_runs'] <= 3) == (vel is THREE)
        if vel is MANY:
            assert m['use_sched'] and not m['nufft_first'] and m['runs'] > 64
        if vel is GRADIENT:
            assert not m['use_sched'] and m['runs'] == SNUM and m['long_runs'] == 0
    else:
        assert (r['runs'], r['long_runs']) == (1, 1)
    fq, sq = nf / 4096., snum / 8192.
    if 'SERIES' in want:
        alt = r['alts'][want.index('SERIES')]
        if env.get('IMPDAR_PS_MFMA') == '7':
            assert alt == 0.0
        elif vel is GRADIENT:
            assert alt == (-10.8e-6 if dbl else -5.3e-6)                   # -SR_MS_PER_PAIR_*
        elif dbl:
            assert alt == 43. * fq * sq + 0.09 * r['runs'] * fq
        else:
            assert alt == 8. * fq * sq + 0.036 * r['runs'] * fq
    # what the metrics line reports: float64 counts its long runs only where the transform path may take a table
    counted = not dbl or (np.ndim(vel) and r['use_sched'] and env.get('IMPDAR_PS_MFMA', '1') in ('1', '6'))
    assert r['long_runs_metric'] == (r['long_runs'] if counted else 0)


def test_half_front(lib):
    kx, ws = PC.axes(TNUM, NT)
    for dtype in (F32, F64):
        assert go(lib, dtype, 1.69e8)['half_front']
        assert go(lib, dtype, 1.69e8, env={'IMPDAR_PS_MFMA': '6'})['half_front']
        assert not go(lib, dtype, 1.69e8, tk_out=True)['half_front']
        assert not go(lib, dtype, 1.69e8, k0=0, nk=TNUM // 2)['half_front']
        assert not go(lib, dtype, 1.69e8, tnum=63)['half_front']
        assert not go(lib, dtype, 1.69e8, snum=63)['half_front']
        assert not go(lib, dtype, 1.69e8, snum=64, nt=64)['half_front']          # nf = 32
        assert go(lib, dtype, 1.69e8, snum=64, nt=128)['half_front']             # nf = 64
        for pref in '0237':
            assert not go(lib, dtype, 1.69e8, env={'IMPDAR_PS_MFMA': pref})['half_front']
        for fft in ('strided', 'rocfft'):
            assert not go(lib, dtype, 1.69e8, env={'IMPDAR_PS_FFT': fft})['half_front']
        # a single zero wavenumber that is not row 0 (the Nyquist row is its own mirror image: the walk stays Hermitian)
        k1 = kx.copy()
        k1[0], k1[TNUM // 2] = kx[TNUM // 2], 0.0
        r = go(lib, dtype, 1.69e8, kx=k1)
        assert r['herm'] and r['k_zero'] == [TNUM // 2] and not r['half_front']
        assert not go(lib, dtype, float('inf'))['half_front'] and not go(lib, dtype, 0.0)['half_front']
    # a table: as nufft_first (6: any table with a schedule)
    assert go(lib, F32, THREE)['half_front'] and go(lib, F64, THREE)['half_front']
    r = go(lib, F32, MANY, snum=len(MANY))
    assert r['use_sched'] and not r['nufft_first'] and not r['half_front']
    assert go(lib, F32, MANY, snum=len(MANY), env={'IMPDAR_PS_MFMA': '6'})['half_front']
    assert not go(lib, F32, GRADIENT)['half_front'] and not go(lib, F32, GRADIENT, env={'IMPDAR_PS_MFMA': '6'})['half_front']


def test_nufft_first_at_field_size(lib):
    """8192^2 float32: the config-5 table and a 41-row table go to the transform path first, tables of
    81 and 161 rows to the runs kernels.  The tables as bench.py builds them; host arithmetic only."""
    import bench
    from impdar_amd import synth
    from oracle import mig_oracle
    n = 8192
    geo = synth.geometry(n, n)
    kx, ws = PC.axes(n, n)
    Rp = 1.9e8 * geo['travel_time'][-1] * 1e-6 / 2.
    assert np.array_equal(bench.gazdag_velocity('layers41', geo, n), np.stack([np.linspace(1.69e8, 2.2e8, 41), np.linspace(0., 2.0 * Rp, 41)], axis=1))
    tables = [('vz4', bench.gazdag_velocity('vz4', geo, n), True), ('layers41', bench.gazdag_velocity('layers41', geo, n), True)] + \
             [('layers%d' % rows, np.stack([np.linspace(1.69e8, 2.2e8, rows), np.linspace(0., 2.0 * Rp, rows)], axis=1), False) for rows in (81, 161)]
    for name, tab, want in tables:
        v = np.ascontiguousarray(mig_oracle.get_velocity_profile(geo['travel_time'], tab))
        r = PC.route(lib, F32, n, kx, ws, v)
        m = model(v, False, n // 2)
        assert r['use_sched'] and {k: r[k] for k in m} == m, name
        # (81 and 161 rows: more than 128 single steps at the boundaries, whatever the two estimates say)
        assert r['nufft_first'] == want and (not want or r['nufft_ms'] <= r['runs_ms']), (name, r['nufft_ms'], r['runs_ms'])
        assert r['attempts'][0] == ('NUFFT' if want else 'SERIES' if r['runs'] > 64 else 'RUNS'), name


def test_row_order(lib):
    tnum = 512
    kx, ws = PC.axes(tnum, NT)
    v = layers([24, 40, 64])
    assert go(lib, F32, v, tnum=tnum, rows=True)['rowmap'] == []                 # no wavenumber near a boundary
    # rows 7 and 9 (and their mirror images) on 2 |w_j| / v of the second and of the third run
    k2 = kx.copy()
    k2[7], k2[9] = 2. * ws[11] / v[30], 2. * ws[5] / v[100]
    k2[tnum - 7], k2[tnum - 9] = -k2[7], -k2[9]
    for dtype in (F32, F64):
        r = go(lib, dtype, v, tnum=tnum, kx=k2, rows=True)
        assert r['runs'] == 3 and r['use_sched']
        # the flagged rows first, longest first (64 steps before 40), stable; then everything else in its natural order
        assert r['rowmap'] == [9, tnum - 9, 7, tnum - 7] + [k for k in range(tnum) if k not in (7, 9, tnum - 7, tnum - 9)]
    assert go(lib, F32, v, tnum=64, kx=np.concatenate([k2[:32], k2[-32:]]), rows=True)['rowmap'] == []         # tnum < 512
    many = np.concatenate([v[0] + 1e3 * np.arange(70), np.full(SNUM - 70, v[100])])
    r = go(lib, F64, many, tnum=tnum, kx=k2, rows=True)
    assert r['runs'] > 64 and r['use_sched'] and r['rowmap'] == []              # more than 64 runs


def test_route_agrees_with_what_the_library_reported(lib):
    """tests/ps_route_recorded.json: the metrics of every case of ps_route_cases.py from a GPU run of the commit before ps_route.h."""
    with open(PC.RECORDED) as f:
        rec = json.load(f)
    assert sorted(rec['cases']) == sorted(PC.IDS)
    for c, cid in zip(PC.CASES, PC.IDS):
        kx, ws = PC.axes(c['tnum'], c['nt'])
        r = PC.route(lib, c['dtype'], PC.SNUM, kx, ws, PC.velocity(c['vel']), env=c['env'])
        m = rec['cases'][cid]
        assert (r['herm'], r['nf'], r['long_runs_metric']) == (m['hermitian_walk'], m['frequencies'], m['long_runs']), cid
        assert (m['transforms'] == 'own') == r['use_own'], cid
        assert any(m['kernel'] in PC.KERNELS[a] for a in r['attempts']), (cid, m['kernel'], r['attempts'])
        if m.get('spectrum') == 'k >= 0, all frequencies':
            assert r['half_front'] and m['kernel'] == 'ps_nufft_kernel', cid
