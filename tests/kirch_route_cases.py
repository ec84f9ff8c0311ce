"""The cases of the Kirchhoff plan's host-side route (test infrastructure, shared by tests/test_kirch_route.py and
tests/test_kirch_route_gpu.py): geometries and knob settings that reach every branch of csrc/kirch_route.h, the axes of each,
and the header compiled by itself with g++ and driven through its probe.  What the library reported on the GPU for the cases
marked gpu, at the commit before the route was split out of impdar_kirch_plan_create, is in tests/kirch_route_recorded.json."""
import ctypes as C
import os

import numpy as np

RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'kirch_route_recorded.json')
VEL, DT = 1.69e8, 1.0e-8
AUTO, EXACT, FAST = 0, 1, 2
KERNELS = ('EXACT_PAIR', 'EXACT_TAB', 'DQUAD', 'QUAD', 'TAB', 'GEN')
UNSUPPORTED = -6
KNOBS = ('XB', 'NH', 'LK', 'PARTS', 'NHD', 'XBD', 'IMPL', 'EXACT_IMPL', 'TIEFIX')


def dx_for(sa):
    """The trace spacing whose moveout 2 dx / (v dt) is sa samples per trace."""
    return sa * VEL * DT / 2.0


def case(name, dtype='float32', snum=300, tnum=96, sa=1.2, mode=AUTO, nranks=1, nearfield=0, env=None, dist='uniform', tt='uniform',
         t0_us=0.0, tmax=None, caller_tables=False, gpu=False):
    return dict(id=name, dtype=dtype, snum=snum, tnum=tnum, sa=sa, mode=mode, nranks=nranks, nearfield=nearfield, env=env or {},
                dist=dist, tt=tt, t0_us=t0_us, tmax=tmax, caller_tables=caller_tables, gpu=gpu)


def _cases():
    out = []
    # float32 on uniform axes by the moveout: 40 fits, only 24 (under and over 65535 bytes of ring), only tab, neither (gen; a spacing gen cannot hold either: refused in FAST)
    for name, sa in (('sa1.2', 1.2), ('sa4', 4.0), ('sa5', 5.0), ('sa10', 10.0), ('sa20', 20.0)):
        out.append(case('f32-' + name, sa=sa, gpu=True))
    out.append(case('f32-sa30-fast', sa=30.0, mode=FAST))
    out.append(case('f32-sa30-auto', sa=30.0))
    out.append(case('f32-sa1.2-fast', sa=1.2, mode=FAST))
    out.append(case('f32-sa1.2-exact', sa=1.2, mode=EXACT, gpu=True))
    out.append(case('f32-sa0.5', sa=0.5))
    # the tile pair: whole radargrams whose two-tile ring is above 65535 bytes and at most 80 KB; blocks of a many-rank plan keep one tile
    for nranks in (1, 2, 4, 8):
        out.append(case('f32-pair-r%d' % nranks, snum=64, tnum=8192, nranks=nranks, gpu=nranks == 1))
    out.append(case('f32-pair-sa0.5', snum=64, tnum=8192, sa=0.5))
    out.append(case('f32-near', nearfield=1, gpu=True))
    out.append(case('f32-near-pair', snum=64, tnum=8192, nearfield=1))
    # each knob, one at a time off the default
    for k, vals in (('XB', ('24', '32', '40', '7')), ('NH', ('2', '3')), ('LK', ('1',)), ('IMPL', ('tab', 'gen')), ('PARTS', ('2', '4'))):
        for v in vals:
            out.append(case('f32-%s=%s' % (k, v), env={'IMPDAR_KIRCH_' + k: v}, gpu=(k, v) in (('XB', '24'), ('XB', '32'), ('NH', '2'), ('NH', '3'), ('IMPL', 'tab'), ('IMPL', 'gen'))))
    out.append(case('f32-pair-XB=7', snum=64, tnum=8192, env={'IMPDAR_KIRCH_XB': '7'}))
    out.append(case('f32-NH=2-LK=1', env={'IMPDAR_KIRCH_NH': '2', 'IMPDAR_KIRCH_LK': '1'}, gpu=True))
    out.append(case('f32-sa4-NH=2', sa=4.0, env={'IMPDAR_KIRCH_NH': '2'}))
    out.append(case('f32-sa20-IMPL=tab', sa=20.0, env={'IMPDAR_KIRCH_IMPL': 'tab'}))
    out.append(case('f32-TIEFIX=0', env={'IMPDAR_KIRCH_TIEFIX': '0'}))
    # float64 exact: two tiles of 20, one of 20, one of 16, none
    out.append(case('f64-pair', 'float64', snum=64, tnum=8192, mode=EXACT, gpu=True))
    out.append(case('f64-pair-r2', 'float64', snum=64, tnum=8192, mode=EXACT, nranks=2))
    for name, sa in (('sa1.2', 1.2), ('sa3', 3.0), ('sa5', 5.0), ('sa8', 8.0)):
        out.append(case('f64-' + name, 'float64', sa=sa, mode=EXACT, gpu=True))
    out.append(case('f64-auto', 'float64', gpu=True))
    out.append(case('f64-fast', 'float64', mode=FAST))
    out.append(case('f64-near-NHD=2', 'float64', sa=2.0, nearfield=1, env={'IMPDAR_KIRCH_NHD': '2'}))
    for env in ({'XBD': '16'}, {'XBD': '20'}, {'NHD': '2'}, {'NHD': '2', 'XBD': '20'}, {'EXACT_IMPL': 'tab'}, {'EXACT_IMPL': 'pair'}):
        name = 'f64-' + '-'.join('%s=%s' % kv for kv in sorted(env.items()))
        out.append(case(name, 'float64', sa=2.0, mode=EXACT, env={'IMPDAR_KIRCH_' + k: v for k, v in env.items()}, gpu=True))
    out.append(case('f64-sa1.2-NHD=2', 'float64', mode=EXACT, env={'IMPDAR_KIRCH_NHD': '2'}))
    out.append(case('f32-exact-EXACT_IMPL=pair', mode=EXACT, env={'IMPDAR_KIRCH_EXACT_IMPL': 'pair'}))
    # axes off the grid: dist sorted / unsorted, tt off by 1e-10 dt (uniform to 1e-9, not to 1e-11) and by 1e-8 dt; tt not increasing
    for dtype in ('float32', 'float64'):
        out.append(case(dtype[-2:] + '-jitter', dtype, dist='jitter', gpu=True))
        out.append(case(dtype[-2:] + '-zigzag', dtype, dist='zigzag', gpu=dtype == 'float32'))
    out.append(case('f32-zigzag-fast', dist='zigzag', mode=FAST))
    out.append(case('f32-jitter-exact', dist='jitter', mode=EXACT))
    for ttk in ('e-10', 'e-8'):
        out.append(case('f32-tt-' + ttk, tt=ttk))
        out.append(case('f32-jitter-tt-' + ttk, dist='jitter', tt=ttk))
        out.append(case('f64-tt-' + ttk, 'float64', tt=ttk))
    out.append(case('f32-tt-flat', tt='flat'))
    # the limits: 65536 samples; an aperture of 65000 traces and more; a walk beyond the 2 GiB raw buffer
    for dtype in ('float32', 'float64'):
        out.append(case(dtype[-2:] + '-snum65536', dtype, snum=65536))
        out.append(case(dtype[-2:] + '-aperture', dtype, sa=1.0e-3))
        out.append(case(dtype[-2:] + '-span', dtype, snum=60000, tnum=5000))
    # pre-trigger samples and a first sample after the trigger
    out.append(case('f32-pretrigger', t0_us=-0.03, gpu=True))
    out.append(case('f64-posttrigger', 'float64', t0_us=0.05, gpu=True))
    out.append(case('f32-tnum1', tnum=1))
    # mig_kirch_loop: the caller's time limit with the plan's own tables, and the caller's own tables
    tlim = float(np.float32((300 - 1) * DT))
    out.append(case('f64-hook-standard', 'float64', mode=EXACT, tmax=tlim))
    out.append(case('f64-hook-own', 'float64', mode=EXACT, tmax=0.9 * tlim, caller_tables=True))
    return out


CASES = _cases()
IDS = [c['id'] for c in CASES]
GPU_CASES = [c for c in CASES if c['gpu']]
assert len(set(IDS)) == len(IDS)


def axes(c):
    """(dist [m], tt [s]) of a case."""
    snum, tnum = c['snum'], c['tnum']
    dx = dx_for(c['sa'])
    j = np.arange(tnum)
    dist = {'uniform': j * dx, 'jitter': j * dx + (j % 3) * 0.2 * dx, 'zigzag': j * dx + (j % 2) * 2.5 * dx}[c['dist']]
    tt = c['t0_us'] * 1.0e-6 + np.arange(snum) * DT
    if c['tt'] in ('e-10', 'e-8'):
        tt[1:-1:2] += {'e-10': 1.0e-10, 'e-8': 1.0e-8}[c['tt']] * DT
    elif c['tt'] == 'flat':
        tt[7] = tt[6]
    # (through the unit conversions of impdar_amd.kirchhoff.KirchhoffPlan, so that the probe sees the plan's own values)
    return np.ascontiguousarray(dist / 1.0e3 * 1.0e3, dtype=np.float64), np.ascontiguousarray(tt * 1.0e6 / 1.0e6, dtype=np.float64)


# ---- the host-only header compiled by itself (as tests/ps_route_cases.py does with ps_route.h)
def probe(tmpdir):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, lib = os.path.join(tmpdir, 'kirch_route_probe.cpp'), os.path.join(tmpdir, 'libkirchroute.so')
    with open(src, 'w') as f:
        f.write('#define KIRCH_ROUTE_PROBE 1\n#include "kirch_route.h"\n')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-shared', '-fPIC', '-I', os.path.join(root, 'impdar_amd', 'csrc'), src, '-o', lib])
    return C.CDLL(lib)


def knob_array(env):
    """The KirchKnobs of an environment as the probe takes them (what KirchKnobs::from_env would read)."""
    k = []
    for name in ('XB', 'NH', 'LK', 'PARTS', 'NHD', 'XBD'):
        v = env.get('IMPDAR_KIRCH_' + name)
        k += [int(v is not None), int(v) if v is not None and v.lstrip('-').isdigit() else 0]          # (atoi: 0 for what is no number)
    impl, ex = env.get('IMPDAR_KIRCH_IMPL'), env.get('IMPDAR_KIRCH_EXACT_IMPL')
    k += [{None: 0, 'tab': 1, 'gen': 2}.get(impl, 0), 0 if ex is None else (2 if ex == 'pair' else 1), int(env.get('IMPDAR_KIRCH_TIEFIX') == '0')]
    return np.array(k, dtype=np.int32)


_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
INTS = ('status', 'mode', 'kernel', 'tnum_pad', 'gen', 'genW', 'quad', 'dquad', 'xb', 'nh', 'lk', 'quadW', 'quadSH', 'walk_parts_log2',
        'want_tie_scan', 'xtab_off', 'tie_ambiguous', 'want_tie_groups', 'increasing', 'uni_t', 'uni_t11', 'uni_x', 'dist_sorted')
DBLS = ('tmax', 'dt', 'dx', 'xnoise', 'sa', 'alpha', 'hest', 'gen_need', 'err_limit', 'err_sa')


def route(lib, c, ties=None, cap=1 << 20):
    """kirch_geometry + kirch_route (+ kirch_route_after_ties with `ties` flagged picks) on a case: a dict of what they decided."""
    dist, tt = axes(c)
    ints, dbls = np.zeros(32, dtype=np.int32), np.zeros(16)
    tmax = None if c['tmax'] is None else C.byref(C.c_double(c['tmax']))
    lib.impdar_kirch_route_probe.argtypes = [C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, _ip,
                                             C.c_longlong, C.c_longlong, _ip, _dp]
    rc = lib.impdar_kirch_route_probe(int(c['dtype'] == 'float64'), c['snum'], c['tnum'], dist.ctypes.data_as(_dp), tt.ctypes.data_as(_dp), VEL,
                                      c['nearfield'], c['mode'], c['nranks'], C.cast(tmax, C.c_void_p) if tmax is not None else None,
                                      int(c['caller_tables']), knob_array(c['env']).ctypes.data_as(_ip), -1 if ties is None else ties, cap,
                                      ints.ctypes.data_as(_ip), dbls.ctypes.data_as(_dp))
    assert rc == 0
    r = {k: int(v) for k, v in zip(INTS, ints)}
    r.update({k: float(v) for k, v in zip(DBLS, dbls)})
    r['kernel'] = KERNELS[r['kernel']] if r['kernel'] >= 0 else None
    return r


def tables(lib, c):
    """The host tables of a case's plan (uniform axes): a dict of arrays."""
    dist, tt = axes(c)
    snum, nch = c['snum'], (c['snum'] + 255) // 256
    big = nch * (c['tnum'] + 256) * 2 + 4096
    sizes, h_half = np.zeros(8, dtype=np.int32), np.zeros(snum, dtype=np.int32)
    c32, c64 = np.zeros(3 * snum, dtype=np.float32), np.zeros(3 * snum)
    hmax, klo, khi, win = np.zeros(nch, dtype=np.int32), np.zeros(big, dtype=np.int32), np.zeros(big, dtype=np.int32), np.zeros(big, dtype=np.int32)
    fp = C.POINTER(C.c_float)
    lib.impdar_kirch_tables_probe.argtypes = [C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_double, C.c_int, C.c_int, C.c_int, _ip, _ip, _ip, fp, _dp,
                                              fp, _dp, _ip, _ip, _ip, _ip]
    rc = lib.impdar_kirch_tables_probe(int(c['dtype'] == 'float64'), snum, c['tnum'], dist.ctypes.data_as(_dp), tt.ctypes.data_as(_dp), VEL,
                                       c['nearfield'], c['mode'], c['nranks'], knob_array(c['env']).ctypes.data_as(_ip), sizes.ctypes.data_as(_ip),
                                       h_half.ctypes.data_as(_ip), c32.ctypes.data_as(fp), c64.ctypes.data_as(_dp), None, None,
                                       hmax.ctypes.data_as(_ip), klo.ctypes.data_as(_ip), khi.ctypes.data_as(_ip), win.ctypes.data_as(_ip))
    assert rc == 0
    n = dict(zip(('nchunks', 'nb', 'ntab', 'nrows', 'mrow0', 'refused', 'nwin'), (int(v) for v in sizes)))
    assert n['nchunks'] * n['nb'] <= big and n['nwin'] <= big
    n.update(h_half=h_half, c32=c32.reshape(3, snum), c64=c64.reshape(3, snum), hmax=hmax, klo=klo[:n['nchunks'] * n['nb']].reshape(n['nchunks'], n['nb']),
             khi=khi[:n['nchunks'] * n['nb']].reshape(n['nchunks'], n['nb']), win=win[:n['nwin']].reshape(n['nchunks'], -1, 2) if n['nwin'] else None)
    return n


def group_ties(lib, pairs):
    t = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    n = len(t)
    g_ti, g_off, g_n = np.zeros(n + 1, dtype=np.int32), np.zeros(n + 2, dtype=np.int32), np.zeros(n + 1, dtype=np.int32)
    ng = lib.impdar_kirch_ties_probe(t.ctypes.data_as(_ip), n, g_ti.ctypes.data_as(_ip), g_off.ctypes.data_as(_ip), g_n.ctypes.data_as(_ip))
    return g_ti[:ng].tolist(), g_off[:ng + 1].tolist(), g_n[:n].tolist()


def tilemap(lib, hmax, tnum, xlo, xhi, tile_w, align_mask, ring_blocks, step_block, G, tiles_per_xcd):
    hm = np.ascontiguousarray(hmax, dtype=np.int32)
    m = np.zeros(len(hm) * tiles_per_xcd * 8, dtype=np.int16)
    n = lib.impdar_kirch_tilemap_probe(hm.ctypes.data_as(_ip), len(hm), tnum, xlo, xhi, tile_w, align_mask, ring_blocks, step_block, G, tiles_per_xcd,
                                       m.ctypes.data_as(C.POINTER(C.c_short)))
    return m[:n].reshape(len(hm), tiles_per_xcd, 8) if n else None


def oneshot_cuts(lib, tnum, halo, two=False):
    """kirch_oneshot_cuts: (output cuts, input traces each block needs) of the one-shot entry point's pipeline."""
    cut, need = np.full(16, -1, dtype=np.int32), np.full(16, -1, dtype=np.int32)
    n = lib.impdar_kirch_oneshot_cuts_probe(tnum, halo, int(two), cut.ctypes.data_as(_ip), need.ctypes.data_as(_ip))
    return cut[:n + 1].tolist(), need[:n].tolist()


# ---- one plan through the C ABI under a case's knobs (GPU)
def run(hip, c, monkeypatch=None):
    """Create the plan of case c, one prep and one migrate of a noise radargram: (what the plan reports, the image)."""
    from impdar_amd.kirchhoff import KirchhoffPlan
    dist, tt = axes(c)
    if monkeypatch is not None:
        for k in KNOBS:
            monkeypatch.delenv('IMPDAR_KIRCH_' + k, raising=False)
        for k, v in c['env'].items():
            monkeypatch.setenv(k, v)
    ctx = hip.context()
    x = np.random.default_rng(c['snum'] + c['tnum']).standard_normal((c['snum'], c['tnum'])).astype(c['dtype'])
    plan = KirchhoffPlan(ctx, x.dtype, c['snum'], c['tnum'], dist / 1.0e3, tt * 1.0e6, VEL, bool(c['nearfield']), ('auto', 'exact', 'fast')[c['mode']],
                         c['nranks'])
    d_in, d_out = hip.DeviceArray.from_host(ctx, x), hip.DeviceArray(ctx, x.shape, x.dtype)
    try:
        plan.prep(d_in, c['tnum'], 0, c['tnum'])
        plan.migrate(d_out, 0, c['tnum'])
        plan.sync()
        img = d_out.to_host()
        rep = dict(kernel=plan.kernel, mode=plan.mode, tnum_pad=plan.tnum_pad, xnoise=plan.xnoise)
    finally:
        plan.destroy()
        d_in.free()
        d_out.free()
    return rep, x, img
