#!/usr/bin/env python3
"""Generate the ``YA_*`` golden vectors (picked-layer analysis) by running the REFERENCE's
``analysis/geometric_power_corrections.py``, ``analysis/attenuation.py`` and ``analysis/Roughness.py`` -- loaded by path,
never copied -- on the synthetic picks of ``tests/analysis_ref.py``.

Every file is one call: the object's arrays before it (``picks_z`` or ``picks_time``, ``picks_power``,
``picks_corrected_power``, ``tnum``, ``elev``, ``trace_int``, ``flags_interp``), the call itself (``call``: JSON with the
module, the function and its arguments, ``"@key"`` naming an array of the file), what it returned (``out0``, ``out1``), the
object's and the caller's arrays after it (``after_picks_z``, ``after_picks_corrected_power``, ``after@key``) or the type
name of what it raised (``raised``), and the NumPy and SciPy versions.  ``YAE_errors`` holds the error cases, each under
its own prefix.  For the decided method 3 fixtures the script prints the smallest decision margin, the reference's distance
from the ``longdouble`` evaluation and the share of traces that stop before the record's edge.

Only runs where the reference is installed; the committed files are what travels.

Usage:  python tests/golden/make_golden_analysis.py REFERENCE_SRC            (the directory that holds impdar/)
"""
import importlib.util
import json
import os
import sys

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import analysis_ref as ar          # noqa: E402

MODS = {'power': 'geometric_power_corrections', 'att': 'attenuation', 'rough': 'Roughness'}


def load(src):
    mods = {}
    for key, name in MODS.items():
        spec = importlib.util.spec_from_file_location('ref_' + name, os.path.join(src, 'impdar', 'lib', 'analysis', name + '.py'))
        mods[key] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mods[key])
    return mods


def call(mod, fn, *args, **kwargs):
    spec = dict(mod=mod, fn=fn, args=list(args), kwargs=kwargs)
    if kwargs.pop('nodat', False):
        spec['nodat'] = True
    return json.dumps(spec)


def one_pick(tnum, seed=0, nan=0.0):
    z, cp = ar.recipe(tnum, seed)
    if nan:
        cp[np.random.default_rng(seed + 1).random(tnum) < nan] = np.nan
    return dict(picks_z=z[None, :], picks_corrected_power=cp[None, :], tnum=tnum)


def cases():
    c = {}
    ns = np.arange(30.)
    # method 3: the two decided fixtures, NaN traces (stale carry, zero tail), odd widths, a step of one trace
    c['YA_m3_400'] = dict(one_pick(400), Ns=ns, call=call('att', 'attenuation_method3', 0, Ns='@Ns', win_init=20, win_step=20))
    c['YA_m3_1000'] = dict(one_pick(1000, 1), Ns=ns, call=call('att', 'attenuation_method3', 0, Ns='@Ns', win_init=50, win_step=50))
    c['YA_m3_nan'] = dict(one_pick(400, 2, nan=0.1), Ns=ns, call=call('att', 'attenuation_method3', 0, Ns='@Ns', win_init=20, win_step=20))
    c['YA_m3_odd'] = dict(one_pick(300, 3), Ns=ns, call=call('att', 'attenuation_method3', 0, Ns='@Ns', win_init=21, win_step=7))
    c['YA_m3_step1'] = dict(one_pick(300, 4), Ns=ns, call=call('att', 'attenuation_method3', 0, Ns='@Ns', win_init=40, win_step=1))
    # several layers: methods 5, 6a, 6b, 7
    z, p, cp = ar.layers(6, 400, 11)
    many = dict(picks_z=z, picks_power=p, picks_corrected_power=cp, tnum=400)
    picks = [0, 1, 2, 3, 4, 5]
    depths = np.linspace(0.45, 1.45, 12)
    c['YA_m6b_km'] = dict(many, picks_z=z / 1000., Ns=ns, att_ds=depths,
                          call=call('att', 'attenuation_method6b', picks, '@att_ds', Ns='@Ns', win_init=0.2, win_step=0.1))
    c['YA_m6b_m'] = dict(many, Ns=ns, att_ds=depths * 1000.,
                         call=call('att', 'attenuation_method6b', picks, '@att_ds', Ns='@Ns', win_init=200., win_step=100.))
    zf, pf, cpf = ar.layers(6, 400, 12, flat=True)
    c['YA_m6b_flat'] = dict(picks_z=zf / 1000., picks_power=pf, picks_corrected_power=cpf, tnum=400, Ns=ns, att_ds=np.linspace(0.6, 1.2, 5),
                            call=call('att', 'attenuation_method6b', picks, '@att_ds', Ns='@Ns', win_init=0.1, win_step=0.1))
    for tag, kw in (('', {}), ('_deming', dict(sigPc=0.5, sigZ=2.0))):
        c['YA_m2' + tag] = dict(one_pick(400, 5, nan=0.05), call=call('att', 'attenuation_method2', 0, **kw))
        c['YA_m5_w1' + tag] = dict(many, call=call('att', 'attenuation_method5', picks, win=1, **kw))
        c['YA_m5_w11' + tag] = dict(many, call=call('att', 'attenuation_method5', picks, win=11, **kw))
        c['YA_m6a' + tag] = dict(many, att_ds=depths * 1000., call=call('att', 'attenuation_method6a', picks, '@att_ds', win=500., **kw))
    z7 = np.vstack((z[3], 2. * z[3] + 3. * np.sin(np.arange(400) / 9.)))
    cp7 = np.vstack((cp[3], cp[3] * 10. ** (-(17.22 + 2. * 14. * z[3] / 1000.) / 10.) / 4.))
    c['YA_m7'] = dict(picks_z=z7, picks_corrected_power=cp7, tnum=400, call=call('att', 'attenuation_method7', 0, 1))
    # the geometric corrections
    c['YA_pc_plain'] = dict(picks_z=z, picks_power=p, tnum=400, call=call('power', 'power_correction'))
    c['YA_pc_time'] = dict(picks_time=z / 84.5, picks_power=p, tnum=400, call=call('power', 'power_correction'))
    c['YA_pc_firn'] = dict(picks_z=z, picks_power=p, tnum=400, call=call('power', 'power_correction', eps=[2.2, 3.15], d_eps=[0., 70.]))
    c['YA_pc_air'] = dict(picks_z=z, picks_power=p, tnum=400,
                          call=call('power', 'power_correction', eps=[1.8, 2.6, 3.15], d_eps=[0., 30., 90.], h_aircraft=500.))
    c['YA_rf_scalar'] = dict(tnum=0, call=call('power', 'refractive_focusing', 70., 900., 2.2, 3.15, nodat=True))
    c['YA_rf_scalar_above'] = dict(tnum=0, call=call('power', 'refractive_focusing', 70., 60., 2.2, 3.15, nodat=True))
    c['YA_rf_array'] = dict(tnum=0, z2=np.array([10., 70., 70.5, 400., 3000., np.nan]),
                            call=call('power', 'refractive_focusing', 70., '@z2', 2.2, 3.15, nodat=True))
    # roughness: NaN gaps in the pick; no picks.z
    zr, cpr = ar.recipe(600, 6)
    zr[[5, 6, 7, 200, 201, 202, 203, 204, 340]] = np.nan
    zr[400:460] = np.nan
    rough = dict(tnum=600, elev=1200. + 0.01 * np.arange(600.), trace_int=np.full(600, 4.), flags_interp=np.array([1., 4.]))
    c['YA_rough_gaps'] = dict(rough, picks_z=zr[None, :], call=call('rough', 'kirchhoff_roughness', 0, 3.0e6, filt_n=11))
    c['YA_rough_noz'] = dict(rough, picks_time=zr[None, :] / 84.5, call=call('rough', 'kirchhoff_roughness', 0, 5.0e6))
    return c


def error_cases():
    e = {}
    z, p, cp = ar.layers(6, 400, 11)
    zr, cpr = ar.recipe(300, 7)
    few = cpr.copy()
    few[5:] = np.nan
    pick = dict(picks_z=zr[None, :], picks_corrected_power=cpr[None, :], tnum=300)
    e['rough_no_interp'] = dict(picks_z=zr[None, :], tnum=300, elev=np.zeros(300), trace_int=np.full(300, 4.),
                                call=call('rough', 'kirchhoff_roughness', 0, 3.0e6))
    e['pc_first_depth'] = dict(picks_z=z, picks_power=p, tnum=400, call=call('power', 'power_correction', eps=[2.2, 3.15], d_eps=[5., 70.]))
    e['m7_not_double'] = dict(picks_z=z, picks_corrected_power=cp, tnum=400, call=call('att', 'attenuation_method7', 0, 3))
    e['m6b_first_outside'] = dict(picks_z=z / 1000., picks_corrected_power=cp, tnum=400, Ns=np.arange(30.), att_ds=np.array([0.05, 0.8]),
                                  call=call('att', 'attenuation_method6b', [0, 1, 2, 3, 4, 5], '@att_ds', Ns='@Ns', win_init=0.2, win_step=0.1))
    e['m3_first_not_entered'] = dict(pick, picks_corrected_power=few[None, :], Ns=np.arange(30.),
                                     call=call('att', 'attenuation_method3', 0, Ns='@Ns', win_init=20, win_step=20))
    e['m3_tie'] = dict(pick, Ns=np.array([0., 5., 10., 14., 14., 20.]),
                       call=call('att', 'attenuation_method3', 0, Ns='@Ns', win_init=20, win_step=20))
    e['m3_no_zero'] = dict(pick, Ns=np.arange(1., 30.), call=call('att', 'attenuation_method3', 0, Ns='@Ns', win_init=20, win_step=20))
    e['m3_constant_depth'] = dict(pick, picks_z=np.full((1, 300), 1500.), Ns=np.arange(30.),
                                  call=call('att', 'attenuation_method3', 0, Ns='@Ns', win_init=20, win_step=20))
    return e


def report(name, g):
    """Margins and the reference's own error on a sample of the traces of a decided method 3 fixture."""
    spec = json.loads(g['call'])['kwargs']
    z, pc = ar.prepared(g['picks_z'][0], g['picks_corrected_power'][0])
    step = max(1, g['tnum'] // 100)
    smallest, dist, inner = np.inf, 0.0, 0
    traces = range(spec['win_init'] // 2, g['tnum'] - spec['win_init'] // 2)
    for tr in traces[::step]:
        w = ar.walk(ar.INDEX, z, pc, g['Ns'], 0.1, 1., spec['win_init'], spec['win_step'], tr)
        smallest = min(smallest, ar.margin(w['rows'], 0.1))
        dist = max(dist, ar.distance(w['rows'], [ar.c_row_ld(z[at], pc[at], g['Ns']) for at in w['windows']]))
        nxt = w['win'] // 2
        inner += bool(nxt <= tr and nxt <= len(z) - tr)
    print('%s: every %d. trace: smallest margin %.2e, reference - longdouble %.2e, %.0f %% stop before the edge'
          % (name, step, smallest, dist, 100. * inner / len(traces[::step])))


def main(src):
    mods = load(src)
    versions = dict(numpy_version=np.__version__, scipy_version=scipy.__version__)
    for name, g in cases().items():
        g = dict(g, **versions)
        g.update(ar.run_call(mods, g))
        np.savez_compressed(os.path.join(HERE, name + '.npz'), **g)
        print(name, os.path.getsize(os.path.join(HERE, name + '.npz')), 'bytes', g.get('raised', ''))
        if name in ('YA_m3_400', 'YA_m3_1000'):
            rates, widths = ar.search(ar.INDEX, *ar.prepared(g['picks_z'][0], g['picks_corrected_power'][0]), g['Ns'], 0.1, 1.,
                                      json.loads(g['call'])['kwargs']['win_init'], json.loads(g['call'])['kwargs']['win_step'],
                                      range(json.loads(g['call'])['kwargs']['win_init'] // 2, g['tnum'] - json.loads(g['call'])['kwargs']['win_init'] // 2),
                                      count=g['tnum'])
            print('%s: restatement == reference bit for bit: %s' % (name, np.array_equal(rates, g['out0']) and np.array_equal(widths, g['out1'])))
            report(name, g)
    packed = dict(versions)
    names = []
    for name, g in error_cases().items():
        g.update(ar.run_call(mods, g))
        assert 'raised' in g, name
        names.append(name)
        print('YAE_errors', name, g['raised'])
        packed.update({name + '__' + k: v for k, v in g.items()})
    packed['names'] = np.array(names)
    np.savez_compressed(os.path.join(HERE, 'YAE_errors.npz'), **packed)
    print('YAE_errors', os.path.getsize(os.path.join(HERE, 'YAE_errors.npz')), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
