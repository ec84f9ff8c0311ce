"""Picked-layer analysis (``impdar_amd/lib/analysis/``) against the ``YA_*`` fixtures the reference wrote
(``tests/golden/make_golden_analysis.py``): what every function returns, what it leaves in ``dat.picks`` and in the caller's
arrays, bit for bit (NaN and Inf positions included), and the kind of every recorded exception.  No GPU is needed: the
window search of methods 3 and 6b runs through its NumPy form where no device is visible, and its fixtures are decided
by margins far above either form's rounding.  The restatement of the search that the GPU tests compare against
(``tests/analysis_ref.py``) is held to the fixtures here."""
import functools
import inspect
import json

import numpy as np
import pytest

from conftest import golden, golden_names

import analysis_ref as ar

NAMES = golden_names('YA_')


def mods():
    from impdar_amd.lib.analysis import Roughness, attenuation, geometric_power_corrections
    return {'power': geometric_power_corrections, 'att': attenuation, 'rough': Roughness}


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype.kind == b.dtype.kind and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


def recorded(g):
    return {k: v for k, v in g.items() if k.startswith(('out', 'after')) or k == 'raised'}


def test_the_fixtures_the_issue_names_are_there():
    assert {'YA_m3_400', 'YA_m3_1000', 'YA_m3_nan', 'YA_m3_odd', 'YA_m3_step1', 'YA_m6b_km', 'YA_m6b_m', 'YA_m6b_flat', 'YA_m2',
            'YA_m2_deming', 'YA_m5_w1', 'YA_m5_w1_deming', 'YA_m5_w11', 'YA_m5_w11_deming', 'YA_m6a', 'YA_m6a_deming', 'YA_m7',
            'YA_pc_plain', 'YA_pc_time', 'YA_pc_firn', 'YA_pc_air', 'YA_rf_scalar', 'YA_rf_scalar_above', 'YA_rf_array',
            'YA_rough_gaps', 'YA_rough_noz'} <= set(NAMES)
    assert golden_names('YAE') == ['YAE_errors']


@pytest.mark.parametrize('name', NAMES)
def test_public_function_equals_the_reference(name, capsys):
    g = golden(name)
    want = recorded(g)
    got = ar.run_call(mods(), g)
    assert 'raised' not in want and sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k in want:
        assert same(got[k], want[k]), (name, k)
    # the warning of the constant velocity is printed exactly where picks.z is absent
    assert ('setting pick depth for constant velocity' in capsys.readouterr().out) == ('picks_time' in g)


def test_in_place_conversions_are_the_reference_s():
    """Methods 5 and 7 turn the caller's picks.z into kilometres, 6a and 6b the caller's att_ds; 2 and 3 leave both."""
    for name, key, changed in (('YA_m5_w1', 'after_picks_z', True), ('YA_m7', 'after_picks_z', True), ('YA_m2', 'after_picks_z', False),
                               ('YA_m3_400', 'after_picks_z', False), ('YA_m6a', 'after@att_ds', True), ('YA_m6b_m', 'after@att_ds', True),
                               ('YA_m6b_km', 'after@att_ds', False), ('YA_m6b_m', 'after_picks_z', False)):
        g = golden(name)
        before = g['picks_z'] if key == 'after_picks_z' else g[key[6:]]
        assert same(g[key], before / 1000. if changed else before), (name, key)
        assert same(ar.run_call(mods(), g)[key], g[key]), (name, key)


def test_every_error_case_raises_the_recorded_kind():
    g = golden('YAE_errors')
    names = [str(n) for n in g['names']]
    assert {'rough_no_interp', 'pc_first_depth', 'm7_not_double', 'm6b_first_outside', 'm3_first_not_entered', 'm3_tie', 'm3_no_zero',
            'm3_constant_depth'} <= set(names)
    for n in names:
        case = {k[len(n) + 2:]: v for k, v in g.items() if k.startswith(n + '__')}
        assert ar.run_call(mods(), case) == dict(raised=str(case['raised'])), n


@functools.lru_cache(maxsize=None)
def searched(name):
    """The restatement's answer to a search fixture."""
    g = golden(name)
    spec = json.loads(str(g['call']))
    kw = spec['kwargs']
    if spec['fn'] == 'attenuation_method3':
        z, pc = ar.prepared(g['picks_z'][0], g['picks_corrected_power'][0])
        return ar.search(ar.INDEX, z, pc, g['Ns'], 0.1, 1., kw['win_init'], kw['win_step'],
                         range(kw['win_init'] // 2, int(g['tnum']) - kw['win_init'] // 2), count=int(g['tnum']))
    z, pc = ar.prepared(g['picks_z'][spec['args'][0]].flatten(), g['picks_corrected_power'][spec['args'][0]].flatten())
    scale = 1000. if kw['win_init'] > 10. else 1.
    return ar.search(ar.DEPTH, z, pc, g['Ns'], 0.1, 1., kw['win_init'] / scale, kw['win_step'] / scale, g['after@att_ds'])


@pytest.mark.parametrize('name', [n for n in NAMES if n.startswith(('YA_m3', 'YA_m6b'))])
def test_search_restatement_equals_the_reference(name):
    g = golden(name)
    rates, widths = searched(name)
    assert np.array_equal(rates, g['out0']) and np.array_equal(widths, g['out1'])


def test_search_restatement_raises_as_the_reference():
    z, pc = ar.synthetic(60, 1)
    with pytest.raises(ValueError):
        ar.search(ar.INDEX, z, pc, np.arange(1., 9.), 0.1, 1., 10, 10, range(5, 55), count=60)          # no rate 0
    with pytest.raises(ValueError):
        ar.search(ar.INDEX, z, pc, np.array([0., 12., 12.]), 0.1, 1., 10, 10, range(5, 55), count=60)    # a tie
    with pytest.raises(UnboundLocalError):
        ar.search(ar.DEPTH, z, pc, np.arange(30.), 0.1, 1., 0.1, 0.1, np.array([0.2, 1.5]))               # first depth outside


def test_host_form_of_the_search_agrees_with_the_restatement():
    """``attsearch.search_host`` -- what the public functions use without a device -- on shapes off the fixtures, centre by
    centre: rates, widths, the stale carry past the NaN-shortened record."""
    from impdar_amd import attsearch
    ns = np.arange(30.)
    for n, tnum, wi, ws in ((90, 100, 8, 6), (70, 70, 5, 3), (64, 64, 2, 1)):
        z, pc = ar.synthetic(n, n)
        traces = range(wi // 2, tnum - wi // 2)
        want = ar.search(ar.INDEX, z, pc, ns, 0.1, 1., wi, ws, traces, count=tnum)
        rates, widths = attsearch.settle(ns, *attsearch.search_host(attsearch.INDEX, z, pc, ns, 0.1, 1., wi, ws, traces))
        assert np.array_equal(rates, want[0][traces.start:traces.stop]) and np.array_equal(widths, want[1][traces.start:traces.stop])
    z, pc = ar.synthetic(500, 3)
    order = np.argsort(z, kind='stable')
    depths = np.linspace(1.2, 1.8, 7)
    want = ar.search(ar.DEPTH, z, pc, ns, 0.1, 1., 0.05, 0.1, depths)
    rates, widths = attsearch.settle(ns, *attsearch.search_host(attsearch.DEPTH, z[order], pc[order], ns, 0.1, 1., 0.05, 0.1, depths))
    assert np.array_equal(rates, want[0]) and np.array_equal(widths * 1000., want[1])


def test_widths_that_cannot_end_are_refused_with_or_without_a_device():
    """``attsearch.search`` checks the widths before it chooses a path: an index width below 2 or a step below 1, fractions,
    a depth step that the width absorbs or that needs more than 2^20 steps across the picks, depths that are not finite."""
    from impdar_amd import attsearch
    from impdar_amd.lib.analysis import attenuation
    ns = np.arange(30.)
    z, pc = ar.synthetic(60, 1)
    for wi, ws in ((1, 1), (0, 5), (2, 0), (2, -1), (2.5, 1), (4, 1.5), (float('nan'), 1), (4, float('inf'))):
        with pytest.raises(ValueError):
            attsearch.search(attsearch.INDEX, z, pc, ns, 0.1, 1., wi, ws, range(2, 58))
    order = np.argsort(z, kind='stable')
    zs, ps = z[order], pc[order]
    inf = zs.copy()
    inf[-1] = np.inf
    for zz, wi, ws in ((zs, 0.2, 1e-17), (zs, 0.2, 1e-9), (zs, 0.0, 0.1), (zs, 0.2, 0.0), (zs, 0.2, float('nan')), (inf, 0.2, 0.1)):
        with pytest.raises(ValueError):
            attsearch.search(attsearch.DEPTH, zz, ps, ns, 0.1, 1., wi, ws, np.array([1.5]))
    # ... and through the public functions
    dat = ar.make_dat(golden('YA_m6b_km'))
    with pytest.raises(ValueError):
        attenuation.attenuation_method6b(dat, [0, 1, 2], np.array([0.8]), win_init=0.2, win_step=1e-17)
    with pytest.raises(ValueError):
        attenuation.attenuation_method3(ar.make_dat(golden('YA_m3_400')), 0, win_init=1, win_step=1)
    dat.picks.z[0, 3] = np.inf
    with pytest.raises(ValueError):
        attenuation.attenuation_method6b(dat, [0, 1, 2], np.array([0.8]), win_init=0.2, win_step=0.1)


def test_signatures_and_defaults_are_the_reference_s():
    m = mods()
    want = {('power', 'power_correction'): "(dat, eps=[], d_eps=[], u=169000000.0, h_aircraft=0.0)",
            ('power', 'refractive_focusing'): "(z1, z2, eps1, eps2)",
            ('att', 'attenuation_method2'): "(dat, picknum, sigPc=0.0, sigZ=0.0, Cint=0.95, u=169000000.0, *args, **kwargs)",
            ('att', 'attenuation_method5'): "(dat, picknums, win=1, sigPc=0, sigZ=0, Cint=0.95, u=169000000.0, *args, **kwargs)",
            ('att', 'attenuation_method6a'): "(dat, picknums, att_ds, win=500.0, sigPc=0, sigZ=0, Cint=0.95, u=169000000.0, *args, **kwargs)",
            ('att', 'attenuation_method7'): "(dat, primary_picknum, secondary_picknum, Rib=-0.22, Rfa=-17, u=169000000.0, *args, **kwargs)",
            ('rough', 'kirchhoff_roughness'): "(dat, picknum, freq, filt_n=101, eps=3.15)"}
    for (mod, fn), sig in want.items():
        assert str(inspect.signature(getattr(m[mod], fn))) == sig, fn
    for fn, names in (('attenuation_method3', ['dat', 'picknum', 'Ns', 'Nh_target', 'Cw', 'win_init', 'win_step', 'u']),
                      ('attenuation_method6b', ['dat', 'picknums', 'att_ds', 'Ns', 'Nh_target', 'Cw', 'win_init', 'win_step', 'u', 'args', 'kwargs'])):
        p = inspect.signature(getattr(m['att'], fn)).parameters
        assert list(p) == names
        assert np.array_equal(p['Ns'].default, np.arange(30.)) and p['Nh_target'].default == 1. and p['Cw'].default == 0.1
        assert p['win_init'].default == 100 and p['win_step'].default == 100 and p['u'].default == 1.69e8
    assert isinstance(inspect.signature(m['att'].attenuation_method3).parameters['win_init'].default, int)
    assert isinstance(inspect.signature(m['att'].attenuation_method6b).parameters['win_init'].default, float)


def test_picks_gain_no_saved_attribute():
    from impdar_amd.lib.Picks import Picks
    assert 'z' not in Picks.attrs and 'corrected_power' not in Picks.attrs
