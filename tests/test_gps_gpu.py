"""The time-offset search of kinematic GPS control on the MI355X (csrc/gpstrack.hip) against ``tests/gps_ref.py``.

The probe rows -- the interpolated latitude and longitude of one candidate -- are SciPy's bits (``np.interp`` /
``interp1d(..., fill_value='extrapolate')``), NaN positions included.  ``cc`` is held to the ``longdouble`` evaluation at
the same candidates: |cc_dev - cc_hi| <= 8 x max |cc_ref - cc_hi|, the right-hand side measured per case from the float64
restatement of the reference (never from the device): 8 is the margin this project gives a differently ordered float64
sum over the reference's own rounding.  NaN positions of ``cc`` and the counters ``nout`` are equal.  End to end,
``kinematic_gps_control(guess_offset=True)`` picks the golden's candidate in every pass of the decided fixture and ends on
its bits."""
import ctypes as C
import functools
import os
import sys
from unittest.mock import patch

import numpy as np
import pytest

from conftest import golden

import gps_ref as gr

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference(shape, extrapolate, variant='plain'):
    """The case and what the restatements say of it, computed once: cc_ref, nout, cc_hi, the probe rows."""
    c = gr.sweep_case(*shape, variant=variant)
    args = (c['gps_t'], c['lat'], c['lon'], c['t'], c['rlat'], c['rlon'], c['base'], c['search'], extrapolate)
    cc_ref, nout = gr.cc_f64(*args)
    cc_hi = gr.cc_ld(*args)
    plat, _ = gr.track_f64(c['gps_t'], c['lat'], c['t'], c['search'][c['probe']], c['base'], extrapolate)
    plon, _ = gr.track_f64(c['gps_t'], c['lon'], c['t'], c['search'][c['probe']], c['base'], extrapolate)
    for a in (cc_ref, nout, cc_hi, plat, plon) + tuple(v for v in c.values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return c, cc_ref, nout, cc_hi, plat, plon


def run(c, extrapolate, probe=True):
    from impdar_amd import gpstrack
    return gpstrack.cc_search(c['gps_t'], c['lat'], c['lon'], c['t'], c['rlat'], c['rlon'], c['base'], c['search'], extrapolate,
                              probe=c['probe'] if probe else None)


def held(cc, cc_ref, cc_hi, what):
    """NaN positions equal, and |cc - cc_hi| <= 8 max |cc_ref - cc_hi|; returns the ratio to that maximum."""
    assert np.array_equal(np.isnan(cc), np.isnan(cc_ref)), what
    bound = gr.bound(cc_ref, cc_hi)
    err = gr.bound(cc, cc_hi)
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else np.inf)
    print('%s: max |cc_dev - cc_hi| %.3e, max |cc_ref - cc_hi| %.3e, ratio %.3f' % (what, err, bound, ratio))
    assert err <= 8 * bound, (what, err, bound)
    return ratio


@pytest.mark.parametrize('extrapolate', [False, True])
@pytest.mark.parametrize('shape', gr.SWEEP)
def test_shape_sweep(hip, shape, extrapolate):
    c, cc_ref, nout_ref, cc_hi, plat_ref, plon_ref = reference(shape, extrapolate)
    cc, nout, plat, plon = run(c, extrapolate)
    what = 'tnum %d ngps %d ncand %d extrapolate %d' % (shape + (extrapolate,))
    assert np.array_equal(plat, plat_ref, equal_nan=True), what
    assert np.array_equal(plon, plon_ref, equal_nan=True), what
    assert nout.dtype == np.int64 and np.array_equal(nout, nout_ref), what
    held(cc, cc_ref, cc_hi, what)


@pytest.mark.parametrize('extrapolate', [False, True])
@pytest.mark.parametrize('variant', ['allnan', 'onepair'])
def test_radar_positions_all_nan_and_one_valid_pair(hip, variant, extrapolate):
    c, cc_ref, nout_ref, cc_hi, plat_ref, plon_ref = reference((257, 64, 5), extrapolate, variant)
    cc, nout, plat, plon = run(c, extrapolate)
    assert np.all(np.isnan(cc_ref)) and np.all(np.isnan(cc))          # one correlation of the two has fewer than 2 pairs
    assert np.array_equal(nout, nout_ref)
    assert np.array_equal(plat, plat_ref, equal_nan=True) and np.array_equal(plon, plon_ref, equal_nan=True)


@pytest.mark.parametrize('shape', [(257, 64, 5), (300, 3000, 1001)])
def test_two_calls_same_bits(hip, shape):
    c = reference(shape, False)[0]
    first, again, bare = run(c, False), run(c, False), run(c, False, probe=False)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    assert len(bare) == 2 and bare[0].tobytes() == first[0].tobytes() and bare[1].tobytes() == first[1].tobytes()


def test_rejected_descriptor_launches_nothing(hip):
    from impdar_amd import gpstrack
    c = dict(reference((257, 64, 5), False)[0])
    run(c, False)
    lib, ctx = hip.load(), hip.context()

    def kernel_ms():
        ms = C.c_float()
        hip.check(lib.impdar_ctx_last_kernel_ms(ctx, C.byref(ms)), 'impdar_ctx_last_kernel_ms')
        return ms.value

    before = kernel_ms()
    down, nan = c['gps_t'].copy(), c['gps_t'].copy()
    down[[10, 11]] = down[[11, 10]]
    nan[5] = np.nan
    bad = [dict(gps_t=c['gps_t'][:1], lat=c['lat'][:1], lon=c['lon'][:1]),             # ngps < 2
           dict(t=c['t'][:0], rlat=c['rlat'][:0], rlon=c['rlon'][:0], probe=None),      # tnum < 1
           dict(search=c['search'][:0], probe=None),                                    # ncand == 0 is an error, not a no-op
           dict(gps_t=down), dict(gps_t=nan), dict(probe=5), dict(probe=1 << 40)]
    for change in bad:
        k = dict(c, **change)
        with pytest.raises(ValueError):
            gpstrack.cc_search(k['gps_t'], k['lat'], k['lon'], k['t'], k['rlat'], k['rlon'], k['base'], k['search'], False, probe=k['probe'])
        assert kernel_ms() == before, change
    n = C.c_longlong()
    assert lib.impdar_gps_cc_plan(64, 257, 5, 0, C.byref(n)) == 0 and n.value >= 8 * (3 * 64 + 5 * 257 + 3 * 5)
    assert lib.impdar_gps_cc_plan(64, 257, 0, 0, C.byref(n)) == hip.ERR_ARG
    assert lib.impdar_gps_cc_plan(1 << 62, 257, 5, 0, C.byref(n)) == hip.ERR_ARG


# ---- end to end

def radar_of(g):
    from impdar_amd.lib.NoInitRadarData import NoInitRadarData
    dat = NoInitRadarData(big=True)
    dat.tnum = len(g['decday'])
    for k in ('decday', 'lat', 'long', 'elev'):
        setattr(dat, k, g[k].copy())
    return dat


def control(g, **kw):
    """``kinematic_gps_control`` on a fixture's inputs; the radar file and the passes of the search."""
    from impdar_amd.lib import gpslib
    dat = radar_of(g)
    with patch.object(gpslib, '_search_log', []) as log:
        gpslib.kinematic_gps_control(dat, g['gps_lat'], g['gps_long'], g['gps_elev'], g['gps_decday'], offset=float(g['offset']),
                                     extrapolate=bool(g['extrapolate']), guess_offset=True, **kw)
    return dat, log


@pytest.mark.parametrize('name', ['NAV_decided', 'NAV_extrap'])
def test_kinematic_gps_control_end_to_end(hip, name):
    g = golden(name)
    dat, log = control(g)
    assert len(log) == 5
    order = np.argsort(g['gps_decday'], kind='stable')
    gt, glat, glon = g['gps_decday'][order], g['gps_lat'][order], (g['gps_long'] % 360)[order]
    offset, on_golden, decided_passes = float(g['offset']), True, 0
    for p, (sv, cc, idx) in enumerate(log):
        args = (gt, glat, glon, g['decday'], g['lat'], g['long'] % 360, offset, sv, bool(g['extrapolate']))
        cc_hi = gr.cc_ld(*args)
        # the golden's pass while this run has chosen as the golden did; after a (tolerated) parting, the restatement
        on_golden = on_golden and np.array_equal(sv, g['search_vals'][p])
        cc_ref = g['cc_coeffs'][p] if on_golden else gr.cc_f64(*args)[0]
        ratio = held(cc, cc_ref, cc_hi, '%s pass %d' % (name, p))
        bound = gr.bound(cc_ref, cc_hi)
        best = int(np.argmax(cc_ref))
        runner_up = np.max(np.delete(cc_ref, best))
        print('%s pass %d: chosen %d, reference %d, gap to the runner-up %.3e, bound %.3e, ratio %.3f'
              % (name, p, idx, best, cc_ref[best] - runner_up, bound, ratio))
        if cc_ref[best] - runner_up > 2 * bound:
            assert idx == best, (name, p)
            decided_passes += 1
        else:
            assert float(np.max(cc_hi) - cc_hi[idx]) <= 2 * bound, (name, p)
        if on_golden:
            on_golden = idx == int(g['chosen'][p])
        offset += sv[idx]
    if name == 'NAV_decided':
        # the tolerance may excuse nothing here: the golden's own choice is decided in all five passes
        assert decided_passes == 5 and on_golden
        assert offset == float(g['final_offset'])
        for k in ('lat', 'long', 'elev'):
            assert np.array_equal(getattr(dat, k), g['out_' + k], equal_nan=True), k


def test_interp_to_a_spacing_on_host_data(hip):
    """``gpslib.interp`` with the reference's .mat and a spacing: the attributes bit for bit the reference's, the radargram to
    the re-spacing kernel's bar (1e-12 of the largest expected value)."""
    from conftest import GOLDEN, rel_max
    from impdar_amd.lib import gpslib
    g = golden('NAV_interp')
    dat = radar_of(dict(g, elev=np.zeros(len(g['decday']))))
    dat.elev = None
    dat.data, dat.dist, dat.x_coord, dat.y_coord = g['data'].copy(), g['dist'].copy(), g['x_coord'].copy(), g['y_coord'].copy()
    gpslib.interp([dat], spacing=float(g['spacing']), fn=os.path.join(GOLDEN, 'gps_control.mat'))
    for k in ('lat', 'long', 'elev', 'dist', 'decday'):
        assert np.array_equal(getattr(dat, k), g['out_' + k]), k
    assert dat.tnum == int(g['out_tnum']) and dat.data.shape == g['out_data'].shape
    assert rel_max(dat.data, g['out_data']) < 1e-12


def wide_line(tnum=50, ngps=2400, seed=31):
    """A short line inside a GPS record of +-0.12 days: what an offset search from 0 (+-0.1 days) needs."""
    rng = np.random.default_rng(seed)
    s_trace = np.arange(tnum, dtype=np.float64)
    s_gps = np.sort(rng.uniform(-0.12 * gr.DAY, 0.12 * gr.DAY + tnum, ngps))
    return dict(decday=gr.DECIDED_T0 + s_trace / gr.DAY, lat=gr.track_lat(s_trace - 2.5), long=gr.track_lon(s_trace - 2.5),
                elev=np.full(tnum, 990.0), gps_decday=gr.DECIDED_T0 + s_gps / gr.DAY, gps_lat=gr.track_lat(s_gps),
                gps_long=gr.track_lon(s_gps), gps_elev=gr.track_elev(s_gps), offset=0.0, extrapolate=0)


def test_refusal_and_the_grid_of_offset_zero(hip):
    """A record that does not span the +-0.1 day window of an offset search from 0 raises; one that does is searched on
    the 5001-candidate grid first, then on 1001 candidates around the running offset."""
    g = dict(golden('NAV_decided'), offset=0.0)
    lat0 = g['lat'].copy()
    with pytest.raises(ValueError):
        control(g)
    assert np.array_equal(g['lat'], lat0)
    w = wide_line()
    dat, log = control(w)
    assert np.array_equal(log[0][0], np.linspace(-0.1, 0.1, 5001))
    o = log[0][0][log[0][2]]
    assert o != 0.0 and np.array_equal(log[1][0], np.linspace(-0.1 * abs(o), 0.1 * abs(o), 1001))
    assert dat.lat.shape == (50,) and not np.any(np.isnan(dat.lat))


# ---- command line

def line_file(tmp_path, w, snum=128):
    from impdar_amd import synth
    from impdar_amd.lib.NoInitRadarData import NoInitRadarData
    tnum = len(w['decday'])
    geo = synth.geometry(snum, tnum)
    d = NoInitRadarData(big=True)
    d.data = synth.noise_radargram(snum, tnum, seed=3).astype(np.float32)
    d.snum, d.tnum = snum, tnum
    for k in ('decday', 'lat', 'long', 'elev'):
        setattr(d, k, w[k].copy())
    d.pressure, d.trig = np.zeros(tnum), np.zeros(tnum)
    d.trace_num = np.arange(tnum) + 1.
    d.travel_time, d.dt = geo['travel_time'], geo['dt']
    d.dist = np.arange(tnum) * 1.1e-3
    d.x_coord, d.y_coord = d.dist * 1000., np.zeros(tnum)
    d.trace_int = np.full(tnum, 1.1)
    fn = str(tmp_path / 'line_raw.mat')
    d.save(fn)
    csv = str(tmp_path / 'gps.csv')
    np.savetxt(csv, np.column_stack((w['gps_decday'], w['gps_long'], w['gps_lat'], w['gps_elev'])), fmt='%.17g')
    return d, fn, csv


def test_cli_geolocate_then_interp(hip, tmp_path):
    from impdar_amd.bin import impproc
    from impdar_amd.lib.RadarData import RadarData
    w = wide_line()
    d, fn, csv = line_file(tmp_path, w)
    with patch.object(sys, 'argv', ['impproc', 'geolocate', '--guess', csv, fn]):
        impproc.main()
    r = RadarData(str(tmp_path / 'line_geolocate.mat'))
    want, _ = control(w)
    for k in ('lat', 'long', 'elev'):
        assert np.array_equal(getattr(r, k), getattr(want, k)), k
    assert np.array_equal(r.data, d.data)
    # ... and the re-spacing of its output keeps the track's positions: the elevation is the track's, not the file's 990 m
    with patch.object(sys, 'argv', ['impproc', 'interp', '5', str(tmp_path / 'line_geolocate.mat')]):
        impproc.main()
    r = RadarData(str(tmp_path / 'line_geolocate_interp.mat'))
    assert r.tnum == 11 and r.data.shape == (128, 11)
    assert list(np.asarray(r.flags.interp, dtype=float)) == [1., 5.] and np.all(np.abs(r.elev - 990.0) > 1.0)
