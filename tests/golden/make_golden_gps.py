#!/usr/bin/env python3
"""Generate the ``NAV_*`` golden vectors (kinematic GPS control) by running the REFERENCE's ``gpslib.kinematic_gps_control``,
``kinematic_gps_mat``, ``kinematic_gps_csv`` and ``interp`` (``src/impdar/lib/gpslib.py:348-595``) -- imported, never
copied -- on its own ``gps_control.mat`` / ``gps_control.csv`` (copied here as data fixtures) and on the decided track of
``tests/gps_ref.py``.

Stored per case: the radar file's ``decday, lat, long, elev`` before the call, the track ``gps_decday, gps_lat, gps_long,
gps_elev`` (where it does not come from a file), the arguments ``offset, extrapolate, guess, gaps``, the result ``out_lat,
out_long, out_elev`` (and ``out_dist, out_tnum, out_data`` after ``interp``), and for a search its five passes:
``search_vals`` and ``cc_coeffs`` (5, n) -- what the reference handed to ``np.linspace`` and ``np.argmax``, recorded through
its own ``np`` name while it runs -- ``chosen`` (5,) and ``final_offset``.  The script also prints, per pass of the decided
cases, the gap from the best candidate to the runner-up and the reference's distance from the ``longdouble`` evaluation.

Only runs where the reference is installed; the committed files are what travels.

Usage:  python tests/golden/make_golden_gps.py REFERENCE_SRC            (the directory that holds impdar/)
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import gps_ref as gr          # noqa: E402


class RecordingNumpy(object):
    """Stands in for the reference's ``np``: every ``linspace`` and ``argmax`` of the search is kept."""

    def __init__(self):
        self.search_vals, self.cc_coeffs, self.chosen = [], [], []

    def __getattr__(self, name):
        return getattr(np, name)

    def linspace(self, *args):
        out = np.linspace(*args)
        self.search_vals.append(out.copy())
        return out

    def argmax(self, a):
        i = np.argmax(a)
        self.cc_coeffs.append(np.array(a, copy=True))
        self.chosen.append(int(i))
        return i


def radar(ref_noinit, d):
    dat = ref_noinit(big=True)
    dat.tnum = len(d['decday'])
    for k in ('decday', 'lat', 'long', 'elev'):
        setattr(dat, k, d[k].copy())
    return dat


def run(ref, dat, call, **kw):
    """One call of the reference with its ``np`` recorded; the fixture's common entries."""
    out = {k: np.array(getattr(dat, k), dtype=np.float64, copy=True) for k in ('decday', 'lat', 'long')}
    out['elev'] = np.full(dat.tnum, np.nan) if dat.elev is None else np.array(dat.elev, dtype=np.float64, copy=True)
    rec = RecordingNumpy()
    ref.np = rec
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            call()
    finally:
        ref.np = np
    out.update(out_lat=dat.lat, out_long=dat.long, out_elev=dat.elev)
    out.update(offset=float(kw.get('offset', 0.0)), extrapolate=int(kw.get('extrapolate', False)), guess=int(kw.get('guess', False)),
               gaps=int(kw.get('gaps', False)))
    if rec.chosen:
        out.update(search_vals=np.array(rec.search_vals), cc_coeffs=np.array(rec.cc_coeffs), chosen=np.array(rec.chosen))
        off = out['offset']
        for sv, i in zip(rec.search_vals, rec.chosen):
            off += sv[i]
        out['final_offset'] = off
    return out


def report(name, d, g):
    order = np.argsort(d['gps_decday'], kind='stable')
    d = {k: v[order] for k, v in d.items()}
    for p in range(len(g['chosen'])):
        cc, base = g['cc_coeffs'][p], g['offset'] + sum(g['search_vals'][q][g['chosen'][q]] for q in range(p))
        top = np.sort(cc[~np.isnan(cc)])[-2:]
        near = np.argsort(cc)[-8:]
        hi = gr.cc_ld(d['gps_decday'], d['gps_lat'], d['gps_long'] % 360, g['decday'], g['lat'], g['long'] % 360, base,
                      g['search_vals'][p][near], bool(g['extrapolate']))
        print('%s pass %d: offset %.4f s -> index %d, gap to the runner-up %.3e, reference - longdouble %.3e'
              % (name, p, base * gr.DAY, g['chosen'][p], top[1] - top[0], gr.bound(cc[near], hi)))


def main(src):
    sys.path.insert(0, src)
    from impdar.lib import gpslib as ref
    from impdar.lib.NoInitRadarData import NoInitRadarData
    assert not ref.conversions_enabled, 'the fixtures are written for a reference without GDAL'
    mat, csv = os.path.join(HERE, 'gps_control.mat'), os.path.join(HERE, 'gps_control.csv')
    cases = {}

    dat = NoInitRadarData(big=True)
    cases['NAV_mat'] = run(ref, dat, lambda: ref.kinematic_gps_mat(dat, mat))
    dat = NoInitRadarData(big=True)
    cases['NAV_csv'] = run(ref, dat, lambda: ref.kinematic_gps_csv([dat], csv, offset=0.25, extrapolate=True), offset=0.25, extrapolate=True)

    d = gr.decided()
    track = {k: d[k] for k in ('gps_decday', 'gps_lat', 'gps_long', 'gps_elev')}
    args = (d['gps_lat'], d['gps_long'], d['gps_elev'], d['gps_decday'])
    dat = radar(NoInitRadarData, d)
    cases['NAV_decided'] = dict(run(ref, dat, lambda: ref.kinematic_gps_control(dat, *args, offset=gr.DECIDED_START), offset=gr.DECIDED_START,
                                   guess=True), **track)
    dat = radar(NoInitRadarData, d)
    cases['NAV_noguess'] = dict(run(ref, dat, lambda: ref.kinematic_gps_control(dat, *args, offset=2.5 / gr.DAY, guess_offset=False),
                                   offset=2.5 / gr.DAY), **track)

    # the track shuffled and shorter than the line: fixes over [20 s, 280 s] only, so both ends are extrapolated
    s = d['gps_decday'] - gr.DECIDED_T0
    keep = np.random.default_rng(5).permutation(np.where((s > 20.0 / gr.DAY) & (s < 280.0 / gr.DAY))[0])
    short = {k: d[k][keep] for k in track}
    sargs = (short['gps_lat'], short['gps_long'], short['gps_elev'], short['gps_decday'])
    dat = radar(NoInitRadarData, d)
    cases['NAV_extrap'] = dict(run(ref, dat, lambda: ref.kinematic_gps_control(dat, *sargs, offset=gr.DECIDED_START, extrapolate=True),
                                  offset=gr.DECIDED_START, extrapolate=True, guess=True), **short)

    # old_gps_gaps: no fix between 100 s and 140 s, some of the radar's own positions 0 (no fix): host only
    hole = np.where((s < 100.0 / gr.DAY) | (s > 140.0 / gr.DAY))[0]
    gap = {k: d[k][hole] for k in track}
    gargs = (gap['gps_lat'], gap['gps_long'], gap['gps_elev'], gap['gps_decday'])
    dg = {k: d[k].copy() for k in ('decday', 'lat', 'long', 'elev')}
    dg['lat'][[3, 120]] = 0.0
    dg['long'][[3, 121]] = 0.0
    dat = radar(NoInitRadarData, dg)
    cases['NAV_gaps'] = dict(run(ref, dat, lambda: ref.kinematic_gps_control(dat, *gargs, offset=2.5 / gr.DAY, guess_offset=False,
                                                                             old_gps_gaps=True), offset=2.5 / gr.DAY, gaps=True), **gap)

    # interp to a spacing on host data, the positions from the .mat first
    dat = NoInitRadarData(big=True)
    dat.x_coord, dat.y_coord = np.arange(dat.tnum) * 1000.0, np.zeros(dat.tnum)
    dat.dist = np.arange(dat.tnum) * 1.0
    dat.data = np.random.default_rng(9).standard_normal(dat.data.shape)
    g = dict(data=dat.data.copy(), x_coord=dat.x_coord.copy(), y_coord=dat.y_coord.copy(), dist=dat.dist.copy(), spacing=700.0)
    g.update(run(ref, dat, lambda: ref.interp([dat], spacing=700.0, fn=mat)))
    g.update(out_data=dat.data, out_dist=dat.dist, out_tnum=dat.tnum, out_decday=dat.decday)
    cases['NAV_interp'] = g

    for name, g in cases.items():
        np.savez_compressed(os.path.join(HERE, name + '.npz'), **g)
        print(name, os.path.getsize(os.path.join(HERE, name + '.npz')), 'bytes')
    report('NAV_decided', track, cases['NAV_decided'])
    report('NAV_extrap', short, cases['NAV_extrap'])
    # the restatement is the reference: cc at the recorded candidates of the first and the last pass
    for name, tr in (('NAV_decided', track), ('NAV_extrap', short)):
        g = cases[name]
        order = np.argsort(tr['gps_decday'], kind='stable')
        for p in (0, 4):
            base = g['offset'] + sum(g['search_vals'][q][g['chosen'][q]] for q in range(p))
            cc, nout = gr.cc_f64(tr['gps_decday'][order], tr['gps_lat'][order], (tr['gps_long'] % 360)[order], g['decday'], g['lat'],
                                 g['long'] % 360, base, g['search_vals'][p], bool(g['extrapolate']))
            print('%s pass %d: restatement == reference bit for bit: %s' % (name, p, np.array_equal(cc, g['cc_coeffs'][p], equal_nan=True)))


if __name__ == '__main__':
    main(sys.argv[1])
