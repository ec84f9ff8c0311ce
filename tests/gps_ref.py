"""The time-offset search of kinematic GPS control restated with NumPy / SciPy (the reference's
``src/impdar/lib/gpslib.py:420-427`` for given candidates), in float64 the reference's way and in ``longdouble``, plus the
decided track of the NAV* fixtures.  What the GPU tests compare against on a box without the reference.

float64: the same ``interp1d`` calls and ``np.corrcoef`` the reference makes; without ``extrapolate`` a trace outside the
shifted record is NaN and counted instead of raising (``bounds_error=False``: the same ``np.interp`` path).
``longdouble``: shifted times, interpolation, means and centred sums all in ``longdouble``, the traces left out being those
the float64 evaluation left out."""
import warnings

import numpy as np
from scipy.interpolate import interp1d

LD = np.longdouble


def track_f64(gps_t, y, t, shift, base, extrapolate):
    """SciPy's float64 interpolation of ``(gps_t + shift + base, y)`` at ``t``, and the out-of-range mask."""
    x = gps_t + shift + base
    with np.errstate(all='ignore'):
        if extrapolate:
            return interp1d(x, y, kind='linear', fill_value='extrapolate')(t), np.zeros(len(t), dtype=bool)
        out = interp1d(x, y, kind='linear', bounds_error=False, fill_value=np.nan)(t)
    return out, (t < x.min()) | (t > x.max())


def _r64(a, b):
    keep = ~np.isnan(a) & ~np.isnan(b)
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        return np.corrcoef(a[keep], b[keep])[0, 1] if keep.sum() > 0 else np.nan


def cc_f64(gps_t, lat, lon, t, rlat, rlon, base, search, extrapolate):
    """``(cc, nout)`` at the candidates ``search``: lines 422-427 of the reference."""
    cc, nout = np.empty(len(search)), np.zeros(len(search), dtype=np.int64)
    for c, s in enumerate(search):
        la, outside = track_f64(gps_t, lat, t, s, base, extrapolate)
        lo, _ = track_f64(gps_t, lon, t, s, base, extrapolate)
        nout[c] = outside.sum()
        cc[c] = _r64(la, rlat) + _r64(lo, rlon)
    return cc, nout


def _track_ld(x, y, t):
    j = (np.searchsorted(x, t, side='right') - 1).clip(0, len(x) - 2)
    with np.errstate(all='ignore'):
        return y[j] + (y[j + 1] - y[j]) / (x[j + 1] - x[j]) * (t - x[j])


def _r_ld(a, b, keep):
    if keep.sum() < 2:
        return LD(np.nan)
    a, b = a[keep], b[keep]
    da, db = a - a.sum() / LD(len(a)), b - b.sum() / LD(len(b))
    with np.errstate(all='ignore'):
        return np.clip((da * db).sum() / np.sqrt((da * da).sum() * (db * db).sum()), -1, 1)


def cc_ld(gps_t, lat, lon, t, rlat, rlon, base, search, extrapolate):
    """``cc`` at the candidates in ``longdouble`` (returned as ``longdouble``)."""
    g, la_g, lo_g, tt = gps_t.astype(LD), lat.astype(LD), lon.astype(LD), t.astype(LD)
    ra, ro = rlat.astype(LD), rlon.astype(LD)
    cc = np.empty(len(search), dtype=LD)
    for c, s in enumerate(search):
        x64 = gps_t + s + base
        skip = np.isnan(t) if extrapolate else (np.isnan(t) | (t < x64.min()) | (t > x64.max()))
        x = (g + LD(s)) + LD(base)
        la, lo = _track_ld(x, la_g, tt), _track_ld(x, lo_g, tt)
        cc[c] = _r_ld(la, ra, ~skip & ~np.isnan(la) & ~np.isnan(ra)) + _r_ld(lo, ro, ~skip & ~np.isnan(lo) & ~np.isnan(ro))
    return cc


def bound(cc_ref, cc_hi):
    """max |cc_ref - cc_hi| over the candidates where both are numbers: the reference's own distance from the exact value."""
    d = np.abs(cc_ref.astype(LD) - cc_hi)
    d = d[~np.isnan(d)]
    return float(d.max()) if d.size else 0.0


# ---- the decided track: 300 traces at 1 s, 3000 fixes at sorted uniform times over [-300 s, 600 s] around the line, no trend;
# the radar's own fixes are the track 2.5 s earlier plus 2e-6 degrees of noise; the search starts from 3 s
DAY = 86400.0
DECIDED_T0 = 100.25                  # decimal day of the first trace
DECIDED_START = 3.0 / DAY


def track_lat(s):
    return -79.0 + 2e-4 * np.sin(s / 37.0) + 1e-4 * np.sin(s / 11.0 + 1.0)


def track_lon(s):
    return 250.0 + 3e-4 * np.cos(s / 53.0) + 1e-4 * np.sin(s / 7.0)


def track_elev(s):
    return 1000.0 + 5.0 * np.sin(s / 90.0)


def decided(tnum=300, ngps=3000, seed=20):
    """``dict(decday, lat, long, elev)`` of the radar file and ``gps_decday, gps_lat, gps_long, gps_elev`` of the track."""
    rng = np.random.default_rng(seed)
    s_trace = np.arange(tnum, dtype=np.float64)
    s_gps = np.sort(rng.uniform(-300.0, 600.0, ngps))
    out = {'decday': DECIDED_T0 + s_trace / DAY,
           'lat': track_lat(s_trace - 2.5) + 2e-6 * rng.standard_normal(tnum),
           'long': track_lon(s_trace - 2.5) + 2e-6 * rng.standard_normal(tnum),
           'elev': np.full(tnum, 990.0),
           'gps_decday': DECIDED_T0 + s_gps / DAY,
           'gps_lat': track_lat(s_gps), 'gps_long': track_lon(s_gps), 'gps_elev': track_elev(s_gps)}
    return out


# ---- the inputs of the kernel's shape sweep
SWEEP = ((1, 2, 1), (2, 2, 3), (3, 5, 7), (255, 64, 5), (256, 64, 5), (257, 64, 5), (300, 3000, 1001), (1000, 17, 5001))


def sweep_case(tnum, ngps, ncand, variant='plain'):
    """A line of ``tnum`` traces inside a record of ``ngps`` fixes (one pair of them duplicates where ngps >= 4) and ``ncand``
    candidates.  As far as ``tnum`` allows, trace times sit exactly on x[0], on x[ngps - 1] and on an interior fix of the
    probed candidate ``probe``, one ulp outside each end, and one is NaN; a few radar positions are NaN.  ``variant``:
    'allnan' (no radar latitude) or 'onepair' (one valid pair of longitudes)."""
    rng = np.random.default_rng(1000 * tnum + ngps + ncand)
    s_gps = np.sort(rng.uniform(0.0, 400.0, ngps))
    if ngps >= 4:
        s_gps[ngps // 2 + 1] = s_gps[ngps // 2]
    gps_t = DECIDED_T0 + s_gps / DAY
    base = 2.0 / DAY
    search = np.linspace(-0.5 / DAY, 0.5 / DAY, ncand) if ncand > 1 else np.array([0.25 / DAY])
    probe = ncand // 2
    x = gps_t + search[probe] + base
    t = np.sort(rng.uniform(x[0] + 1.0 / DAY, x[-1] - 1.0 / DAY, tnum))
    specials = [x[0], x[-1], x[ngps // 3], np.nextafter(x[0], -np.inf), np.nextafter(x[-1], np.inf), np.nan]
    where = rng.permutation(tnum)[:len(specials)]
    for k, j in enumerate(where):
        t[j] = specials[k]
    s_t = (np.where(np.isnan(t), 0.0, t) - DECIDED_T0) * DAY
    rlat = track_lat(s_t - 2.0) + 2e-6 * rng.standard_normal(tnum)
    rlon = track_lon(s_t - 2.0) + 2e-6 * rng.standard_normal(tnum)
    if tnum >= 16:
        rlat[rng.permutation(tnum)[:3]] = np.nan
        rlon[rng.permutation(tnum)[:2]] = np.nan
    if variant == 'allnan':
        rlat[:] = np.nan
    elif variant == 'onepair':
        rlon[np.arange(tnum) != tnum // 2] = np.nan
    return dict(gps_t=gps_t, lat=track_lat(s_gps), lon=track_lon(s_gps), t=t, rlat=rlat, rlon=rlon, base=base, search=search,
                probe=probe)
