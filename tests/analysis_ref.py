"""The growing-window search of the attenuation methods 3 and 6b restated with NumPy from its rules (the reference's
``analysis/attenuation.py``), in float64 with the reference's own passes and in ``longdouble``, plus the synthetic pick of
the ``YA_*`` fixtures.  What the GPU tests compare against on a box without the reference.

A centre (a trace of method 3, a depth of method 6b) walks nested windows.  At each window every rate ``N = Ns[j]`` gets
``pa = pc + 2 z N`` and ``C[j] = |sum (z - mean z)(pa - mean pa) / (sqrt(sum (z - mean z)^2) sqrt(sum (pa - mean pa)^2))|``;
``Cm = min C``; if ``Cm < Cw`` and ``C[Ns == 0] > Cw`` then ``Nh = max Ns[C < Cw] - min Ns[C < Cw]`` (halved for 6b); the
walk stops when ``Nh <= Nh_target`` or the next window leaves the record, and reports the rate at the minimum of the last
window visited and the width after the last increment.

``INDEX`` (method 3): the window of width ``win`` around trace ``tr`` of the NaN-free pick is ``[tr - win//2, tr + win//2)``,
visited while ``win//2 <= tr`` and ``win//2 <= n - tr``; sums with Python's ``sum``, as the reference has them.
``DEPTH`` (method 6b): the pairs with ``|Z - d| < win/2`` in float64, visited while ``d - win/2 >= min Z`` and
``d + win/2 <= max Z``; ``win += win_step`` by repeated addition; ``nansum`` / ``nanmean`` / ``nanmin``."""
import json
import warnings

import numpy as np

LD = np.longdouble
INDEX, DEPTH = 0, 1


def recipe(tnum, seed=0):
    """The pick of the decided fixtures: depth in metres and corrected power (linear) per trace."""
    rng = np.random.default_rng(seed)
    j = np.arange(tnum, dtype=np.float64)
    z = 1500. + 300. * np.sin(j / 37.) + 120. * np.sin(j / 11. + 1.) + 2. * rng.standard_normal(tnum)
    db = -40. - 2. * (12. + 4. * np.sin(j / 150.)) * z / 1000. + 0.5 * rng.standard_normal(tnum)
    return z, 10. ** (db / 10.)


def prepared(z_m, power):
    """What both methods do first: dB, the pairs where both are numbers, kilometres when any depth exceeds 10."""
    pc = 10. * np.log10(power)
    keep = ~np.isnan(pc) & ~np.isnan(z_m)
    z, pc = z_m[keep], pc[keep]
    if np.any(z > 10.):
        z = z / 1000.
    return z, pc


def members(flavour, z, centre, win):
    """The indices of the window, or None where the walk may not visit it."""
    if flavour == INDEX:
        if not (win // 2 <= centre and win // 2 <= len(z) - centre):
            return None
        return np.arange(centre - win // 2, centre + win // 2)
    if not (centre - win / 2 >= np.nanmin(z) and centre + win / 2 <= np.nanmax(z)):
        return None
    return np.argwhere(abs(z - centre) < win / 2)[:, 0]


def c_row(flavour, zw, pw, ns):
    """``C`` of one window in float64, pass by pass as the reference computes it."""
    out = np.empty(len(ns))
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        if flavour == INDEX:
            sum2 = np.sqrt(sum((zw - np.mean(zw)) ** 2.))
            for j, nj in enumerate(ns):
                pa = pw + 2. * zw * nj
                sum1 = sum((zw - np.mean(zw)) * (pa - np.mean(pa)))
                sum3 = np.sqrt(sum((pa - np.mean(pa)) ** 2.))
                out[j] = abs(sum1 / (sum2 * sum3))
            return out
        zw, pw = zw[:, None], pw[:, None]
        sum2 = np.sqrt(np.nansum((zw - np.nanmean(zw)) ** 2.))
        for j in range(len(ns)):
            pa = pw + 2. * zw * ns[j]
            sum1 = np.nansum((zw - np.nanmean(zw)) * (pa - np.nanmean(pa)))
            sum3 = np.sqrt(np.nansum((pa - np.nanmean(pa)) ** 2.))
            out[j] = np.nan if np.any(np.isnan([sum1, sum2, sum3])) else abs(sum1 / (sum2 * sum3))
    return out


def c_row_ld(zw, pw, ns):
    """``C`` of one window with every operation in ``longdouble``."""
    z, p, n = zw.astype(LD), pw.astype(LD), ns.astype(LD)
    dz = z - z.sum() / LD(len(z))
    pa = p[None, :] + LD(2) * z[None, :] * n[:, None]
    dpa = pa - (pa.sum(axis=1) / LD(len(z)))[:, None]
    with np.errstate(all='ignore'):
        return np.abs((dz[None, :] * dpa).sum(axis=1) / (np.sqrt((dz * dz).sum()) * np.sqrt((dpa * dpa).sum(axis=1))))


def walk(flavour, z, pc, ns, cw, nh_target, win_init, win_step, centre):
    """One centre: ``rows`` (the float64 ``C`` of every window visited), ``windows`` (their indices), ``nm`` (the rates at the
    minimum of the last window, an array; None where no window was visited) and ``win``."""
    win, nh, nm, rows, windows = win_init, nh_target + 1., None, [], []
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        while nh > nh_target:
            at = members(flavour, z, centre, win)
            if at is None:
                break
            cs = c_row(flavour, z[at], pc[at], ns)
            rows.append(cs)
            windows.append(at)
            cm = np.min(cs) if flavour == INDEX else np.nanmin(cs)
            nm = ns[cs == cm]
            if cm < cw and cs[ns == 0] > cw:
                nh = np.max(ns[cs < cw]) - np.min(ns[cs < cw])
                if flavour == DEPTH:
                    nh = nh / 2.
            win += win_step
    return dict(rows=rows, windows=windows, nm=nm, win=win)


def search(flavour, z, pc, ns, cw, nh_target, win_init, win_step, centres, count=None):
    """The reference's loop over the centres: ``(rates, widths)``, one per centre (``count``: the length of the arrays of
    method 3, with zeros where the loop does not go).  A centre that visits no window takes the rate left over from the
    centre before (``UnboundLocalError`` at the first); no single rate at the minimum: ``ValueError``."""
    if not np.any(ns == 0):
        raise ValueError('no rate 0 in Ns')
    rates, widths = np.zeros(count if count is not None else len(centres)), np.zeros(count if count is not None else len(centres))
    left = None
    for b, centre in enumerate(centres):
        w = walk(flavour, z, pc, ns, cw, nh_target, win_init, win_step, centre)
        left = w['nm'] if w['nm'] is not None else left
        if left is None:
            raise UnboundLocalError('the first centre visits no window')
        at = centre if flavour == INDEX else b
        if left.size != 1:
            raise ValueError('no single rate at the minimum of the last window')
        rates[at] = left[0]
        widths[at] = w['win'] if flavour == INDEX else w['win'] * 1000.
    return rates, widths


def margin(rows, cw):
    """A centre's decision margin: the smaller of the gap from the minimum ``C`` to its runner-up and of any ``|C - Cw|``,
    over the windows it visited (inf for none, or for a single rate and no threshold nearby)."""
    m = np.inf
    for cs in rows:
        s = np.sort(cs)
        if len(s) > 1:
            m = min(m, float(s[1] - s[0]))
        m = min(m, float(np.min(np.abs(cs - cw))))
    return m


def distance(rows, rows_ld):
    """max |C - C_longdouble| over the given rows."""
    d = 0.0
    for a, b in zip(rows, rows_ld):
        d = max(d, float(np.max(np.abs(a.astype(LD) - b))))
    return d


def synthetic(n, seed, relief=1.0):
    """A smaller pick for the shape tests: prepared ``(z km, pc dB)`` of ``n`` traces with a rate of about 12 dB/km."""
    rng = np.random.default_rng(seed)
    j = np.arange(n, dtype=np.float64)
    z = 1.5 + relief * (0.3 * np.sin(j / 7.) + 0.1 * np.sin(j / 3. + 1.)) + 0.002 * rng.standard_normal(n)
    pc = -40. - 2. * 12. * z + 0.5 * rng.standard_normal(n)
    return z, pc


# ---- the YA_* fixtures: a call of one public function, recorded

class Bag(object):
    """A bare object: the functions read attributes of ``dat``, ``dat.picks`` and ``dat.flags`` and nothing else."""


def make_dat(g):
    """The radar object of a fixture: ``picks_<attribute>`` arrays become ``dat.picks.<attribute>`` (copies), and so on."""
    dat, dat.picks, dat.flags = Bag(), Bag(), Bag()
    for k in ('z', 'time', 'power', 'corrected_power'):
        if 'picks_' + k in g:
            setattr(dat.picks, k, np.array(g['picks_' + k], copy=True))
    dat.tnum = int(g['tnum'])
    for k in ('elev', 'trace_int'):
        if k in g:
            setattr(dat, k, np.array(g[k], copy=True))
    if 'flags_interp' in g:
        dat.flags.interp = np.array(g['flags_interp'], copy=True)
    return dat


def run_call(mods, g):
    """Run the call a fixture describes -- ``g['call']``: JSON ``{mod, fn, args, kwargs}``, a string ``"@key"`` standing for a
    fresh copy of the array ``g[key]`` -- on the modules ``mods`` (name -> module).  Returns what came of it as a dict:
    ``out0, out1, ...`` (the returned values), ``after_picks_z`` / ``after_picks_corrected_power`` (the object's arrays after
    the call), ``after@key`` (the caller's array arguments after the call), or ``raised`` (the exception's type name)."""
    spec = json.loads(str(g['call']))
    dat = make_dat(g)
    held = {}

    def value(v):
        if isinstance(v, str) and v.startswith('@'):
            held[v] = np.array(g[v[1:]], copy=True)
            return held[v]
        return v

    args = [value(v) for v in spec.get('args', [])]
    kwargs = {k: value(v) for k, v in spec.get('kwargs', {}).items()}
    fn = getattr(mods[spec['mod']], spec['fn'])
    first = [] if spec.get('nodat') else [dat]
    out = {}
    try:
        with warnings.catch_warnings(), np.errstate(all='ignore'):
            warnings.simplefilter('ignore')
            res = fn(*(first + args), **kwargs)
    except Exception as exc:            # the kind is what a fixture records
        return dict(raised=type(exc).__name__)
    if res is not None:
        for k, r in enumerate(res if isinstance(res, tuple) else (res,)):
            out['out%d' % k] = np.asarray(r)
    for k in ('z', 'corrected_power'):
        if k in vars(dat.picks):
            out['after_picks_' + k] = np.asarray(getattr(dat.picks, k))
    for k, v in held.items():
        out['after' + k] = v
    return out


def layers(npick, tnum, seed, flat=False):
    """``npick`` picked layers of ``tnum`` traces: depth in metres (npick, tnum), power and corrected power (linear), a few NaN."""
    rng = np.random.default_rng(seed)
    j = np.arange(tnum, dtype=np.float64)
    base = 250. + 260. * np.arange(npick, dtype=np.float64)[:, None]
    z = base + (0. if flat else 1.) * (60. * np.sin(j / 41. + np.arange(npick)[:, None]) + 1.5 * rng.standard_normal((npick, tnum)))
    z = z + np.zeros((npick, tnum))
    db = -35. - 2. * (9. + 6. * z / 1800.) * z / 1000. + 0.6 * rng.standard_normal((npick, tnum))
    cp = 10. ** (db / 10.)
    for a in (z, cp):
        a[rng.integers(0, npick, 7), rng.integers(0, tnum, 7)] = np.nan
    return z, cp / (2. * z) ** 2., cp
