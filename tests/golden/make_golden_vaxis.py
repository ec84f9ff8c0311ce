#!/usr/bin/env python3
"""Generate the ``X*`` golden vectors (steps that change the sample axis) by running the REFERENCE's ``crop``,
``nmo`` and ``elev_correct`` (``src/impdar/lib/RadarData/_RadarDataProcessing.py:50-337, 585-632``, imported --
never copied) on small synthetic radargrams.  Every file stores the inputs, every attribute the step changes and
the flags; the error cases store the reference's exception type and message.  Only runs where the reference is
installed; the committed ``*.npz`` files are what travels.

Usage:  python tests/golden/make_golden_vaxis.py
"""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference/src')

from impdar.lib.NoInitRadarData import NoInitRadarData          # noqa: E402

VERS = dict(numpy_version=np.__version__, scipy_version=scipy.__version__)
SNUM, TNUM, DT = 200, 60, 1e-8


def radargram(dtype, seed, snum=SNUM, tnum=TNUM, amp=1.0):
    rng = np.random.default_rng(seed)
    t = np.arange(snum)[:, None]
    x = np.arange(tnum)[None, :]
    data = 0.3 * rng.standard_normal((snum, tnum))
    data += 4.0 * np.exp(-0.5 * ((t - 12) / 2.0) ** 2) * np.cos(0.9 * t)       # direct wave
    data += 1.5 * np.exp(-0.5 * ((t - (60 + 0.8 * x)) / 1.5) ** 2)             # dipping reflector
    data *= amp
    if np.issubdtype(dtype, np.integer):
        return np.round(data).astype(dtype)
    return data.astype(dtype)


def make_dat(data, t0_us=0.0, trig=None, elev=None):
    d = NoInitRadarData(big=True)
    d.data = data.copy()
    d.snum, d.tnum = data.shape
    d.dt = DT
    d.travel_time = t0_us + np.arange(d.snum) * DT * 1e6
    d.trig = np.zeros(d.tnum) if trig is None else trig
    d.elev = elev
    return d


def state(d, prefix):
    out = {prefix + 'data': d.data.copy(), prefix + 'travel_time': np.array(d.travel_time), prefix + 'snum': d.snum,
           prefix + 'trig': np.array(d.trig), prefix + 'flags_crop': np.array(d.flags.crop, dtype=np.float64),
           prefix + 'flags_nmo': np.array(d.flags.nmo, dtype=np.float64), prefix + 'flags_elev': d.flags.elev}
    if d.nmo_depth is not None:
        out[prefix + 'nmo_depth'] = np.array(d.nmo_depth)
    return out


def save(name, **arrs):
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **arrs, **VERS)
    print('wrote', path, os.path.getsize(path), 'bytes')


def quiet(fn, *a, **k):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        fn(*a, **k)
    return buf.getvalue()


def firn_column():
    depth = np.linspace(0., 120., 49)
    rho = 917. - (917. - 380.) * np.exp(-depth / 28.)
    return depth, rho


def nmo_case(name, dtype, seed, ant_sep, amp=1.0, profile=False, **kw):
    d = make_dat(radargram(dtype, seed, amp=amp))
    extra = {}
    call = dict(kw)
    if profile:
        depth, rho = firn_column()
        extra.update(profile_depth=depth, profile_rho=rho)
        tmp = tempfile.NamedTemporaryFile('w', suffix='.csv', delete=False)
        np.savetxt(tmp, np.column_stack((depth, rho)), delimiter=',')
        tmp.close()
        call['rho_profile'] = tmp.name
    before = state(d, 'in_')
    stdout = quiet(d.nmo, ant_sep, **call)
    if profile:
        os.unlink(call['rho_profile'])
    save(name, kind='nmo', dt=DT, ant_sep=ant_sep, uice=kw.get('uice', 1.69e8), uair=kw.get('uair', 3.0e8),
         const_firn_offset=np.nan if kw.get('const_firn_offset') is None else kw['const_firn_offset'],
         const_sample=bool(kw.get('const_sample', False)), has_profile=profile, stdout=stdout, **extra, **before,
         **state(d, 'out_'))


def crop_case(name, dtype, seed, calls, with_nmo=False, trig=None, amp=1.0):
    """``calls``: a list of (lim, kwargs) applied one after the other; the state after each is stored."""
    d = make_dat(radargram(dtype, seed, amp=amp), trig=trig)
    if with_nmo:
        d.nmo_depth = d.travel_time / 2. * 1.69e8 * 1.0e-6
    arrs = dict(kind='crop', dt=DT, ncalls=len(calls), **state(d, 'in_'))
    out = ''
    for k, (lim, kw) in enumerate(calls):
        out += quiet(d.crop, lim, **kw)
        arrs.update(state(d, 'out%d_' % k))
        arrs['call%d_lim' % k] = lim
        for key in ('top_or_bottom', 'dimension'):
            arrs['call%d_%s' % (k, key)] = kw.get(key, 'top' if key == 'top_or_bottom' else 'snum')
        arrs['call%d_rezero' % k] = kw.get('rezero', True)
        arrs['call%d_zero_trig' % k] = kw.get('zero_trig', True)
    save(name, stdout=out, **arrs)


def elev_case(name, dtype, seed, elev, ant_sep=60.):
    d = make_dat(radargram(dtype, seed), elev=elev)
    quiet(d.nmo, ant_sep)
    arrs = dict(kind='elev', dt=DT, elev=elev, **state(d, 'in_'))
    quiet(d.elev_correct)
    save(name, elevation=d.elevation, **arrs, **state(d, 'out_'))


def errors():
    labels, types, messages = [], [], []

    def record(label, fn):
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                fn()
        except Exception as e:                                       # noqa: BLE001 -- recording what it raises
            labels.append(label)
            types.append(type(e).__name__)
            messages.append(str(e))
        else:
            raise AssertionError('the reference accepted ' + label)
    data = radargram(np.float64, 50)
    record('nmo_range', lambda: make_dat(data, t0_us=0.2).nmo(60.))
    record('nmo_trig', lambda: make_dat(data, trig=np.full(TNUM, 3.)).nmo(60.))
    record('crop_top_or_bottom', lambda: make_dat(data).crop(10, top_or_bottom='side'))
    record('crop_dimension', lambda: make_dat(data).crop(10, dimension='dist'))
    record('crop_bottom_pretrig', lambda: make_dat(data).crop(10, top_or_bottom='bottom', dimension='pretrig'))
    record('elev_without_nmo', lambda: make_dat(data, elev=np.zeros(TNUM)).elev_correct())
    save('XZ_errors', label=np.array(labels), exc_type=np.array(types), message=np.array(messages), data=data, dt=DT)


def main():
    nmo_case('XA_nmo_f64_sep0', np.float64, 1, 0.)
    nmo_case('XB_nmo_f64_sep60', np.float64, 2, 60.)
    nmo_case('XC_nmo_f32_sep60', np.float32, 3, 60.)
    nmo_case('XD_nmo_int16_sep160', np.int16, 4, 160., amp=300.)
    nmo_case('XE_nmo_f32_sep0', np.float32, 5, 0.)
    nmo_case('XF_nmo_f64_sep160_uice_offset', np.float64, 6, 160., uice=1.8e8, const_firn_offset=7.5)
    nmo_case('XG_nmo_f64_profile', np.float64, 7, 60., profile=True)
    nmo_case('XH_nmo_f32_profile_const_sample', np.float32, 8, 60., profile=True, const_sample=True)
    top, bot = dict(top_or_bottom='top'), dict(top_or_bottom='bottom')
    for k, dim, lim_t, lim_b in (('I', 'snum', 17, 150), ('J', 'twtt', 0.33, 1.5), ('K', 'depth', 21.0, 110.0)):
        crop_case('X%s_crop_%s_f64' % (k, dim), np.float64, 10 + ord(k),
                  [(lim_t, dict(top, dimension=dim)), (lim_b, dict(bot, dimension=dim))], with_nmo=(dim != 'twtt'))
    crop_case('XL_crop_depth_no_nmo_f32', np.float32, 30, [(21.0, dict(top, dimension='depth'))])
    crop_case('XM_crop_no_rezero_no_zero_trig_int16', np.int16, 31, [(20, dict(top, rezero=False, zero_trig=False))],
              trig=np.full(TNUM, 25.), amp=300.)
    crop_case('XN_crop_pretrig_scalar_f64', np.float64, 32, [(0, dict(top, dimension='pretrig'))], trig=13)
    rng = np.random.default_rng(33)
    crop_case('XO_crop_pretrig_vector_f64', np.float64, 33, [(0, dict(top, dimension='pretrig'))],
              trig=(8 + rng.integers(0, 9, TNUM)).astype(float))
    crop_case('XP_crop_pretrig_vector_f32', np.float32, 34, [(0, dict(top, dimension='pretrig'))],
              trig=(5 + rng.integers(0, 4, TNUM)).astype(int))
    x = np.arange(TNUM)
    elev_case('XQ_elev_hill_f64', np.float64, 40, 1200. + 6. * np.sin(x / 9.) - 0.05 * x)
    elev_case('XR_elev_hill_f32', np.float32, 41, 900. + 3. * np.cos(x / 5.))
    elev_case('XS_elev_flat_f64', np.float64, 42, np.full(TNUM, 1000.))
    errors()


if __name__ == '__main__':
    main()
