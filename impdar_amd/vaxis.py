"""Host side of the steps that change the sample axis of a radargram: ``crop``, ``nmo`` (with
``constant_sample_depth_spacing``) and ``elev_correct``.  Everything that is O(snum) or O(tnum) -- the move-out
times, the velocity profile of a firn column, the knot search of the interpolation, the crop index, the
per-trace shifts -- is NumPy here, as in the reference; everything that touches the (snum, tnum) radargram runs
in ``csrc/vaxis.hip`` through the C ABI, on host buffers or on an array that is already resident in HBM.

Reference: ``src/impdar/lib/RadarData/_RadarDataProcessing.py:50-61, 64-236, 238-337, 585-632``.
"""
import ctypes as C

import numpy as np

from . import _hip
from .preproc import _check_range


# ------------------------------------------------------------------------------------------------ move-out
def firn_permittivity(rhof, rhoi=917., epsi_real=3.12, epsi_imag=-9.5):
    """Relative permittivity of firn of density ``rhof`` (kg/m3) by the DECOMP mixing formula of Wilhelms (2005,
    GRL 32, L16501): the cube root of the permittivity is linear in the volume fraction of ice,
    ``eps_f**(1/3) = 1 + (rhof / rhoi) * (eps_i**(1/3) - 1)``, with ``eps_i = epsi_real - 1j * epsi_imag``."""
    root_i = (epsi_real - 1j * epsi_imag) ** (1 / 3.)
    return (1. + (rhof / rhoi) * (root_i - 1)) ** 3.


def load_rho_profile(rho_profile):
    """(depth, density) columns of a csv density profile (:118-124)."""
    try:
        table = np.genfromtxt(rho_profile, delimiter=',')
        return table[:, 0], table[:, 1]
    except IndexError:
        raise IndexError('Cannot load the depth-density profile')


def _rms_velocity_above(t_us, u_guess, grid_depth, grid_u2, tol):
    """RMS velocity of the column above the reflector a two-way time ``t_us`` (microseconds) reaches.  The depth
    depends on the velocity and the velocity on the depth, so the pair is found by fixed-point rounds from the
    depth at ``u_guess``: at least five of them, then until the depth moves by no more than ``tol`` metres."""
    def reach(u):
        return t_us / 2. * u * 1.0e-6
    depth = reach(u_guess)
    rounds = 0
    while True:
        above = np.searchsorted(grid_depth, depth, side='right')        # grid points at or above the reflector
        u_rms = np.sqrt(np.mean(grid_u2[:above]))
        moved = abs(reach(u_rms) - depth)
        depth = reach(u_rms)
        rounds += 1
        if rounds >= 5 and moved <= tol:
            return u_rms


def nmo_times(travel_time, ant_sep, uice=1.69e8, uair=3.0e8, dt=None, snum=None, profile=None,
              permittivity_model=firn_permittivity):
    """Vertical two-way travel time (microseconds) of every sample of a trace recorded with the antennas
    ``ant_sep`` metres apart (reference ``:132-158``).  The recorded time plus the direct-arrival time
    ``sep = 1e6 * ant_sep / u`` is the hypotenuse of a triangle whose other side is ``sep``, so the vertical leg is
    ``sqrt((t + sep)**2 - sep**2)``.  ``u`` is ``uice`` for every sample, or with ``profile = (depth, density)``
    the RMS velocity of the firn column above the sample, on a grid of ``10 * snum`` depths (``:126-152``)."""
    t = np.asarray(travel_time, dtype=np.float64)
    if profile is None:
        u = uice
    else:
        from scipy.interpolate import interp1d
        knots, rho = profile
        u_knots = uair / np.sqrt(np.real(permittivity_model(rho)))
        grid_depth = np.linspace(np.min(knots), np.max(knots), 10 * snum)
        grid_u2 = interp1d(knots, u_knots)(grid_depth) ** 2.
        print('Iterating velocity profile in firn...')
        tol = 0.1 * dt / 2. * uice                                # a tenth of a sample, in metres of ice
        u = np.array([_rms_velocity_above(ti, uice, grid_depth, grid_u2, tol) for ti in t])
    sep = 1e6 * (ant_sep / u)
    return np.sqrt((t + sep) ** 2. - sep ** 2.)


def traveltime_to_depth(travel_time, dt, profile_depth, profile_rho, c=3.0e8, permittivity_model=firn_permittivity):
    """Depth of every sample under a density profile (reference ``:196-235``).  The wave is followed down the
    time axis one sample at a time, each sample at the velocity of the profile knot nearest the depth reached so
    far; the first sample after time zero covers only its own share of a time step, at the surface velocity.
    Samples before time zero keep the depth solid ice (917 kg/m3) would give them."""
    t = np.asarray(travel_time, dtype=np.float64)
    knot_u = c / np.sqrt(np.real(permittivity_model(profile_rho)))
    depth = t / 2. * c / np.sqrt(np.real(permittivity_model(917.))) * 1.0e-6
    step_us = dt * 1.0e6
    reached = 0.
    for i in np.flatnonzero(t >= 0.):
        if t[i] < step_us:
            reached += t[i] / 2. * knot_u[0] * 1.0e-6
        else:
            nearest = np.nanargmin(np.abs(profile_depth - reached))
            reached += dt / 2. * knot_u[nearest]
        depth[i] = reached
    return depth


# ------------------------------------------------------------------------------------------------ row blend
class RowLerpTables(object):
    """``lo, hi, den, t`` per output row of ``scipy.interpolate.interp1d(x, data, axis=0)(x_new)``:
    ``out[i] = (data[hi[i]] - data[lo[i]]) / den[i] * t[i] + data[lo[i]]``.

    SciPy searches the knots in two ways.  ``np_interp=True`` is what a 1-D float64 (or integer, widened) trace
    gets, ``np.interp``: the interval with ``x[j] <= x_new < x[j + 1]``, and a new point ON a knot returns that
    sample (``t = 0`` and ``hi = lo`` here, so that a NaN in the next sample does not leak).  ``np_interp=False`` is
    ``interp1d._call_linear``, what float32 traces and 2-D arrays get: ``searchsorted(x, x_new).clip(1, n - 1)``,
    so a point on knot j is evaluated from the interval below it.  Out-of-range points raise SciPy's ValueError."""

    def __init__(self, x, x_new, np_interp):
        x = np.asarray(x, dtype=np.float64)
        x_new = np.asarray(x_new, dtype=np.float64)
        order = np.argsort(x, kind='mergesort')
        xs = x[order]
        _check_range(xs, x_new)
        n = len(xs)
        if np_interp:
            j = np.searchsorted(xs, x_new, side='right') - 1
            j_hi = np.minimum(j + 1, n - 1)
            t = x_new - xs[j]
            on_knot = (t == 0) | (j_hi == j)
            j_hi = np.where(on_knot, j, j_hi)
            den = np.where(on_knot, 1.0, xs[j_hi] - xs[j])
            t = np.where(on_knot, 0.0, t)
        else:
            j_hi = np.searchsorted(xs, x_new).clip(1, n - 1).astype(int)
            j = j_hi - 1
            den = xs[j_hi] - xs[j]
            t = x_new - xs[j]
        self.n_out = len(x_new)
        self.lo = np.ascontiguousarray(order[j], dtype=np.int32)
        self.hi = np.ascontiguousarray(order[j_hi], dtype=np.int32)
        self.den = np.ascontiguousarray(den, dtype=np.float64)
        self.t = np.ascontiguousarray(t, dtype=np.float64)

    def pointers(self):
        ip = C.POINTER(C.c_int)
        return (self.lo.ctypes.data_as(ip), self.hi.ctypes.data_as(ip), _hip.as_dp(self.den)[1], _hip.as_dp(self.t)[1])


def np_interp_convention(dtype):
    """True when SciPy interpolates a 1-D trace of this dtype with ``np.interp`` (float64, and integers, which it
    widens to float64 first); float32 goes through ``interp1d._call_linear``."""
    return np.dtype(dtype) != np.float32


def _work(data):
    return _hip.work_array(data, 'changing the sample axis of complex data is', copy=False)


def row_lerp_host(data, tables):
    """float64 (n_out, tnum) blend of the rows of a host radargram (integers widened to float64 first)."""
    work = _work(data)
    snum, tnum = work.shape
    out = np.empty((tables.n_out, tnum), dtype=np.float64)
    if out.size == 0:
        return out
    lo, hi, den, t = tables.pointers()
    rc = _hip.load().impdar_row_lerp(_hip.context(), work.ctypes.data_as(C.c_void_p), _hip.dtype_code(work.dtype), snum,
                                    tnum, lo, hi, den, t, tables.n_out, out.ctypes.data_as(C.c_void_p))
    _hip.check(rc, 'impdar_row_lerp')
    return out


def row_lerp_dev(d_arr, tables):
    """New resident float64 (n_out, tnum) array; the caller frees the old one."""
    snum, tnum = d_arr.shape
    with _hip.new_device_array(d_arr.ctx, (tables.n_out, tnum), np.float64) as d_out:
        if d_out.nbytes:
            lo, hi, den, t = tables.pointers()
            rc = _hip.load().impdar_row_lerp_dev(d_arr.ctx, d_arr.ptr, _hip.dtype_code(d_arr.dtype), snum, tnum, lo,
                                                hi, den, t, tables.n_out, d_out.ptr)
            _hip.check(rc, 'impdar_row_lerp')
    return d_out


# ------------------------------------------------------------------------------------------------ column shift
def _shift_arg(shift, tnum):
    shift = np.ascontiguousarray(shift, dtype=np.int32)
    if shift.shape != (tnum,):
        raise ValueError('the shift table must have tnum = %d entries' % tnum)
    return shift, shift.ctypes.data_as(C.POINTER(C.c_int))


def col_shift_host(data, shift, n_out):
    """float64 (n_out, tnum) array with ``out[i, j] = data[i + shift[j], j]`` where that row exists, NaN
    elsewhere (integers widened to float64 first)."""
    work = _work(data)
    snum, tnum = work.shape
    shift, p_shift = _shift_arg(shift, tnum)
    out = np.empty((n_out, tnum), dtype=np.float64)
    if out.size == 0:
        return out
    rc = _hip.load().impdar_col_shift(_hip.context(), work.ctypes.data_as(C.c_void_p), _hip.dtype_code(work.dtype), snum,
                                     tnum, p_shift, n_out, out.ctypes.data_as(C.c_void_p))
    _hip.check(rc, 'impdar_col_shift')
    return out


def col_shift_dev(d_arr, shift, n_out):
    """New resident float64 (n_out, tnum) array; the caller frees the old one."""
    snum, tnum = d_arr.shape
    shift, p_shift = _shift_arg(shift, tnum)
    with _hip.new_device_array(d_arr.ctx, (n_out, tnum), np.float64) as d_out:
        if d_out.nbytes:
            rc = _hip.load().impdar_col_shift_dev(d_arr.ctx, d_arr.ptr, _hip.dtype_code(d_arr.dtype), snum, tnum,
                                                 p_shift, n_out, d_out.ptr)
            _hip.check(rc, 'impdar_col_shift')
    return d_out


def row_range_dev(d_arr, start, stop):
    """New resident array of the array's own dtype holding its rows ``[start:stop]`` (Python slice bounds): one
    device-to-device copy."""
    snum, tnum = d_arr.shape
    start, stop, _ = slice(start, stop).indices(snum)
    rows = max(stop - start, 0)
    with _hip.new_device_array(d_arr.ctx, (rows, tnum), d_arr.dtype) as d_out:
        if d_out.nbytes:
            code = _hip.dtype_code(d_arr.dtype)
            src = C.c_void_p(d_arr.ptr.value + start * tnum * d_arr.dtype.itemsize)
            rc = _hip.load().impdar_cast_dev(d_arr.ctx, src, code, d_out.ptr, code, rows * tnum)
            _hip.check(rc, 'impdar_cast_dev')
    return d_out


# ------------------------------------------------------------------------------------------------ crop, elevation
def crop_index(lim, top_or_bottom, dimension, travel_time, nmo_depth, trig, uice=1.69e8):
    """The sample index ``crop`` cuts at (:262-283): an int, or for ``dimension='pretrig'`` with a trace-wise
    ``trig`` an int array, one trigger sample per trace."""
    if top_or_bottom not in ['top', 'bottom']:
        raise ValueError('top_or_bottom must be "top" or "bottom" not {:s}'.format(top_or_bottom))
    if dimension not in ['snum', 'twtt', 'depth', 'pretrig']:
        raise ValueError('Dimension must be in [\'snum\', \'twtt\', \'depth\']')
    if top_or_bottom == 'bottom' and dimension == 'pretrig':
        raise ValueError('Only use pretrig to crop from the top')
    if dimension == 'twtt':
        return np.min(np.argwhere(travel_time >= lim))
    if dimension == 'depth':
        depth = nmo_depth if nmo_depth is not None else travel_time / 2. * uice * 1.0e-6
        return np.min(np.argwhere(depth >= lim))
    if dimension == 'pretrig':
        return trig.astype(int) if isinstance(trig, np.ndarray) else int(trig)
    return int(lim)


def elev_shifts(elev, dt, v_avg, nmo_depth):
    """``(top_inds, max_samp, elevation)`` of ``elev_correct`` (:612-631): the samples every trace moves down by,
    the rows added, and the elevation of every row of the new array."""
    elev_diffs = np.max(elev) - elev
    max_diff = np.max(elev_diffs)
    dz_avg = dt * (v_avg / 2.)
    max_samp = int(np.floor(max_diff / dz_avg))
    top_inds = (elev_diffs / dz_avg).astype(int)
    elevation = np.hstack((np.arange(np.max(elev), np.min(elev), -dz_avg), np.min(elev) - nmo_depth))
    return top_inds, max_samp, elevation
