"""The time-offset search of kinematic GPS control on the MI355X (``csrc/gpstrack.hip``): the correlation of the radar's own
positions with the GPS track interpolated to the trace times, for a batch of candidate offsets in one launch."""
import ctypes as C

import numpy as np

from . import _hip


def cc_search(gps_t, lat, lon, t, rlat, rlon, base, search, extrapolate, probe=None):
    """``cc[c] = r(lat_i, rlat) + r(lon_i, rlon)`` for every candidate ``search[c]``, where ``lat_i`` / ``lon_i`` are the
    track ``(gps_t + search[c] + base, lat / lon)`` interpolated to the trace times ``t`` as the reference's ``interp1d``
    calls do it (``include/impdar_hip.h``: ``impdar_gps_cc``).  ``gps_t`` must be non-decreasing; nothing is sorted here.
    Returns ``(cc, nout)`` -- ``nout[c]`` traces of candidate ``c`` lay outside the shifted record -- and, with ``probe``
    a candidate's index, also its interpolated latitude and longitude."""
    lib = _hip.load()
    ctx = _hip.context()
    gps_t, p_gt = _hip.as_dp(gps_t)
    lat, p_lat = _hip.as_dp(lat)
    lon, p_lon = _hip.as_dp(lon)
    t, p_t = _hip.as_dp(t)
    rlat, p_rlat = _hip.as_dp(rlat)
    rlon, p_rlon = _hip.as_dp(rlon)
    search, p_s = _hip.as_dp(search)
    if not (gps_t.ndim == lat.ndim == lon.ndim == t.ndim == rlat.ndim == rlon.ndim == search.ndim == 1):
        raise ValueError('cc_search takes one-dimensional arrays')
    if not (gps_t.size == lat.size == lon.size and t.size == rlat.size == rlon.size):
        raise ValueError('gps_t, lat, lon must have one length and t, rlat, rlon another')
    cc = np.empty(search.size, dtype=np.float64)
    nout = np.empty(search.size, dtype=np.int64)
    p_nout = nout.ctypes.data_as(C.POINTER(C.c_longlong))
    if probe is None:
        _hip.check(lib.impdar_gps_cc(ctx, p_gt, p_lat, p_lon, gps_t.size, p_t, p_rlat, p_rlon, t.size, float(base), p_s,
                                     search.size, int(bool(extrapolate)), cc.ctypes.data_as(_hip._dp), p_nout, -1, None, None),
                   'impdar_gps_cc')
        return cc, nout
    plat, plon = np.empty(t.size, dtype=np.float64), np.empty(t.size, dtype=np.float64)
    _hip.check(lib.impdar_gps_cc(ctx, p_gt, p_lat, p_lon, gps_t.size, p_t, p_rlat, p_rlon, t.size, float(base), p_s,
                                 search.size, int(bool(extrapolate)), cc.ctypes.data_as(_hip._dp), p_nout, int(probe),
                                 plat.ctypes.data_as(_hip._dp), plon.ctypes.data_as(_hip._dp)), 'impdar_gps_cc')
    return cc, nout, plat, plon
