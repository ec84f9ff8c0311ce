"""The part of the reference's ``gpslib`` that the instrument loaders use (``src/impdar/lib/gpslib.py:18-345``):
``hhmmss2dec``, the GGA table ``nmea_info`` with its accessors, ``nmea_all_info`` and ``RadarGPS``, which carries sparse
GPS fixes onto every trace.  All of it is host NumPy / SciPy on O(tnum) vectors, in the reference's operation order, so
the results equal the reference's bit for bit.

Without GDAL (``osgeo`` / ``osr``) ``conversions_enabled`` is False, as in the reference: projected coordinates are then
the reference's spherical guess (``y = 110000 lat``, ``x = 110000 lon |cos lat|``) and the conversion helpers raise its
``ImportError``.

``kinematic_gps_control`` (``:348-464``), ``kinematic_gps_mat``, ``kinematic_gps_csv`` and ``interp`` (``:467-595``) attach a
precision GPS track to the traces.  Their time-offset search (``guess_offset``: 5 passes over 5001 or 1001 candidate
offsets, each a re-interpolation of the whole track and two correlations) runs on the MI355X
(``impdar_amd.gpstrack.cc_search``); everything else, the final interpolation included, is the reference's own host
NumPy / SciPy calls.
"""
import numpy as np
from scipy.interpolate import interp1d

try:
    import osr                                                       # noqa: F401
    conversions_enabled = True
except ImportError:
    try:
        from osgeo import osr                                        # noqa: F401
        conversions_enabled = True
    except ImportError:
        conversions_enabled = False

_NO_OSR = 'Cannot convert coordinates: osr not importable'
_GUESS = 110000.0                 # metres per degree, the reference's stand-in for a projection


def _utm_transform(lat, lon):
    """WGS84 -> the UTM zone of (lat, lon), through GDAL."""
    zone = int(1 + (lon + 180.0) / 6.0)
    utm = osr.SpatialReference()
    utm.SetWellKnownGeogCS('WGS84')
    utm.SetUTM(zone, not lat < 0.0)
    geo = utm.CloneGeogCS()
    for cs in (utm, geo):
        if hasattr(osr, 'OAMS_TRADITIONAL_GIS_ORDER'):
            cs.SetAxisMappingStrategy(osr.OAMS_TRADITIONAL_GIS_ORDER)
    return osr.CoordinateTransformation(geo, utm).TransformPoints, utm.ExportToPrettyWkt()


def _srs_transform(t_srs, reverse=False):
    out = osr.SpatialReference()
    try:
        out.SetFromUserInput(t_srs)
    except TypeError:
        out.SetFromUserInput(t_srs[0])
    geo = out.CloneGeogCS()
    for cs in (out, geo):
        if hasattr(osr, 'OAMS_TRADITIONAL_GIS_ORDER'):
            cs.SetAxisMappingStrategy(osr.OAMS_TRADITIONAL_GIS_ORDER)
    pair = (out, geo) if reverse else (geo, out)
    return osr.CoordinateTransformation(*pair).TransformPoints, out.ExportToPrettyWkt()


def get_utm_conversion(lat, lon):
    if not conversions_enabled:
        raise ImportError(_NO_OSR)
    return _utm_transform(lat, lon)


def get_conversion(t_srs):
    if not conversions_enabled:
        raise ImportError(_NO_OSR)
    return _srs_transform(t_srs)


def get_rev_conversion(t_srs):
    if not conversions_enabled:
        raise ImportError(_NO_OSR)
    return _srs_transform(t_srs, reverse=True)


def hhmmss2dec(times):
    """hhmmss(.ss) as a number -> fraction of a day."""
    sec = times % 100
    minute = (times % 10000 - sec) / 100
    hour = (times - minute * 100 - sec) / 10000
    return (hour + minute / 60.0 + sec / 3600.0) / 24.0


def _degrees(ddmm, sign):
    """ddmm.mmmm -> signed decimal degrees."""
    minutes = ddmm % 100
    return sign * ((ddmm - minutes) / 100 + minutes / 60)


class nmea_info(object):
    """The GGA table (``all_data``: time, lat, sign, lon, sign, quality, satellites, hdop, elevation, geoid offset) and
    what is read from it: ``lat``, ``lon``, ``qual``, ``sats``, ``z``, ``geo_offset``, ``times``, projected ``x`` and
    ``y``, ``dist`` in km."""

    all_data = None
    lat = None
    lon = None
    qual = None
    sats = None
    x = None
    y = None
    z = None
    geo_offset = None
    times = None
    scans = None

    def get_all(self):
        self.glat()
        self.glon()
        self.gqual()
        self.gsats()
        self.gz()
        self.ggeo_offset()
        self.gtimes()
        if conversions_enabled:
            self.get_utm()
        self.get_dist()

    def glat(self):
        if self.lat is None:
            self.lat = _degrees(self.all_data[:, 1], self.all_data[:, 2])
        if self.y is None:
            self.y = self.lat * _GUESS
        return self.lat

    def glon(self):
        if self.lon is None:
            self.lon = _degrees(self.all_data[:, 3], self.all_data[:, 4])
        if self.x is None:
            if self.lat is None:
                self.glat()
            self.x = self.lon * _GUESS * np.abs(np.cos(self.lat * np.pi / 180.0))
        return self.lon

    def gqual(self):
        self.qual = self.all_data[:, 5]
        return self.qual

    def gsats(self):
        self.sats = self.all_data[:, 6]
        return self.sats

    def gz(self):
        self.z = self.all_data[:, 8]
        return self.z

    def ggeo_offset(self):
        self.geo_offset = self.all_data[:, 8]          # the reference reads the elevation column here too
        return self.geo_offset

    def gtimes(self):
        self.times = self.all_data[:, 0]
        return self.times

    def get_dist(self):
        if self.y is None:
            self.glat()
        if self.x is None:
            self.glon()
        if conversions_enabled:
            self.get_utm()
        self.dist = np.zeros((len(self.y), ))
        self.dist[1:] = np.cumsum(np.sqrt(np.diff(self.x) ** 2.0 + np.diff(self.y) ** 2.0)) / 1000.0

    def get_utm(self):
        transform, _ = get_utm_conversion(np.nanmean(self.lat), np.nanmean(self.lon))
        pts = np.array(transform(np.vstack((self.lon, self.lat)).transpose()))
        self.x, self.y = pts[:, 0], pts[:, 1]

    @property
    def dectime(self):
        return hhmmss2dec(self.times)


def _number(field):
    return float(field) if field != '' else np.nan


def _gga_row(sentence):
    """The ten numbers of one GGA sentence (three for a short one); NaN for an empty field, all NaN for a corrupted line."""
    f = sentence.split(',')
    if len(f) <= 2:
        return [np.nan] * 10
    try:
        if len(f) > 5:
            row = [_number(x) for x in f[1:3] + [1] + [f[4]] + [1] + f[6:10] + [f[11]]]
            if f[5] == 'W':
                row[4] = -1
        else:
            row = [_number(x) for x in f[1:3] + [1]]
        if f[3] == 'S':
            row[2] = -1
    except (ValueError, IndexError):
        row = [np.nan] * 10
    return row


def nmea_all_info(list_of_sentences):
    """An :class:`nmea_info` whose table holds the sentences, which must all be $GPGGA."""
    if not np.all([sentence.split(',')[0] == '$GPGGA' for sentence in list_of_sentences]):
        raise ValueError('I can only do gga sentences right now')
    data = nmea_info()
    data.all_data = np.array([_gga_row(sentence) for sentence in list_of_sentences])
    return data


class RadarGPS(nmea_info):
    """GGA fixes taken at the traces ``scans``, carried onto every trace of ``trace_num`` by linear interpolation
    (extrapolated at the ends).  Fixes whose time or scan repeats the previous one's are left out."""

    def __init__(self, gga, scans, trace_num):
        self.nmea_info = nmea_all_info(gga)
        self.nmea_info.scans = scans
        self.nmea_info.get_all()
        src = self.nmea_info
        fresh = np.logical_and(~np.isnan(src.times[1:]), np.diff(src.scans) != 0)
        fresh = np.logical_and(np.diff(src.times) != 0, fresh)
        keep = np.hstack((np.array([0]), 1 + np.where(fresh)[0]))

        def onto_traces(values):
            return interp1d(src.scans[keep], values[keep], kind='linear', fill_value='extrapolate')(trace_num)

        self.lat = onto_traces(src.lat)
        self.lon = onto_traces(src.lon)
        self.z = onto_traces(src.z)
        self.times = onto_traces(src.times)
        if conversions_enabled:
            self.get_utm()
        self.get_dist()


# a list here collects (search_vals, cc_coeffs, chosen index) of every pass of the offset search, for tests and benchmarks
_search_log = None


def _gaps_to_nan(decday_interp, decday):
    """``old_gps_gaps``: the trace times farther than a second from every fix become NaN (the reference's loop over
    ``np.min(abs(dday - decday))``, through a sorted copy: the nearest fix is one of the two neighbours, so the distance
    is the same float)."""
    if len(decday) == 0 or np.any(np.isnan(decday)):
        return                                       # (np.min of nothing raises there; a NaN fix makes every minimum NaN)
    fixes = np.sort(decday)
    right = np.searchsorted(fixes, decday_interp).clip(0, len(fixes) - 1)
    left = (right - 1).clip(0, len(fixes) - 1)
    nearest = np.minimum(np.abs(decday_interp - fixes[left]), np.abs(decday_interp - fixes[right]))
    decday_interp[nearest > 1. / (24 * 3600.)] = np.nan


def kinematic_gps_control(dats, lat, lon, elev, decday, offset=0.0, extrapolate=False, guess_offset=True,
                          old_gps_gaps=False):
    """New, better GPS data for ``lat``, ``long`` and ``elev`` of ``dats`` (one RadarData or a list), interpolated at the
    traces' ``decday`` (the reference's ``gpslib.py:348-464``, same arguments and defaults).

    ``offset`` translates the GPS times onto the radar's.  ``extrapolate`` fills traces outside the GPS record by
    extrapolation instead of raising -- use with caution.  ``guess_offset`` searches the offset: 5 passes, each over
    ``np.linspace(-0.1 |o|, 0.1 |o|, 1001)`` around the running offset ``o`` (``np.linspace(-0.1, 0.1, 5001)`` days when
    it is zero), keeping the candidate whose interpolated track correlates best with the radar's own positions.  The
    candidates of a pass are scored in one launch on the GPU, on the GPS arrays sorted once by a stable argsort of
    ``decday`` (the reference re-sorts the shifted times for every candidate: fixes whose shifted times coincide only
    after rounding are outside what is held to the reference).  A candidate that leaves a trace outside the GPS record
    raises ``ValueError`` without ``extrapolate``, as the reference does at the first such candidate.
    ``old_gps_gaps`` keeps the radar's own position wherever no fix lies within a second of the trace."""
    fill_value = 'extrapolate' if extrapolate else np.nan
    if type(dats) not in [list, tuple]:
        dats = [dats]
    for in_dat in [lat, lon, elev]:
        if len(decday) != len(in_dat):
            raise IndexError('lat, lon, elev, and decday must be the same len')
    offsets = [offset for i in dats]
    if guess_offset:
        from .. import gpstrack
        print('CC search')
        order = np.argsort(decday, kind='stable')
        gps_t, gps_lat, gps_lon = np.asarray(decday)[order], np.asarray(lat)[order], (lon % 360)[order]
        for j, dat in enumerate(dats):
            decday_interp = dat.decday.copy()
            if old_gps_gaps:
                _gaps_to_nan(decday_interp, decday)
                dat.lat[dat.lat == 0.] = np.nan
                dat.long[dat.long == 0.] = np.nan
                if np.all(np.isnan(decday_interp)):
                    raise ValueError("Too much time offset")
            for i in range(5):
                if (min(lon % 360) - max(dat.long % 360)) > 0. or (min(dat.long % 360) - max(lon % 360)) > 0.:
                    raise ValueError('No overlap in longitudes')
                if offsets[j] != 0.0:
                    search_vals = np.linspace(-0.1 * abs(offsets[j]), 0.1 * abs(offsets[j]), 1001)
                else:
                    search_vals = np.linspace(-0.1, 0.1, 5001)
                cc_coeffs, outside = gpstrack.cc_search(gps_t, gps_lat, gps_lon, decday_interp, dat.lat, dat.long % 360,
                                                        offsets[j], search_vals, extrapolate)
                if not extrapolate and np.any(outside > 0):
                    first = int(np.argmax(outside > 0))
                    raise ValueError('{:d} trace times are outside the GPS record at the candidate offset {:f}: the '
                                     'interpolation range does not cover the search window'.format(
                                         int(outside[first]), offsets[j] + search_vals[first]))
                best = np.argmax(cc_coeffs)
                if _search_log is not None:
                    _search_log.append((search_vals, cc_coeffs, int(best)))
                offsets[j] += search_vals[best]
                print('Maximum correlation at offset: {:f}'.format(offsets[j]))

    for j, dat in enumerate(dats):
        decday_interp = dat.decday.copy()
        lat_interpolator = interp1d(decday + offsets[j], lat, kind='linear', fill_value=fill_value)
        long_interpolator = interp1d(decday + offsets[j], lon % 360, kind='linear', fill_value=fill_value)
        elev_interpolator = interp1d(decday + offsets[j], elev, kind='linear', fill_value=fill_value)
        if old_gps_gaps:
            # (again: otherwise the traces off the record are out of bounds)
            _gaps_to_nan(decday_interp, decday)
            lat_interp = lat_interpolator(decday_interp)
            long_interp = long_interpolator(decday_interp)
            elev_interp = elev_interpolator(decday_interp)
            gaps = np.isnan(decday_interp)
            lat_interp[gaps] = dat.lat[gaps]
            long_interp[gaps] = dat.long[gaps]
            elev_interp[gaps] = dat.elev[gaps]
            dat.lat = lat_interp
            dat.long = long_interp % 360
            dat.elev = elev_interp
        else:
            dat.lat = lat_interpolator(decday_interp)
            dat.long = long_interpolator(decday_interp)
            dat.elev = elev_interpolator(decday_interp)
        if conversions_enabled:
            dat.get_projected_coords()


def kinematic_gps_mat(dats, mat_fn, offset=0.0, extrapolate=False, guess_offset=False, old_gps_gaps=False):
    """:func:`kinematic_gps_control` with ``lat``, ``long``, ``elev`` and ``decday`` of a matlab file."""
    from scipy.io import loadmat
    mat = loadmat(mat_fn)
    for val in ['lat', 'long', 'elev', 'decday']:
        if val not in mat:
            raise ValueError('{:s} needs to be contained in matlab input file'.format(val))
    kinematic_gps_control(dats, mat['lat'].flatten(), mat['long'].flatten(), mat['elev'].flatten(),
                          mat['decday'].flatten(), offset=offset, extrapolate=extrapolate, guess_offset=guess_offset,
                          old_gps_gaps=old_gps_gaps)


def kinematic_gps_csv(dats, csv_fn, offset=0, names='decday,long,lat,elev', extrapolate=False, guess_offset=False,
                      old_gps_gaps=False, **genfromtxt_flags):
    """:func:`kinematic_gps_control` with the columns of a csv file read by ``numpy.genfromtxt``: ``names`` (a
    comma-separated string, a list, or True to read them from the file) must contain 'decday', 'long', 'lat' and
    'elev'; further keywords go to ``genfromtxt``."""
    data = np.genfromtxt(csv_fn, names=names, **genfromtxt_flags)
    kinematic_gps_control(dats, data['lat'].flatten(), data['long'].flatten(), data['elev'].flatten(),
                          data['decday'].flatten(), offset=offset, extrapolate=extrapolate, guess_offset=guess_offset,
                          old_gps_gaps=old_gps_gaps)


def interp(dats, spacing=None, fn=None, fn_type=None, offset=0.0, min_movement=1.0e-2, genfromtxt_kwargs={},
           extrapolate=False, guess_offset=False, **kwargs):
    """Kinematic GPS control from ``fn`` (a mat or csv file with lat, long, elev and decday; ``fn_type`` 'mat' or 'csv',
    else by extension; None: no control), then every radargram to constant ``spacing`` in metres (None: none).  A file
    without ``dist`` first takes its positions from its own GPS.  ``min_movement`` culls stationary traces."""
    if fn is not None:
        if fn_type == 'mat' or ((fn_type is None) and (fn[-4:] == '.mat')):
            kinematic_gps_mat(dats, fn, offset=offset, extrapolate=extrapolate, guess_offset=guess_offset)
        elif fn_type == 'csv' or (fn_type is None and fn[-4:] in ['.csv', '.txt']):
            kinematic_gps_csv(dats, fn, offset=offset, extrapolate=extrapolate, guess_offset=guess_offset,
                              **genfromtxt_kwargs)
        else:
            raise ValueError('Cannot identify fn filetype, must be mat or csv')
    if spacing is not None:
        for dat in dats:
            if dat.dist is None:
                kinematic_gps_control(dat, dat.lat, dat.long, dat.elev, dat.decday, extrapolate=extrapolate,
                                      guess_offset=False)
            dat.constant_space(spacing, min_movement=min_movement)
