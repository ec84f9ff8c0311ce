"""The part of the reference's ``gpslib`` that the instrument loaders use (``src/impdar/lib/gpslib.py:18-345``):
``hhmmss2dec``, the GGA table ``nmea_info`` with its accessors, ``nmea_all_info`` and ``RadarGPS``, which carries sparse
GPS fixes onto every trace.  All of it is host NumPy / SciPy on O(tnum) vectors, in the reference's operation order, so
the results equal the reference's bit for bit.

Without GDAL (``osgeo`` / ``osr``) ``conversions_enabled`` is False, as in the reference: projected coordinates are then
the reference's spherical guess (``y = 110000 lat``, ``x = 110000 lon |cos lat|``) and the conversion helpers raise its
``ImportError``.  ``kinematic_gps_control`` and ``interp`` are not part of this package.
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
