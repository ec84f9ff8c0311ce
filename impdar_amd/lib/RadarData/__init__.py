"""Minimal ``RadarData`` container: the attribute contract the migration path
reads and writes, the ``.mat`` (StoDeep/ImpDAR) round trip and the
``migrate`` dispatch.

Mirrors (re-implemented, not copied) the reference's
``src/impdar/lib/RadarData/__init__.py:36-61`` (attribute lists), ``:124-244``
(None-initialisation and ``.mat`` load), ``:270-331`` (``check_attrs``),
``_RadarDataSaving.py:32-78`` (``save`` incl. the cast back to the file's
dtype), ``_RadarDataFiltering.py:590-637`` (``migrate``) and the two steps an
impproc chain runs in front of a migration: ``vertical_band_pass``
(``_RadarDataFiltering.py:469-549``) and ``constant_space``
(``_RadarDataProcessing.py:499-583``), and the steps that change the sample
axis: ``crop``, ``nmo``, ``constant_sample_depth_spacing`` and ``elev_correct``
(``_RadarDataProcessing.py:50-337, 585-632``), the steps that change the
trace axis, ``reverse``, ``hcrop`` and ``restack`` (``:20-47, 340-453``), the
gains ``rangegain`` and ``agc`` (``:456-496``) and ``winavg_hfilt``
(``_RadarDataFiltering.py:353-440``), and picking as the last step of a chain:
``pick_layers`` and ``continuity_index`` (``_RadarDataPicking.py``), after which
``picks`` is a ``Picks`` object that ``save()`` writes.  A loaded ``picks``
struct is still carried as ``_picks_struct`` until something picks, and the
spectra behind the reference's ``plot_ft``, ``plot_hft`` and
``plot_spectrogram``: ``vertical_spectrum``, ``horizontal_spectrum`` and
``spectrogram`` (``_RadarDataSpectra.py``; drawn by ``lib/plot.py``), and what
its ``plot_radargram`` and ``plot_traces`` read: ``percentiles``, ``window``
and ``flattened`` (``_RadarDataDisplay.py``), and two extensions on the Stolt
transforms: ``velocity_scan`` (``velscan.py``) and the f-k fan filter with its
spectrum, ``fk_filter`` and ``fk_spectrum`` (``fk.py``), and a third along the
traces: ``predictive_decon``, ``decon_operators`` and ``autocorrelation``
(``decon.py``), and a fourth, the complex-trace attributes ``envelope``,
``instantaneous_phase``, ``instantaneous_frequency``, ``complex_attribute``
and ``analytic_signal`` (``attributes.py``), and a fifth, the layers' local
slope and the mean along it, ``layer_slope`` and ``dip_smooth``
(``slope.py``).  Everything else in the
reference's class (moving picks with the data, GPS, the ApRES plots) is out
of scope.
"""
import numpy as np

from ..ImpdarError import ImpdarError
from ..RadarFlags import RadarFlags
from ._RadarDataFiltering import migrate as _migrate, vertical_band_pass as _vertical_band_pass
from ._RadarDataFiltering import adaptivehfilt as _adaptivehfilt, hfilt as _hfilt, horizontalfilt as _horizontalfilt
from ._RadarDataFiltering import denoise as _denoise, winavg_hfilt as _winavg_hfilt
from ._RadarDataFiltering import highpass as _highpass, horizontal_band_pass as _horizontal_band_pass, lowpass as _lowpass
from ._RadarDataProcessing import constant_space as _constant_space
from ._RadarDataProcessing import constant_sample_depth_spacing as _constant_sample_depth_spacing, crop as _crop
from ._RadarDataProcessing import elev_correct as _elev_correct, nmo as _nmo
from ._RadarDataProcessing import hcrop as _hcrop, restack as _restack, reverse as _reverse
from ._RadarDataProcessing import agc as _agc, rangegain as _rangegain
from ._RadarDataPicking import continuity_index as _continuity_index, pick_layers as _pick_layers
from ._RadarDataSpectra import horizontal_spectrum as _horizontal_spectrum, spectrogram as _spectrogram
from ._RadarDataSpectra import vertical_spectrum as _vertical_spectrum
from ._RadarDataDisplay import flattened as _flattened, percentiles as _percentiles, window as _window
from ... import resident as _resident
from ...velscan import stolt_velocity_scan as _velocity_scan
from ...fk import fk_filter as _fk_filter, fk_spectrum as _fk_spectrum
from ...decon import autocorrelation as _autocorrelation, decon_operators as _decon_operators, predictive_decon as _predictive_decon
from ...attributes import analytic_signal as _analytic_signal, complex_attribute as _complex_attribute, envelope as _envelope
from ...attributes import instantaneous_frequency as _instantaneous_frequency, instantaneous_phase as _instantaneous_phase
from ...slope import dip_smooth as _dip_smooth, layer_slope as _layer_slope
from ._resident import data_dtype as _resident_dtype, data_shape as _resident_shape

STODEEP_ATTRS = ['data', 'migdata', 'interp_data', 'nmo_data', 'filtdata', 'hfilt_data']


class RadarData(object):
    attrs_guaranteed = ['chan', 'data', 'decday', 'dt', 'pressure', 'snum', 'tnum', 'trace_int',
                        'trace_num', 'travel_time', 'trig', 'trig_level']
    attrs_optional = ['nmo_depth', 'lat', 'long', 'elev', 'dist', 'x_coord', 'y_coord', 'fn', 't_srs']
    stodeep_attrs = STODEEP_ATTRS

    migrate = _migrate
    vertical_band_pass = _vertical_band_pass
    hfilt = _hfilt
    horizontalfilt = _horizontalfilt
    adaptivehfilt = _adaptivehfilt
    denoise = _denoise
    horizontal_band_pass = _horizontal_band_pass
    highpass = _highpass
    lowpass = _lowpass
    constant_space = _constant_space
    crop = _crop
    nmo = _nmo
    constant_sample_depth_spacing = _constant_sample_depth_spacing
    elev_correct = _elev_correct
    reverse = _reverse
    hcrop = _hcrop
    restack = _restack
    rangegain = _rangegain
    agc = _agc
    winavg_hfilt = _winavg_hfilt
    pick_layers = _pick_layers
    continuity_index = _continuity_index
    vertical_spectrum = _vertical_spectrum
    horizontal_spectrum = _horizontal_spectrum
    spectrogram = _spectrogram
    percentiles = _percentiles
    window = _window
    flattened = _flattened
    velocity_scan = _velocity_scan
    fk_filter = _fk_filter
    fk_spectrum = _fk_spectrum
    predictive_decon = _predictive_decon
    decon_operators = _decon_operators
    autocorrelation = _autocorrelation
    envelope = _envelope
    instantaneous_phase = _instantaneous_phase
    instantaneous_frequency = _instantaneous_frequency
    complex_attribute = _complex_attribute
    analytic_signal = _analytic_signal
    layer_slope = _layer_slope
    dip_smooth = _dip_smooth
    to_device = _resident.to_device
    from_device = _resident.from_device

    def __init__(self, fn_mat):
        for attr in self.attrs_guaranteed + self.attrs_optional:
            setattr(self, attr, None)
        self.flags = RadarFlags()
        self.picks = None
        self.data_dtype = None
        self._picks_struct = None
        self._dev = None
        self.fn = fn_mat
        if fn_mat is None:
            return
        from scipy.io import loadmat
        mat = loadmat(fn_mat)
        for attr in self.attrs_guaranteed:
            if attr == 'data':
                self._take_data(mat)
            elif attr not in mat:
                raise KeyError('.mat file does not appear to be in the StoDeep/ImpDAR format')
            else:
                setattr(self, attr, self._unbox(mat[attr], strict2d=True))
        for attr in self.attrs_optional:
            setattr(self, attr, self._unbox(mat[attr], strict2d=False) if attr in mat else None)
        self.data_dtype = self.data.dtype
        self.fn = fn_mat
        self.flags = RadarFlags()
        self.flags.from_matlab(mat['flags'])
        if 'picks' in mat:
            self._picks_struct = mat['picks']     # carried through save() untouched
        self.check_attrs()

    @staticmethod
    def _unbox(val, strict2d):
        """loadmat returns everything 2-D: scalars -> python scalars, vectors -> 1-D."""
        if val.shape == (1, 1):
            return val[0][0]
        if val.shape[0] == 1 or (len(val.shape) > 1 and val.shape[1] == 1):
            return val.flatten()
        return val

    def _take_data(self, mat):
        """First available of the StoDeep data matrices becomes ``data``."""
        for i, name in enumerate(self.stodeep_attrs):
            if name in mat:
                val = mat[name]
                if len(val.dtype) > 0:
                    print('Warning: Multiple arrays stored in {:s}, taking the first.'.format(name))
                    val = val[0][0][0]
                if i > 0:
                    print('First priority data {:s} not in structure, using {:s}'.format(
                        self.stodeep_attrs[0], name))
                self.data = val
                return
        raise KeyError('Data do not appear to be in StoDeep format')

    def check_attrs(self):
        """Raise ImpdarError for an ill-defined object."""
        for attr in self.attrs_guaranteed + ['fn']:
            if not hasattr(self, attr):
                raise ImpdarError('{:s} is missing. It appears that this is an ill-defined RadarData object'.format(attr))
            if getattr(self, attr) is None and not (attr == 'data' and getattr(self, '_dev', None) is not None):
                raise ImpdarError('{:s} is None. It appears that this is an ill-defined RadarData object'.format(attr))
        for attr in self.attrs_optional:
            if not hasattr(self, attr):
                raise ImpdarError('{:s} is missing. It appears that this is an ill-defined RadarData object'.format(attr))
        # (a radargram that was decoded in HBM has no host array: the resident shape is checked)
        if (tuple(_resident_shape(self)) != (self.snum, self.tnum)) and (self.elev is None):
            raise ImpdarError('The data shape does not match the snum and tnum values!!!')
        for attr in ['lat', 'long', 'pressure', 'trig', 'elev', 'dist', 'x_coord', 'y_coord', 'decday']:
            val = getattr(self, attr, None)
            if val is None:
                continue
            if (not hasattr(val, 'shape')) or len(val.shape) < 1:
                if val == 0:
                    setattr(self, attr, None)       # matlab's stand-in for None
                elif attr == 'trig':
                    self.trig = np.ones((self.tnum,), dtype=int) * int(self.trig)
                else:
                    raise ImpdarError('{:s} needs to be a vector'.format(attr))
            elif val.shape[0] != self.tnum:
                raise ImpdarError('{:s} needs length tnum {:d}'.format(attr, self.tnum))
        if getattr(self, 'data_dtype', None) is None:
            self.data_dtype = _resident_dtype(self)

    def get_projected_coords(self, t_srs=None):
        """``x_coord``, ``y_coord`` and ``dist`` (km) from ``lat`` / ``long`` (the reference's ``RadarData/__init__.py:333-354``):
        through ``t_srs`` (a string GDAL accepts, e.g. EPSG:3031), else the object's own ``t_srs``, else the UTM zone of the
        mean position.  Needs GDAL, as in the reference."""
        from .. import gpslib
        if t_srs is not None:
            transform, self.t_srs = gpslib.get_conversion(t_srs=t_srs)
        elif self.t_srs is not None:
            transform, _ = gpslib.get_conversion(t_srs=self.t_srs)
        else:
            transform, self.t_srs = gpslib.get_utm_conversion(np.nanmean(self.lat), np.nanmean(self.long))
        pts = np.array(transform(np.vstack((self.long, self.lat)).transpose()))
        self.x_coord, self.y_coord = pts[:, 0], pts[:, 1]
        self.dist = np.zeros((len(self.y_coord), ))
        self.dist[1:] = np.cumsum(np.sqrt(np.diff(self.x_coord) ** 2.0 + np.diff(self.y_coord) ** 2.0)) / 1000.0

    def save(self, fn):
        """Write a StoDeep/ImpDAR ``.mat``; ``data`` is cast back to the dtype
        it was loaded with (NaN-aware for integer files)."""
        from scipy.io import savemat
        if getattr(self, '_dev', None) is not None:
            self.from_device()
        mat = {}
        for attr in self.attrs_guaranteed:
            val = getattr(self, attr)
            mat[attr] = val if val is not None else 0
        for attr in self.attrs_optional + self.stodeep_attrs:
            if getattr(self, attr, None) is not None:
                mat[attr] = getattr(self, attr)
        if hasattr(self.picks, 'to_struct'):
            mat['picks'] = self.picks.to_struct()
        elif self._picks_struct is not None:
            mat['picks'] = self._picks_struct
        mat['flags'] = (self.flags if self.flags is not None else RadarFlags()).to_matlab()
        want = getattr(self, 'data_dtype', None)
        if want is not None and want != mat['data'].dtype:
            has_nan = np.issubdtype(mat['data'].dtype, np.floating) and np.any(np.isnan(mat['data']))
            if want in [int, np.int8, np.int16] and has_nan:
                print('Warning: new file is float16 rather than ', want, ' since we now have NaNs')
                mat['data'] = mat['data'].astype(np.float16)
            elif want in [np.int32] and has_nan:
                print('Warning: new file is float32 rather than ', want, ' since we now have NaNs')
                mat['data'] = mat['data'].astype(np.float32)
            elif want in [np.int64] and has_nan:
                print('Warning: new file is float64 rather than ', want, ' since we now have NaNs')
                mat['data'] = mat['data'].astype(np.float64)
            else:
                mat['data'] = mat['data'].astype(want)
        savemat(fn, mat)
