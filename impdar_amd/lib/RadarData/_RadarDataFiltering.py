"""``RadarData.migrate``: the string dispatch into the migration library
(reference ``src/impdar/lib/RadarData/_RadarDataFiltering.py:590-637``: same
mtype names, per-mtype keyword forwarding, defaults, ValueError for unknown
names, ``flags.mig`` recorded afterwards), ``RadarData.vertical_band_pass``
(``:469-549``), the horizontal filters ``hfilt`` / ``horizontalfilt`` / ``adaptivehfilt`` (``:19-135``,
``:443-466``), ``winavg_hfilt`` (``:353-440``), ``denoise`` (``:552-587``) and the horizontal frequency filters ``horizontal_band_pass`` /
``highpass`` / ``lowpass`` (``:138-350``), the filters an impproc chain runs in front of a migration."""
import numpy as np

from .. import migrationlib
from ... import denoise as _dn
from ... import hfilt as _hf
from ... import hpass as _hp
from ... import preproc
from ._resident import data_shape as _data_shape, replace_data as _replace_data, update_data as _update_data


def adaptivehfilt(self, window_size, *args, **kwargs):
    """Subtract from every trace the mean of the ``window_size`` traces around it, smoothed vertically
    (``filtfilt([.25] * 4, 1, .)``) and tapered with travel time; the reference's windows, including their
    edge branches and empty windows (NaN traces).  The filtering runs on the MI355X whatever the window."""
    print('Adaptive filtering')
    snum, tnum = _data_shape(self)
    lo, hi = _hf.ahfilt_windows(tnum, window_size)
    scale = _hf.taper(self.travel_time)
    _update_data(self, lambda dev: _hf.ahfilt_dev(dev, lo, hi, scale), lambda data: _hf.ahfilt_host(data, lo, hi, scale))
    print('Adaptive filtering complete')
    self.flags.hfilt[0] = 1
    self.flags.hfilt[1] = 4


def winavg_hfilt(self, avg_win, taper='full', filtdepth=100):
    """Subtract from every trace the mean of the ``avg_win`` traces around it (made odd and at most ``tnum``,
    with the reference's messages; the window is the reference's half-open one, so the trace ``avg_win // 2``
    to the right is not in it and ``avg_win = 1`` gives NaN), tapered with travel time: ``taper='full'`` as
    ``adaptivehfilt``, ``'pexp'`` down to zero at sample ``filtdepth``.  ``'tukey'`` fails in the reference on an
    undefined name and raises ``NotImplementedError`` here.  The filtering runs on the MI355X whatever the
    window."""
    snum, tnum = _data_shape(self)
    avg_win = _hf.winavg_window(avg_win, self.tnum)
    scale = _hf.winavg_taper(self.travel_time, taper, filtdepth)
    lo, hi = _hf.winavg_windows(tnum, avg_win)
    _update_data(self, lambda dev: _hf.winavg_dev(dev, lo, hi, scale), lambda data: _hf.winavg_host(data, lo, hi, scale))
    self.flags.hfilt = np.zeros((2,))
    self.flags.hfilt[1] = 2
    print('Horizontal filter complete.')


def horizontalfilt(self, ntr1, ntr2, *args, **kwargs):
    """Subtract the tapered mean of traces ``ntr1`` to ``ntr2`` (clamped as the reference clamps them) from
    every trace, in the data's own dtype."""
    snum, tnum = _data_shape(self)
    htr1, htrn = _hf.hfilt_bounds(ntr1, ntr2, tnum)
    print('Subtracting mean trace found between {:d} and {:d}'.format(htr1, htrn))
    scale = _hf.taper(self.travel_time)
    _update_data(self, lambda dev: _hf.hfilt_dev(dev, htr1, htrn, scale), lambda data: _hf.hfilt_host(data, htr1, htrn, scale))
    print('Horizontal filter complete.')
    self.flags.hfilt = np.ones((2,))


def hfilt(self, ftype='hfilt', bounds=None, window_size=None):
    """Horizontally filter the data: ``ftype`` 'hfilt' (``bounds`` = (first, last) trace of the mean) or
    'adaptive' (``window_size`` traces in the moving mean)."""
    if ftype == 'hfilt':
        self.horizontalfilt(bounds[0], bounds[1])
    elif ftype == 'adaptive':
        self.adaptivehfilt(window_size=window_size)
    else:
        raise ValueError('Unrecognized filter type')


def denoise(self, vert_win=1, hor_win=10, noise=None, ftype='wiener'):
    """Denoising filter over a (``vert_win`` samples, ``hor_win`` traces) window, on the MI355X.

    ``ftype='wiener'``: ``scipy.signal.wiener(data, mysize=(vert_win, hor_win), noise=noise)``; the data becomes
    float64, as in the reference (a resident float32 radargram becomes a resident float64 one).  ``noise`` is the
    noise power, by default the mean of the local variance.  ``ftype='median'``:
    ``scipy.ndimage.median_filter(data, size=(vert_win, hor_win))``, in the data's own dtype.  Any other ftype
    raises ``ValueError`` as the reference does.

    Deliberate differences from the reference: integer data is widened to float64 before it is
    squared (the reference's int16 squares wrap); with ``noise=None`` a flat window gives its mean instead of
    raising, and ``ValueError('Could not compute variance, specify noise for denoise')`` is raised only when
    every window is flat (estimated noise exactly 0); window sizes below 1 raise ``ValueError``; with ``noise``
    given, an output is NaN exactly when its window holds a non-finite value (with ``noise=None`` every output
    is, as in the reference).
    """
    if ftype not in ('wiener', 'median'):
        raise ValueError(_dn.FTYPE_MESSAGE)
    if ftype == 'wiener':
        # both forms return (result, noise used)
        _replace_data(self, lambda dev: _dn.wiener_dev(dev, vert_win, hor_win, noise=noise)[0],
                      lambda data: _dn.wiener_host(data, vert_win, hor_win, noise=noise)[0])
    else:
        _replace_data(self, lambda dev: _dn.median_dev(dev, vert_win, hor_win), lambda data: _dn.median_host(data, vert_win, hor_win))


def _hpass_apply(self, spec):
    # a resident float64 radargram is filtered in place and handed back: nothing is freed then
    _replace_data(self, lambda dev: _hp.filtfilt_dev(dev, spec), lambda data: _hp.filtfilt_host(data, spec))
    self.flags.hfilt = np.ones((2,))
    self.flags.hfilt[1] = 3


def horizontal_band_pass(self, low, high):
    """Band-pass every sample row along the traces between the wavelengths ``low`` and ``high`` (m):
    ``filtfilt(butter(5, corners, 'bandpass'), data, axis=1)`` on the MI355X, float64 out.  Needs constantly
    spaced (``constant_space``), not elevation-corrected data; the reference's checks, messages and corner
    frequencies.  A resident float32 radargram becomes a resident float64 one.  Integer data is widened to
    float64 before the odd extension (the reference's int16 extension wraps)."""
    tracespace = _hp.trace_spacing(self.flags)
    _hpass_apply(self, _hp.band_pass_design(low, high, tracespace, self.tnum))
    print('Highpass filter complete.')


def highpass(self, wavelength):
    """High pass along the traces for ``wavelength`` (m): ``filtfilt(butter(5, c, 'high'), data)`` with the
    reference's corner ``c = (100 / nsamp) MHz / (0.5 / dt)``, on the MI355X, float64 out (see
    :func:`horizontal_band_pass` for the checks, residency and integer data)."""
    tracespace = _hp.trace_spacing(self.flags)
    _hpass_apply(self, _hp.pass_design('high', wavelength, tracespace, self.tnum, self.dt))
    print('Highpass filter complete.')


def lowpass(self, wavelength):
    """Low pass along the traces for ``wavelength`` (m): ``filtfilt(butter(3, c, 'low'), data)``, corner as in
    :func:`highpass`."""
    tracespace = _hp.trace_spacing(self.flags)
    _hpass_apply(self, _hp.pass_design('low', wavelength, tracespace, self.tnum, self.dt))
    print('Lowpass filter complete.')


def vertical_band_pass(self, low, high, order=5, filttype='butter', cheb_rp=5, fir_window='hamming',
                       *args, **kwargs):
    """Band-pass every trace along time between ``low`` and ``high`` MHz: forward-backward IIR
    (butter / cheb / bessel) or a delayed-and-shifted FIR; same designs, padding and initial conditions as
    the reference (SciPy), the filtering itself on the MI355X."""
    spec = preproc.design_filter(self.dt, low, high, order=order, filttype=filttype, cheb_rp=cheb_rp)
    print('Bandpassing from {:4.1f} to {:4.1f} MHz...'.format(low, high))
    _update_data(self, lambda dev: preproc.filter_dev(dev, spec), lambda data: preproc.filter_host(data, spec))
    print('Bandpass filter complete.')
    self.flags.bpass[0] = 1
    self.flags.bpass[1] = low
    self.flags.bpass[2] = high


def migrate(self, mtype='stolt', vtaper=10, htaper=10, tmig=0, vel_fn=None, vel=1.68e8,
            nxpad=10, nearfield=False, verbose=0):
    """Migrate the data in place.  mtype: 'kirch', 'stolt', 'phsh', 'tk' or 'su*'."""
    if getattr(self, '_dev', None) is not None:
        # radargram held in HBM (to_device): Kirchhoff and Stolt run on it where it is
        from ... import resident
        if mtype == 'kirch':
            resident.kirchhoff_resident(self, vel=vel, nearfield=nearfield)
        elif mtype == 'stolt':
            resident.stolt_resident(self, vel=vel, htaper=htaper, vtaper=vtaper)
        elif mtype == 'phsh':
            migrationlib.mig_hip._phase_shift(self, vel, vel_fn, htaper, vtaper, {}, self._dev)
        else:
            self.from_device()
            migrate(self, mtype=mtype, vtaper=vtaper, htaper=htaper, tmig=tmig, vel_fn=vel_fn, vel=vel,
                    nxpad=nxpad, nearfield=nearfield, verbose=verbose)
            self.to_device()
            return
        self.flags.mig = mtype
        return
    if mtype == 'kirch':
        migrationlib.migrationKirchhoff(self, vel=vel, nearfield=nearfield)
    elif mtype == 'stolt':
        migrationlib.migrationStolt(self, vel=vel, htaper=htaper, vtaper=vtaper)
    elif mtype == 'phsh':
        migrationlib.migrationPhaseShift(self, vel=vel, vel_fn=vel_fn, htaper=htaper, vtaper=vtaper)
    elif mtype == 'tk':
        migrationlib.migrationTimeWavenumber(self, vel=vel, vel_fn=vel_fn, htaper=htaper, vtaper=vtaper)
    elif mtype[:2] == 'su':
        migrationlib.migrationSeisUnix(self, mtype=mtype, vel=vel, vel_fn=vel_fn, tmig=tmig,
                                       verbose=verbose, nxpad=nxpad, htaper=htaper, vtaper=vtaper)
    else:
        raise ValueError('Unrecognized migration routine')
    self.flags.mig = mtype
