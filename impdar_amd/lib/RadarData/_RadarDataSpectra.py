"""Spectra of the radargram where it is -- resident or on the host: what the reference's ``plot_ft``, ``plot_hft`` and
``plot_spectrogram`` (``src/impdar/lib/plot.py:286-365, 621-725``) compute before they draw, each with the axis the
reference plots it against.  Only the spectrum (``snum`` or ``tnum`` doubles) or the ``(snum // 2 + 1, tnum)`` image
comes back from the device.
"""
import numpy as np

from ... import spectra


def _shape(self):
    dev = getattr(self, '_dev', None)
    return dev.shape if dev is not None else np.shape(self.data)


def _mean(self, axis):
    dev = getattr(self, '_dev', None)
    if dev is not None:
        return spectra.mean_spectrum_dev(dev, axis)
    return spectra.mean_spectrum_host(self.data, axis)


def vertical_spectrum(self):
    """``(freq_mhz, power)``: the power spectrum along the samples, averaged over the traces, at the frequencies
    ``fftfreq(snum) / dt >= 0`` in MHz -- the curve of ``plot_ft``."""
    snum = _shape(self)[0]
    freq = np.fft.fftfreq(snum) / self.dt
    power = _mean(self, 0)
    keep = freq >= 0
    return freq[keep] / 1.0e6, power[keep]


def horizontal_spectrum(self):
    """``(wavelength, power)``: the power spectrum along the traces, averaged over the samples, against the
    wavelength ``flags.interp[1] / fftfreq(tnum)`` for the frequencies >= 0 (infinite at zero) -- the curve of
    ``plot_hft``.  The trace spacing comes from ``flags.interp``, as in the reference."""
    spacing = self.flags.interp[1]          # (the reference's error where interp is not a pair)
    tnum = _shape(self)[1]
    freq = np.fft.fftfreq(tnum)
    with np.errstate(divide='ignore', invalid='ignore'):
        wavelength = spacing / freq
        wavelength[freq == 0.0] = np.inf
    power = _mean(self, 1)
    keep = freq >= 0
    return wavelength[keep], power[keep]


def spectrogram(self, window=None, scaling='spectrum'):
    """``(freq_mhz, power)``: ``scipy.signal.periodogram`` of every trace with ``fs = 1 / dt`` -- ``power`` is the
    ``(snum // 2 + 1, tnum)`` image of ``plot_spectrogram``, ``freq_mhz = rfftfreq(snum, dt) / 1e6``."""
    fs = 1.0 / self.dt
    dev = getattr(self, '_dev', None)
    if dev is not None:
        freq, power = spectra.periodogram_dev(dev, fs, window=window, scaling=scaling)
    else:
        freq, power = spectra.periodogram_host(self.data, fs, window=window, scaling=scaling)
    return freq / 1.0e6, power
