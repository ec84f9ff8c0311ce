"""The three spectral plots of the reference's ``lib/plot.py`` -- ``plot_ft``, ``plot_hft`` and ``plot_spectrogram``
(``src/impdar/lib/plot.py:286-365, 621-725``) -- with its signatures, defaults, labels, title and ``freq_limit`` checks,
drawing what ``RadarData.vertical_spectrum``, ``horizontal_spectrum`` and ``spectrogram`` compute on the MI355X (on the
resident radargram when there is one).  ``plot`` wraps these three kinds for the ``impplot`` executable.  The reference's
other plots (radargram, traces, power, picks, ApRES) are not part of this engine.

matplotlib is imported inside the functions: ``import impdar_amd`` does not pull it in.
"""
import os

import numpy as np

from .load import load


def _axes(fig, ax, figsize):
    import matplotlib.pyplot as plt
    if fig is not None:
        if ax is None:
            ax = plt.gca()
    else:
        fig, ax = plt.subplots(figsize=figsize)
    return fig, ax


def plot(fns, s=False, ftype='png', dpi=300, spectra=None, window=None, scaling='spectrum', filetype='mat', ft=False,
         hft=False, *args, **kwargs):
    """Load every file of ``fns`` and draw its vertical spectrum (``ft``), horizontal spectrum (``hft``) or spectrogram
    (``spectra``, the pair of frequency limits in MHz); save next to the input with extension ``ftype`` (``s``) or
    show."""
    import matplotlib.pyplot as plt
    radar_data = load(filetype, fns)
    if ft:
        figs = [plot_ft(dat) for dat in radar_data]
    elif hft:
        figs = [plot_hft(dat) for dat in radar_data]
    elif spectra:
        figs = [plot_spectrogram(dat, spectra, window=window, scaling=scaling) for dat in radar_data]
    else:
        raise ValueError('this engine plots ft, hft and spectra; use the reference\'s impplot for the other kinds')
    for fig, dat in zip(figs, radar_data):
        manager = getattr(fig[0].canvas, 'manager', None)
        if dat.fn is not None and manager is not None:
            manager.set_window_title(dat.fn)
    if s:
        for fig, fn0 in zip(figs, fns):
            fig[0].savefig(os.path.splitext(fn0)[0] + '.' + ftype, dpi=dpi)
    else:
        plt.tight_layout()
        plt.show()
    return figs


def plot_ft(dat, fig=None, ax=None, **line_kwargs):
    """Plot the mean power spectrum along the samples against the frequency in MHz; ``line_kwargs`` go to the line."""
    freq_mhz, power = dat.vertical_spectrum()
    fig, ax = _axes(fig, ax, (12, 8))
    ax.plot(freq_mhz, power, **line_kwargs)
    ax.set_xlabel('Freq (MHz)')
    ax.set_ylabel('Power spectral density')
    return fig, ax


def plot_hft(dat, fig=None, ax=None):
    """Plot the mean power spectrum along the traces against the horizontal wavelength."""
    wavelength, power = dat.horizontal_spectrum()
    fig, ax = _axes(fig, ax, (12, 8))
    ax.plot(wavelength, power)
    ax.set_xlabel('Wavelength')
    ax.set_ylabel('Power spectral density')
    return fig, ax


def plot_spectrogram(dat, freq_limit=None, window=None, scaling='spectrum', fig=None, ax=None, **kwargs):
    """Filled contours of the periodogram of every trace: trace number against frequency in MHz.  ``freq_limit``: the
    pair (low, high) in MHz the frequency axis is limited to; ``window`` and ``scaling`` as
    ``scipy.signal.periodogram`` takes them."""
    import matplotlib.pyplot as plt
    y, power = dat.spectrogram(window=window, scaling=scaling)
    xx, yy = np.meshgrid(dat.trace_num, y)
    fig, ax = _axes(fig, ax, (10, 7))
    contours = ax.contourf(xx, yy, power)
    cbar = plt.colorbar(contours, shrink=0.9, orientation='vertical', pad=0.03, ax=ax)
    cbar.set_label('Power (Amplitude **2)')
    if freq_limit is not None:
        if hasattr(freq_limit, '__len__'):
            if freq_limit[1] < np.nanmin(y):
                raise ValueError('Y-axis limit {} MHz too low.'.format(freq_limit[1]))
            if freq_limit[1] > np.nanmax(y):
                print('Warning: y-axis limit large compared to the frequencies plotted')
            ax.set_ylim(freq_limit[0], freq_limit[1])
        else:
            print('Frequency limit should be a tuple of low, high. Ignoring.')
    ax.set_xlabel('Trace Number')
    ax.set_ylabel('Frequency (MHz)')
    ax.set_title('PSD(tnum, f)')
    return fig, ax
