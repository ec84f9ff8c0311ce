#! /usr/bin/env python
# -*- coding: utf-8 -*-
"""``impplot``: ``rg``, ``traces``, ``power``, ``ft``, ``hft`` and ``spectrogram``, with the reference's option names
(``src/impdar/bin/impplot.py``), and two extensions: ``fk``, the f-k power spectrum in dB, and ``acorr``, the autocorrelogram.  What reads the whole radargram -- colour limits, the flattened image, the spectra -- is
computed on the MI355X (``impdar_amd/lib/plot.py``).

    python -m impdar_amd.bin.impplot rg [-s] [-o OUT] [--o_fmt png] [-dpi 300] [-xd] [-yd | -dualy] [-picks] [-clims LO HI]
                                        [-flatten_layer N] [-cmap gray] files
    python -m impdar_amd.bin.impplot traces [-yd | -dualy] ... files T_START T_END
    python -m impdar_amd.bin.impplot power ... files LAYER
    python -m impdar_amd.bin.impplot ft ... files
    python -m impdar_amd.bin.impplot hft ... files
    python -m impdar_amd.bin.impplot spectrogram files FREQ_LOWER FREQ_UPPER [-window W] [-scaling spectrum|density]
    python -m impdar_amd.bin.impplot fk ... files
    python -m impdar_amd.bin.impplot acorr [--maxlag L] ... files
"""
import argparse
import sys

from ..lib.load import FILETYPE_OPTIONS


def _get_args():
    parser = argparse.ArgumentParser()
    subparsers = parser.add_subparsers(help='sub-command help')
    rg = _add_parser(subparsers, 'rg', 'Plot radargram', plot_radargram)
    rg.add_argument('-xd', action='store_true', help='Plot the dist rather than the trace number')
    _add_depth_args(rg)
    rg.add_argument('-picks', action='store_true', help='Plot picks')
    rg.add_argument('-clims', nargs=2, type=float, help='Color limits')
    rg.add_argument('-flatten_layer', type=int, default=None, help='Distort plot so this layer is flat')
    rg.add_argument('-cmap', type=str, default='gray', help='Color map name')
    traces = _add_parser(subparsers, 'traces', 'Plot traces vs depth', plot_traces)
    _add_depth_args(traces)
    traces.add_argument('t_start', type=int, help='Starting trace number')
    traces.add_argument('t_end', type=int, help='Ending trace number')
    power = _add_parser(subparsers, 'power', 'Plot power on a layer', plot_power)
    power.add_argument('layer', type=int, help='Layer upon which to plot the power')
    _add_parser(subparsers, 'ft', 'Plot the power spectrum in the vertical', plot_ft)
    _add_parser(subparsers, 'hft', 'Plot the power spectrum in the horizontal', plot_hft)
    _add_parser(subparsers, 'fk', '(extension) Plot the f-k power spectrum', plot_fk)
    acorr = _add_parser(subparsers, 'acorr', '(extension) Plot the autocorrelation of every trace', plot_acorr)
    acorr.add_argument('--maxlag', type=int, default=None, help='Largest lag in samples (default: a quarter of the trace, at most 256)')
    spec = _add_parser(subparsers, 'spectrogram', 'Plot spectrogram for all traces', plot_spectrogram)
    spec.add_argument('freq_lower', type=float, help='Lower frequency bound')
    spec.add_argument('freq_upper', type=float, help='Upper frequency bound')
    spec.add_argument('-window', type=str, default=None, help='Window of the periodogram (default boxcar)')
    spec.add_argument('-scaling', type=str, default='spectrum', choices=['spectrum', 'density'],
                      help='Power spectrum or power spectral density (default spectrum)')
    return parser


def _add_parser(subparsers, name, helpstr, func):
    parser = subparsers.add_parser(name, help=helpstr)
    parser.set_defaults(func=func)
    parser.add_argument('fns', type=str, nargs='+', help='The files to process')
    parser.add_argument('-o', type=str, help='Output to this file (folder if multiple inputs)')
    parser.add_argument('-s', action='store_true', help='Save file (do not plt.show())')
    parser.add_argument('--o_fmt', type=str, default='png', help='Save file with this extension (default png)')
    parser.add_argument('-dpi', type=int, default=300, help='Save file with this resolution (default 300)')
    parser.add_argument('--in_fmt', type=str, help='Type of file', default='mat', choices=FILETYPE_OPTIONS)
    return parser


def _add_depth_args(parser):
    parser.add_argument('-yd', action='store_true', help='Plot the depth rather than travel time')
    parser.add_argument('-dualy', action='store_true', help='Primary y axis is TWTT, secondary is depth')


def plot_radargram(fns=None, s=False, o=None, xd=False, yd=False, o_fmt='png', dpi=300, in_fmt='mat', picks=False, clims=None,
                   cmap='gray', flatten_layer=None, dualy=False, **kwargs):
    """Plot the data as a radio echogram, with its picks and with a picked layer made flat if asked for."""
    from ..lib import plot
    plot.plot(fns, xd=xd, yd=yd, s=s, o=o, ftype=o_fmt, dpi=dpi, filetype=in_fmt, pick_colors=picks, cmap=cmap, clims=clims,
              flatten_layer=flatten_layer, dualy=dualy)


def plot_traces(fns=None, t_start=None, t_end=None, yd=False, dualy=False, s=False, o=None, o_fmt='png', dpi=300, in_fmt='mat',
                **kwargs):
    """Plot traces t_start to t_end as amplitude against travel time or depth."""
    from ..lib import plot
    plot.plot(fns, tr=(t_start, t_end), yd=yd, s=s, o=o, ftype=o_fmt, dpi=dpi, dualy=dualy, filetype=in_fmt)


def plot_power(fns=None, layer=None, s=False, o=None, o_fmt='png', dpi=300, in_fmt='mat', **kwargs):
    """Plot the power returned from a picked layer, all files on one axis."""
    from ..lib import plot
    plot.plot(fns, power=layer, s=s, o=o, ftype=o_fmt, dpi=dpi, filetype=in_fmt)


def plot_ft(fns=None, s=False, o=None, o_fmt='png', dpi=300, in_fmt='mat', **kwargs):
    """Plot the power spectrum along the samples: what frequencies the data holds."""
    from ..lib import plot
    plot.plot(fns, s=s, o=o, ftype=o_fmt, dpi=dpi, filetype=in_fmt, ft=True)


def plot_hft(fns=None, s=False, o=None, o_fmt='png', dpi=300, in_fmt='mat', **kwargs):
    """Plot the power spectrum along the traces: where a horizontal filter belongs."""
    from ..lib import plot
    plot.plot(fns, s=s, o=o, ftype=o_fmt, dpi=dpi, filetype=in_fmt, hft=True)


def plot_fk(fns=None, s=False, o=None, o_fmt='png', dpi=300, in_fmt='mat', **kwargs):
    """(extension) Plot the f-k power spectrum: where the fan of ``impproc fk`` is chosen."""
    from ..lib import plot
    plot.plot(fns, s=s, o=o, ftype=o_fmt, dpi=dpi, filetype=in_fmt, fk=True)


def plot_acorr(fns=None, maxlag=None, s=False, o=None, o_fmt='png', dpi=300, in_fmt='mat', **kwargs):
    """(extension) Plot the autocorrelogram: where ``--gap`` and ``--oplen`` of ``impproc decon`` are chosen."""
    from ..lib import plot
    return plot.plot(fns, s=s, o=o, ftype=o_fmt, dpi=dpi, filetype=in_fmt, acorr=True, maxlag=maxlag)


def plot_spectrogram(fns=None, freq_lower=None, freq_upper=None, window=None, scaling='spectrum', s=False, o=None,
                     o_fmt='png', dpi=300, in_fmt='mat', **kwargs):
    """Plot the periodogram of every trace."""
    from ..lib import plot
    plot.plot(fns, spectra=(freq_lower, freq_upper), window=window, scaling=scaling, s=s, o=o, ftype=o_fmt, dpi=dpi,
              filetype=in_fmt)


def main():
    parser = _get_args()
    args = parser.parse_args(sys.argv[1:])
    if not hasattr(args, 'func'):
        parser.parse_args(['-h'])
        return
    args.func(**vars(args))


if __name__ == '__main__':
    main()
