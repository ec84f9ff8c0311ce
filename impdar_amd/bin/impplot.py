#! /usr/bin/env python
# -*- coding: utf-8 -*-
"""``impplot`` for the spectra this engine computes: ``ft``, ``hft`` and ``spectrogram``, with the reference's option
names (``src/impdar/bin/impplot.py``).  The spectra are computed on the MI355X (``impdar_amd/lib/plot.py``); the
reference's other sub-commands (rg, traces, power) are not part of this engine.

    python -m impdar_amd.bin.impplot ft [-s] [-o OUT] [--o_fmt png] [-dpi 300] files
    python -m impdar_amd.bin.impplot hft ... files
    python -m impdar_amd.bin.impplot spectrogram files FREQ_LOWER FREQ_UPPER [-window W] [-scaling spectrum|density]
"""
import argparse
import sys

from ..lib.load import FILETYPE_OPTIONS


def _get_args():
    parser = argparse.ArgumentParser()
    subparsers = parser.add_subparsers(help='sub-command help')
    _add_parser(subparsers, 'ft', 'Plot the power spectrum in the vertical', plot_ft)
    _add_parser(subparsers, 'hft', 'Plot the power spectrum in the horizontal', plot_hft)
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


def plot_ft(fns=None, s=False, o=None, o_fmt='png', dpi=300, in_fmt='mat', **kwargs):
    """Plot the power spectrum along the samples: what frequencies the data holds."""
    from ..lib import plot
    plot.plot(fns, s=s, o=o, ftype=o_fmt, dpi=dpi, filetype=in_fmt, ft=True)


def plot_hft(fns=None, s=False, o=None, o_fmt='png', dpi=300, in_fmt='mat', **kwargs):
    """Plot the power spectrum along the traces: where a horizontal filter belongs."""
    from ..lib import plot
    plot.plot(fns, s=s, o=o, ftype=o_fmt, dpi=dpi, filetype=in_fmt, hft=True)


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
