#! /usr/bin/env python
"""``impdar load TYPE files`` and ``impdar proc [-vbp LOW HIGH] [-ahfilt WIN] [-denoise V H] [-interp SPACING GPS_FN]
[-migrate X] files`` on the MI355X engine (reference ``src/impdar/bin/impdarexec.py:17-119,175-182`` ->
``load.load_and_exit`` / ``process.process_and_exit``).  ``load`` writes GSSI, pulseEKKO, RAMAC and Tek files as
``*_raw.mat``, which ``proc`` and ``impproc`` read; ``proc`` has these five steps."""
import argparse
import sys

from ..lib import loaders, process


def _get_args():
    parser = argparse.ArgumentParser()
    subparsers = parser.add_subparsers(help='Choose a processing step')
    parser_load = subparsers.add_parser('load', help='Load data')
    parser_load.set_defaults(func=loaders.load_and_exit)
    parser_load.add_argument('filetype', type=str, help='Type of file', choices=loaders.FILETYPE_OPTIONS)
    parser_load.add_argument('fns_in', type=str, nargs='+', help='File(s) to load')
    parser_load.add_argument('-channel', type=str, default='processed',
                             help='Receiver channel to load (kept for the reference\'s command line; the four '
                                  'instrument types here have one)')
    parser_load.add_argument('-gps_offset', type=float, default=0.0,
                             help='Offset of GPS and data times (kept for the reference\'s command line)')
    parser_load.add_argument('-t_srs', type=str, default=None,
                             help='Convert to this coordinate reference system (GDAL required; without it, no effect)')
    parser_load.add_argument('-s_srs', type=str, default=None,
                             help='Convert from this system (GDAL required; without it, no effect)')
    parser_load.add_argument('-o', type=str, help='Write to this filename')
    parser_load.add_argument('--nans', type=str, choices=['interp', 'delete'], default=None,
                             help='Interpolate or delete bad GPS (kept for the reference\'s command line)')
    parser_load.add_argument('-dname', type=str, default='data', help='Name of data field')

    parser_proc = subparsers.add_parser('proc', help='Process data')
    parser_proc.set_defaults(func=process.process_and_exit)
    parser_proc.add_argument('-vbp', nargs=2, type=float,
                             help='Bandpass the data vertically at low (MHz) and high (MHz)')
    parser_proc.add_argument('-ahfilt', nargs=1, type=int, help='Adaptive horizontal filtering')
    parser_proc.add_argument('-denoise', nargs=2, type=int,
                             help='Denoising filter vertical and horizontal (scipy wiener for now)')
    parser_proc.add_argument('-interp', nargs=2, type=str,
                             help='Reinterpolate GPS. First argument is the new spacing, in meters. Second argument '
                                  'is the filename with new GPS data (not supported by this engine)')
    parser_proc.add_argument('-migrate', type=str, help='Migrate with the indicated routine.')
    parser_proc.add_argument('fn', type=str, nargs='+', help='File(s) to process')
    parser_proc.add_argument('-o', type=str, help='Write to this filename')
    return parser


def main():
    parser = _get_args()
    args = parser.parse_args(sys.argv[1:])
    if not hasattr(args, 'func'):
        parser.parse_args(['-h'])
        return None
    kw = vars(args)
    func = kw.pop('func')
    return func(**kw)


if __name__ == '__main__':
    main()
