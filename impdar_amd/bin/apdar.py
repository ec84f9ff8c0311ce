#! /usr/bin/env python
"""``apdar``: single actions on ApRES files from the command line, with the reference's sub-commands, options,
defaults and output names (``src/impdar/bin/apdar.py``).

    apdar load -acq_type single a.DAT b.DAT      ->  a_apraw.mat
    apdar proc a_apraw.mat                       ->  a_proc.mat

Every sub-command but ``load`` first loads its files; without ``-acq_type`` it tries a single acquisition, then a
time difference, then a quad-polarized set, and fails with one error that lists what each attempt said.  ``plot`` is
accepted and raises ``NotImplementedError``: the ApRES plots are not in this package."""
import argparse
import os.path
import sys

import numpy as np

from ..lib.ApresData import load_apres, load_quadpol, load_time_diff
from ..lib.ImpdarError import ImpdarError


def _get_args():
    parser = argparse.ArgumentParser()
    subparsers = parser.add_subparsers(help='Choose a processing step')

    parser_load = _add_procparser(subparsers, 'load', 'load apres data', load, defname='load')
    parser_load.add_argument('-acq_type', type=str, help='Acquisition type', default='single',
                             choices=['single', 'timediff', 'quadpol'])
    _add_def_args(parser_load)

    parser_singleproc = _add_procparser(subparsers, 'proc', 'full processing flow on the apres data object',
                                        single_processing, 'proc')
    parser_singleproc.add_argument('-max_range', type=float, help='maximum range for the range conversion')
    parser_singleproc.add_argument('-num_chirps', type=int, help='number of chirps to stack (default: stack all)')
    parser_singleproc.add_argument('-noise_bed_range', type=float,
                                   help='bed range under which the noise phasor will be calculated')
    parser_singleproc.set_defaults(max_range=4000., num_chirps=0, noise_bed_range=3000.)
    _add_def_args(parser_singleproc)

    parser_diffproc = _add_procparser(subparsers, 'diffproc',
                                      'create an ApresDiff object and then execute the full differencing processing flow',
                                      time_diff_processing, 'diffproc')
    parser_diffproc.add_argument('-window', type=int, help='window size over which the cross correlation is done')
    parser_diffproc.add_argument('-step', type=int, help='step size in samples for the moving window')
    parser_diffproc.add_argument('-thresh', type=int, help='coherence threshold for the unwrapping')
    parser_diffproc.add_argument('-strain_window', type=tuple, help='range window for the strain-rate regression')
    parser_diffproc.add_argument('-w_surf', type=float, help='surface vertical velocity (ice equivalent accumulation rate)')
    parser_diffproc.set_defaults(window=20, step=20, thresh=0.95, strain_window=(200, 1000), w_surf=-0.15)
    _add_def_args(parser_diffproc)

    parser_qpproc = _add_procparser(subparsers, 'qpproc', 'full processing flow on the quadpol data object',
                                    quadpol_processing, 'qpproc')
    parser_qpproc.add_argument('-nthetas', type=int, help='number of theta values to rotate into')
    parser_qpproc.add_argument('-dtheta', type=float, help='size of coherence window in theta direction')
    parser_qpproc.add_argument('-drange', type=float, help='size of coherence window in range direction')
    parser_qpproc.add_argument('-cross_pol_flip', type=str, help='flip the sign on one of the cross polarized terms.')
    parser_qpproc.set_defaults(nthetas=100, dtheta=20. * np.pi / 180., drange=100, cross_pol_flip=False)
    _add_def_args(parser_qpproc)

    parser_range = _add_procparser(subparsers, 'range', 'convert the recieved waveform to a range-amplitude array',
                                   range_conversion, 'range')
    parser_range.add_argument('-max_range', type=float, help='maximum range for the range conversion', default=4000.)
    _add_def_args(parser_range)

    parser_stack = _add_procparser(subparsers, 'stack', 'stack apres chirps into a single array', stack, 'stacked')
    parser_stack.add_argument('-num_chirps', type=int, help='number of chirps to stack (default: stack all)', default=0)
    _add_def_args(parser_stack)

    parser_unc = _add_procparser(subparsers, 'uncertainty', 'calculate the phase uncertainty for all samples', uncertainty,
                                 'uncertainty')
    parser_unc.add_argument('-noise_bed_range', type=float, help='bed range under which the noise phasor will be calculated',
                            default=3000.)
    _add_def_args(parser_unc)

    parser_pdiff = _add_procparser(subparsers, 'pdiff', 'calculate correlation between the two acquisitions',
                                   phase_differencing, 'pdiff')
    parser_pdiff.add_argument('-window', type=int, help='window size over which the cross correlation is done')
    parser_pdiff.add_argument('-step', type=int, help='step size in samples for the moving window')
    parser_pdiff.set_defaults(window=20, step=20)
    _add_def_args(parser_pdiff)

    # (no name of their own in the reference: its default, 'proc')
    parser_unwrap = _add_procparser(subparsers, 'unwrap', 'unwrap the differenced phase profile from top to bottom', unwrap)
    _add_def_args(parser_unwrap)
    parser_rdiff = _add_procparser(subparsers, 'rdiff', 'convert the differenced phase profile to range', range_differencing)
    _add_def_args(parser_rdiff)

    parser_rotate = _add_procparser(subparsers, 'rotate', 'use a rotational transform to find data at all azimuths', rotate,
                                    'rotated')
    parser_rotate.add_argument('-nthetas', type=int, help='number of theta values to rotate into', default=100)
    parser_rotate.add_argument('-cross_pol_flip', type=str, help='flip the sign on one of the cross polarized terms.',
                               default=False)
    _add_def_args(parser_rotate)

    parser_coherence = _add_procparser(subparsers, 'coherence', '2-dimensional coherence between HH and VV polarizations',
                                       coherence, 'chhvv')
    parser_coherence.add_argument('-dtheta', type=float, help='size of coherence window in theta direction')
    parser_coherence.add_argument('-drange', type=float, help='size of coherence window in range direction')
    parser_coherence.set_defaults(dtheta=20. * np.pi / 180., drange=100.)
    _add_def_args(parser_coherence)

    parser_cpe = _add_procparser(subparsers, 'cpe', 'find the depth-azimuth profile for cross-polarized extinction',
                                 cross_polarized_extinction, 'cpe')
    parser_cpe.add_argument('-Wn', type=float, help='filter frequency')
    parser_cpe.add_argument('-fs', type=float, help='sampling frequency')
    _add_def_args(parser_cpe)

    parser_plot = _add_procparser(subparsers, 'plot', 'plot apres data from a single acquisition', plot_apres, 'plot')
    parser_plot.add_argument('-acq_type', type=str, help='Acquisition type', default=None,
                             choices=['single', 'timediff', 'quadpol'])
    parser_plot.add_argument('-s', action='store_true', help='Save file (do not plt.show())')
    parser_plot.add_argument('-yd', action='store_true', help='plot the depth rather than travel time')
    _add_def_args(parser_plot)
    return parser


def _add_procparser(subparsers, name, helpstr, func, defname='proc'):
    parser = subparsers.add_parser(name, help=helpstr)
    parser.set_defaults(func=func, name=defname)
    return parser


def _add_def_args(parser):
    parser.add_argument('fns', type=str, nargs='+', help='The files to process')
    parser.add_argument('-o', type=str, help='Output to this file (folder if multiple inputs)')


def output_name(fns, name, o=None):
    """``-o`` as given; else the first file's name without its extension -- and without a trailing ``_??raw`` where
    it ends in ``raw`` -- plus ``_{name}.mat`` (reference :277-285)."""
    if o is not None:
        return o
    bn = os.path.splitext(fns[0])[0]
    if bn[-3:] == 'raw':
        bn = bn[:-6]
    return bn + '_{:s}.mat'.format(name)


def main(argv=None):
    """Parse, load, run the step, save."""
    parser = _get_args()
    args = parser.parse_args(sys.argv[1:] if argv is None else argv)
    if not hasattr(args, 'func'):
        parser.parse_args(['-h'])

    if args.name == 'plot':
        return args.func(None, **vars(args))
    if args.name == 'load':
        apres_data, name = args.func(**vars(args))
    else:
        apres_data, empty_name = load(**{**vars(args), 'acq_type': getattr(args, 'acq_type', None)})
        name = args.name
        args.func(apres_data, **vars(args))
    apres_data.save(output_name(args.fns, name, args.o))


# ------------------------------------------------------------------------------------------------ loading
def _load_single(fns):
    return load_apres.load_apres(fns), 'apraw'


def _load_timediff(fns):
    if len(fns) == 1:
        return load_time_diff.load_time_diff(fns[0], load_single_acquisitions=False), 'tdraw'
    return load_time_diff.load_time_diff(fns), 'tdraw'


def _load_quadpol(fns):
    if len(fns) == 1:
        return load_quadpol.load_quadpol(fns[0], load_single_pol=False), 'qpraw'
    return load_quadpol.load_quadpol(fns), 'qpraw'


_LOADERS = (('single', _load_single), ('timediff', _load_timediff), ('quadpol', _load_quadpol))


def load(fns='', acq_type=None, **kwargs):
    """``(object, name)`` of the files as ``acq_type``; without one the first of single, timediff and quadpol that
    loads (the reference tries all three behind bare ``except``s and keeps the last that did, :308-329)."""
    if acq_type is not None:
        return dict(_LOADERS)[acq_type](fns)
    said = []
    for kind, loader in _LOADERS:
        try:
            return loader(fns)
        except Exception as exc:
            said.append('%s: %s: %s' % (kind, type(exc).__name__, exc))
            if kind == 'single':
                said[-1] += _why_no_file_loaded(fns)
    raise ImpdarError('Cannot load %s as any acquisition type (%s)' % (', '.join(fns), '; '.join(said)))


def _why_no_file_loaded(fns):
    """``load_apres`` leaves out a file that does not load, as the reference does, and fails on the empty list that may
    remain: what the first such file said when loaded alone."""
    for fn in fns:
        try:
            load_apres.load_apres_single_file(fn)
        except Exception as exc:
            return ' (%s: %s: %s)' % (fn, type(exc).__name__, exc)
    return ''


# ------------------------------------------------------------------------------------------------ full flows
def single_processing(dat, p=2, max_range=4000., num_chirps=0., noise_bed_range=3000., **kwargs):
    """Range conversion, stacking, uncertainty (the converted chirps stay in HBM between the first two)."""
    dat.single_processing(p=p, max_range=max_range, num_chirps=num_chirps, noise_bed_range=noise_bed_range)


def time_diff_processing(diffdat, window=20, step=20, thresh=0.95, strain_window=(200, 1000), w_surf=-0.15, **kwargs):
    """Phase difference, unwrapping, range difference, strain rate, bed pick.  (The reference names the parameter
    ``win`` and the option ``-window``, so that its option never arrives, :348; here it does.)"""
    diffdat.phase_diff(window, step)
    diffdat.phase_unwrap(window, thresh)
    diffdat.range_diff()
    diffdat.strain_rate(strain_window=strain_window, w_surf=w_surf)
    diffdat.bed_pick()


def quadpol_processing(dat, nthetas=100, dtheta=20.0 * np.pi / 180., drange=100., cross_pol_flip=False, **kwargs):
    """Rotation, cross-polarized extinction (at the default ``Wn`` of ``find_cpe``: the reference passes none),
    coherence."""
    dat.rotational_transform(n_thetas=nthetas, cross_pol_flip=cross_pol_flip)
    dat.find_cpe()
    dat.coherence2d(delta_theta=dtheta, delta_range=drange)


# ------------------------------------------------------------------------------------------------ single steps
def range_conversion(dat, p=2, max_range=4000, **kwargs):
    dat.apres_range(p, max_range)


def stack(dat, num_chirps=0, **kwargs):
    if num_chirps == 0:
        dat.stacking()
    else:
        dat.stacking(num_chirps)


def uncertainty(dat, noise_bed_range=3000, **kwargs):
    dat.phase_uncertainty(noise_bed_range)


def phase_differencing(diffdat, window=20, step=20, **kwargs):
    diffdat.phase_diff(window, step)


def unwrap(diffdat, win=20, thresh=.95, **kwargs):
    diffdat.phase_unwrap(win, thresh)


def range_differencing(diffdat, **kwargs):
    diffdat.range_diff()


def rotate(dat, nthetas=100, cross_pol_flip=False, **kwargs):
    dat.rotational_transform(n_thetas=nthetas, cross_pol_flip=cross_pol_flip)


def coherence(dat, dtheta=20.0 * np.pi / 180., drange=100., **kwargs):
    dat.coherence2d(delta_theta=dtheta, delta_range=drange)


def cross_polarized_extinction(dat, Wn=None, fs=0., **kwargs):
    """``find_cpe`` at ``-Wn``, or at its default without the option."""
    if Wn is None:
        dat.find_cpe()
    else:
        dat.find_cpe(Wn=Wn)


def plot_apres(dat, acq_type=None, s=False, o=None, **kwargs):
    raise NotImplementedError('apdar plot: the ApRES plots are not part of this package')


if __name__ == '__main__':
    main()
