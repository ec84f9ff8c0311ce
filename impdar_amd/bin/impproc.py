#! /usr/bin/env python
"""``impproc migrate`` (and the steps usually run around it, ``vbp``, ``hfilt``, ``ahfilt``, ``denoise``,
``interp``, ``geolocate``, ``hbp``, ``lp``, ``crop``, ``nmo``, ``elev``, ``rev``, ``hcrop``, ``restack``, ``rgain`` and ``agc``) on the
MI355X engine, and ``autopick``, an extension: ``impproc autopick files --snums S ... --tnums T ... [--freq F] [--pol +-1]
[--picknums N ...]`` picks one layer per seed (the reference's ``picklib.auto_pick``, which its GUI drives) and
writes ``<name>_picked.mat``; the files come before the seed lists, which take every number that follows them.
``impproc vscan VMIN VMAX NV [--htaper --vtaper --traces T0 T1 --samples S0 S1 --gates G --migrate] files``, another
extension, scans the focus of the Stolt image over NV velocities (``RadarData.velocity_scan``), prints and saves it
(``<name>_vscan.mat``) and, with ``--migrate``, migrates at the best one (``<name>_migrated.mat``).
``impproc fk [--va_lo V] [--va_hi V] [--taper T] [--mode pass|reject] [--dip both|down_right|down_left] files``, a third
extension, is the f-k fan (dip) filter (``RadarData.fk_filter``) and writes ``<name>_fk.mat``.
``impproc decon --oplen N [--gap G] [--prewhiten P] [--window S0 S1] [--design each|mean] files``, a fourth, is predictive
deconvolution (``RadarData.predictive_decon``) and writes ``<name>_decon.mat``.
``impproc attr --kind envelope|phase|frequency [--smooth W] files``, a fifth, replaces every trace by a complex-trace
attribute (``RadarData.envelope``, ``instantaneous_phase``, ``instantaneous_frequency``) and writes ``<name>_env.mat``,
``<name>_phase.mat`` or ``<name>_ifreq.mat``.
``impproc dipsmooth HALF [--sigma SZ SX] [--max_slope P] files``, a sixth, averages every sample over ``2 HALF + 1`` traces
along the layers' local slope (``RadarData.dip_smooth``) and writes ``<name>_dipsm.mat``; ``impproc slope --kind
slope|dip|coherence [--sigma SZ SX] [--max_slope P] files`` replaces the data by that field (``RadarData.layer_slope``) and
writes ``<name>_slope.mat``, ``<name>_dip.mat`` or ``<name>_coh.mat``, which ``impplot rg`` shows.

Mirrors these sub-commands of the reference's ``src/impdar/bin/impproc.py`` (migrate parser ``:295-343``,
hfilt ``:30-43``, ahfilt ``:46-54``, vbp ``:113-125``, hbp ``:128-139``, lp ``:141-146``, interp ``:222-251``,
geolocate ``:253-272``, ``geolocate`` ``:494-500``, denoise ``:275-293``, ``main`` ``:378-415``, ``hfilt`` ``:418-420``, ``ahfilt`` ``:423-425``, ``mig``
``:508-519``, ``vbp`` ``:438-440``, ``hbp`` ``:443-445``, ``lp`` ``:448-450``, ``interp`` ``:483-491``,
``denoise`` ``:503-505``; crop parser ``:152-171``, nmo ``:193-220``, elev ``:71-75``, ``elev`` ``:433-435``,
``crop`` ``:453-455``, ``nmo`` ``:463-465``; rev parser ``:57-61``, restack ``:78-87``, rgain ``:90-99``, agc
``:102-111``, hcrop ``:174-190``, ``rev`` ``:428-430``, ``hcrop`` ``:458-460``, ``restack`` ``:468-470``, ``rgain``
``:473-475``, ``agc`` ``:478-480``): same options, types and defaults, same output naming
(``<name minus _raw>_<migrated|hfilted|ahfilt|bandpassed|hbp|lp|interp|geolocate|denoise|cropped|nmo|elev|rev|hcropped|restacked|rgain|agc>.mat``, ``-o`` file or
folder).  As in the reference, ``impproc ahfilt WIN`` parses ``WIN`` but filters with the function's default
window of 1000 traces.  ``impproc denoise V H`` accepts ``--filt weiner|wiener|median`` (default ``weiner``, the reference's
spelling, which runs the Wiener filter; the reference's own default fails in its ``RadarData.denoise``).
As in the reference, ``impproc nmo --const_firn_offset X`` parses ``X`` and does not forward it.
As in the reference, ``impproc agc`` has no option for the scaling factor and gains with the function's default of 50.
``impproc geolocate FILE [--extrapolate] [--guess]`` attaches a precision GPS track (``gpslib.interp``); with ``--guess``
the clock offset between radar and GPS is searched on the MI355X.  ``impproc interp --gps_fn`` stays refused: run
``geolocate`` first, then ``interp`` on its output.
The reference's other processing sub-commands (``cat`` and the rest) are out of scope.

    python -m impdar_amd.bin.impproc migrate --mtype kirch line1_raw.mat
"""
import argparse
import os
import sys

from ..lib.load import load, FILETYPE_OPTIONS
from ..lib.gpslib import interp as interpdeep


SLOPE_NAMES = {'slope': 'slope', 'dip': 'dip', 'coherence': 'coh'}                # `impproc slope --kind`: the output's suffix
ATTR_NAMES = {'envelope': 'env', 'phase': 'phase', 'frequency': 'ifreq'}      # `impproc attr --kind`: the output's suffix


def _get_args():
    parser = argparse.ArgumentParser()
    subparsers = parser.add_subparsers(help='Choose a processing step')
    parser_mig = subparsers.add_parser('migrate', help='Migration')
    parser_mig.set_defaults(func=mig, name='migrated')
    parser_mig.add_argument('--mtype', type=str, default='phsh',
                            choices=['stolt', 'kirch', 'phsh', 'tk', 'sumigtk', 'sustolt', 'sumigffd'],
                            help='Migration routines.')
    parser_mig.add_argument('--vel', type=float, default=1.69e8,
                            help='Speed of light in dielectric medium m/s (default is for ice, 1.69e8)')
    parser_mig.add_argument('--vel_fn', type=str, default=None,
                            help='Filename for input velocity array. Column 1: velocities, '
                                 'Column 2: z locations, Column 3: x locations (optional)')
    parser_mig.add_argument('--nearfield', action='store_true',
                            help='Boolean for nearfield operator in Kirchhoff migration.')
    parser_mig.add_argument('--htaper', type=int, default=100, help='Number of samples for horizontal taper')
    parser_mig.add_argument('--vtaper', type=int, default=1000, help='Number of samples for vertical taper')
    parser_mig.add_argument('--nxpad', type=int, default=100, help='Number of traces to pad with zeros for FFT')
    parser_mig.add_argument('--tmig', type=int, default=0, help='Times for velocity profile')
    parser_mig.add_argument('--verbose', type=int, default=1, help='Print output from SeisUnix migration')
    parser_mig.add_argument('--gpus', type=int, default=0,
                            help='(extension) shard a Kirchhoff (output-trace blocks) or constant-v / v(z) phase-shift (wavenumber '
                                 'slabs) migration over this many MI355X of the node '
                                 '(default: $IMPDAR_NGPUS, else one)')
    _add_def_args(parser_mig)

    parser_hfilt = subparsers.add_parser('hfilt', help='Horizontally filter the data by subtracting the average '
                                                        'trace from a window')
    parser_hfilt.set_defaults(func=hfilt, name='hfilted')
    parser_hfilt.add_argument('start_trace', type=int, help='First trace of representative subset')
    parser_hfilt.add_argument('end_trace', type=int, help='Last trace of representative subset')
    _add_def_args(parser_hfilt)

    parser_ahfilt = subparsers.add_parser('ahfilt', help='Horizontally filter the data adaptively')
    parser_ahfilt.set_defaults(func=ahfilt, name='ahfilt')
    parser_ahfilt.add_argument('win', type=int, help='Number of traces to include in the moving average')
    _add_def_args(parser_ahfilt)

    parser_denoise = subparsers.add_parser('denoise', help='Denoising filter for the data image')
    parser_denoise.set_defaults(func=denoise, name='denoise')
    parser_denoise.add_argument('vert_win', type=int, help='Size of filtering window in vertical (number of samples)')
    parser_denoise.add_argument('hor_win', type=int, help='Size of filtering window in horizontal (number of traces)')
    parser_denoise.add_argument('--filt', type=str, choices=['weiner', 'wiener', 'median'], default='weiner',
                                help='Filter type (Wiener or median with specified dimensions)')
    _add_def_args(parser_denoise)

    parser_vbp = subparsers.add_parser('vbp', help='Vertically bandpass the data')
    parser_vbp.set_defaults(func=vbp, name='bandpassed')
    parser_vbp.add_argument('low_MHz', type=float, help='Lowest frequency passed (in MHz)')
    parser_vbp.add_argument('high_MHz', type=float, help='Highest frequency passed (in MHz)')
    _add_def_args(parser_vbp)

    parser_hbp = subparsers.add_parser('hbp', help='Horizontally bandpass the data')
    parser_hbp.set_defaults(func=hbp, name='hbp')
    parser_hbp.add_argument('low', type=float, help='Lowest frequency passed (in wavelength)')
    parser_hbp.add_argument('high', type=float, help='Highest frequency passed (in wavelength)')
    _add_def_args(parser_hbp)

    parser_lp = subparsers.add_parser('lp', help='Horizontally lowpass the data')
    parser_lp.set_defaults(func=lp, name='lp')
    parser_lp.add_argument('low', type=float, help='Lowest frequency passed (in wavelength)')
    _add_def_args(parser_lp)

    parser_crop = subparsers.add_parser('crop', help='Crop the data in the vertical')
    parser_crop.set_defaults(func=crop, name='cropped')
    parser_crop.add_argument('top_or_bottom', choices=['top', 'bottom'], help='Remove from the top or bottom')
    parser_crop.add_argument('dimension', choices=['snum', 'twtt', 'depth', 'pretrig'],
                             help='Set the bound in terms of snum (sample number), twtt (two way travel time in '
                                  'microseconds), depth (m, from nmo_depth or a light speed of 1.69e8 m/s) or pretrig '
                                  '(the recorded trigger sample)')
    parser_crop.add_argument('lim', type=float, help='The cutoff value')
    _add_def_args(parser_crop)

    parser_nmo = subparsers.add_parser('nmo', help='Normal move-out correction')
    parser_nmo.set_defaults(func=nmo, name='nmo')
    parser_nmo.add_argument('ant_sep', type=float, help='Antenna separation')
    parser_nmo.add_argument('--uice', type=float, default=1.69e8, help='Speed of light in ice in m/s (default 1.69e8)')
    parser_nmo.add_argument('--uair', type=float, default=3.0e8, help='Speed of light in air in m/s (default 3.0e8)')
    parser_nmo.add_argument('--const_firn_offset', type=float, default=None,
                            help='A constant value added to depth to account for firn. Default None (0.0).')
    parser_nmo.add_argument('--rho_profile', type=str, default=None,
                            help='Filename for a depth density profile to correct wave velocity.')
    _add_def_args(parser_nmo)

    parser_elev = subparsers.add_parser('elev', help='Elevation correct')
    parser_elev.set_defaults(func=elev, name='elev')
    _add_def_args(parser_elev)

    parser_rev = subparsers.add_parser('rev', help='Reverse the data')
    parser_rev.set_defaults(func=rev, name='rev')
    _add_def_args(parser_rev)

    parser_hcrop = subparsers.add_parser('hcrop', help='Crop the data in the horizontal')
    parser_hcrop.set_defaults(func=hcrop, name='hcropped')
    parser_hcrop.add_argument('left_or_right', choices=['left', 'right'], help='Remove from the left or right')
    parser_hcrop.add_argument('dimension', choices=['tnum', 'dist'],
                              help='Set the bound in terms of tnum (trace number, 1 indexed) or dist (distance in km)')
    parser_hcrop.add_argument('lim', type=float, help='The cutoff value')
    _add_def_args(parser_hcrop)

    parser_restack = subparsers.add_parser('restack', help='Restack to interval')
    parser_restack.set_defaults(func=restack, name='restacked')
    parser_restack.add_argument('traces', type=int, help='Number of traces to stack. Must be an odd number')
    _add_def_args(parser_restack)

    parser_rgain = subparsers.add_parser('rgain', help='Add a range gain')
    parser_rgain.set_defaults(func=rgain, name='rgain')
    parser_rgain.add_argument('-slope', type=float, default=0.1, help='Slope of linear range gain. Default 0.1')
    _add_def_args(parser_rgain)

    parser_agc = subparsers.add_parser('agc', help='Add an automatic gain')
    parser_agc.set_defaults(func=agc, name='agc')
    parser_agc.add_argument('-window', type=int, default=50, help='Number of samples to average')
    _add_def_args(parser_agc)

    parser_autopick = subparsers.add_parser('autopick', help='(extension) Pick layers from seed points, as the last '
                                                             'step of a chain')
    parser_autopick.set_defaults(func=autopick, name='picked')
    parser_autopick.add_argument('--snums', type=int, nargs='+', required=True,
                                 help='Sample number of every seed (0 indexed)')
    parser_autopick.add_argument('--tnums', type=int, nargs='+', required=True,
                                 help='Trace number of every seed (0 indexed), as many as --snums')
    parser_autopick.add_argument('--freq', type=float, default=None,
                                 help='Pick frequency in MHz (default: that of the file\'s picks, else 4)')
    parser_autopick.add_argument('--pol', type=int, default=None, choices=[1, -1],
                                 help='Polarity of the centre peak (default: that of the file\'s picks, else 1)')
    parser_autopick.add_argument('--picknums', type=int, nargs='+', default=None,
                                 help='Numbers of the new picks (default: continue after the largest present)')
    _add_def_args(parser_autopick)

    parser_vscan = subparsers.add_parser('vscan', help='(extension) Stolt velocity scan: focus of the migrated image '
                                                       'at NV velocities from VMIN to VMAX')
    parser_vscan.set_defaults(func=vscan, name='vscan')
    parser_vscan.add_argument('vmin', type=float, help='Lowest velocity of the scan (m/s)')
    parser_vscan.add_argument('vmax', type=float, help='Highest velocity of the scan (m/s)')
    parser_vscan.add_argument('nv', type=int, help='Number of velocities, evenly spaced from vmin to vmax')
    parser_vscan.add_argument('--htaper', type=int, default=100, help='Number of samples for horizontal taper')
    parser_vscan.add_argument('--vtaper', type=int, default=1000, help='Number of samples for vertical taper')
    parser_vscan.add_argument('--traces', type=int, nargs=2, default=None, metavar=('T0', 'T1'),
                              help='Measure the focus over traces T0 <= j < T1 (default: all)')
    parser_vscan.add_argument('--samples', type=int, nargs=2, default=None, metavar=('S0', 'S1'),
                              help='Measure the focus over samples S0 <= k < S1 (default: all)')
    parser_vscan.add_argument('--gates', type=int, default=None,
                              help='Split the sample range into this many depth gates, one best velocity each')
    parser_vscan.add_argument('--migrate', action='store_true',
                              help='Then migrate (stolt) at the best velocity and save <name>_migrated.mat')
    _add_def_args(parser_vscan)

    parser_fk = subparsers.add_parser('fk', help='(extension) f-k fan (dip) filter: keep or remove the events whose '
                                                 'apparent velocity lies between --va_lo and --va_hi')
    parser_fk.set_defaults(func=fk, name='fk')
    parser_fk.add_argument('--va_lo', type=float, default=None, help='Lowest apparent velocity of the fan (m/s along the profile)')
    parser_fk.add_argument('--va_hi', type=float, default=None, help='Highest apparent velocity of the fan (m/s along the profile)')
    parser_fk.add_argument('--taper', type=float, default=0.1,
                           help='Relative half-width of the cosine taper in slowness around either edge, in [0, 1) (default 0.1)')
    parser_fk.add_argument('--mode', type=str, default='pass', choices=['pass', 'reject'], help='Keep the fan or remove it')
    parser_fk.add_argument('--dip', type=str, default='both', choices=['both', 'down_right', 'down_left'],
                           help='Filter events that dip either way, or only those whose arrival time grows (down_right) or '
                                'shrinks (down_left) with distance')
    _add_def_args(parser_fk)

    parser_decon = subparsers.add_parser('decon', help='(extension) predictive (gapped) deconvolution of every trace: '
                                                       'shortens the wavelet, removes ringing and short-period multiples')
    parser_decon.set_defaults(func=decon, name='decon')
    parser_decon.add_argument('--oplen', type=int, required=True, help='Length of the prediction operator in samples (1 .. 256)')
    parser_decon.add_argument('--gap', type=int, default=1, help='Prediction distance in samples (default 1: spiking deconvolution)')
    parser_decon.add_argument('--prewhiten', type=float, default=0.1, help='Per cent of the zero lag added to it (default 0.1)')
    parser_decon.add_argument('--window', type=int, nargs=2, default=None, metavar=('S0', 'S1'),
                              help='Samples [S0, S1) the operator is designed on (default: the whole trace)')
    parser_decon.add_argument('--design', type=str, default='each', choices=['each', 'mean'],
                              help='An operator per trace, or one from the autocorrelations summed over the traces')
    _add_def_args(parser_decon)

    parser_attr = subparsers.add_parser('attr', help='(extension) complex-trace attribute of every trace: envelope '
                                                     '(reflection strength), instantaneous phase or frequency')
    parser_attr.set_defaults(func=attr, name='attr')
    parser_attr.add_argument('--kind', type=str, required=True, choices=sorted(ATTR_NAMES), help='The attribute that replaces the data')
    parser_attr.add_argument('--smooth', type=int, default=1,
                             help='Frequency only: mean over so many samples (odd, 1 .. 255) weighted by the squared envelope (default 1: none)')
    _add_def_args(parser_attr)

    parser_dipsm = subparsers.add_parser('dipsmooth', help='(extension) mean over 2 HALF + 1 traces along the local slope of the layers')
    parser_dipsm.set_defaults(func=dipsmooth, name='dipsm')
    parser_dipsm.add_argument('half', type=int, help='Traces on either side of the sample (1 .. 32)')
    parser_dipsm.add_argument('--sigma', type=float, nargs=2, default=[2.0, 8.0], metavar=('SZ', 'SX'),
                              help='Gaussian neighbourhood of the slope estimate in samples and in traces (default 2 8)')
    parser_dipsm.add_argument('--max_slope', type=float, default=4.0, help='Largest slope followed, in samples per trace (default 4)')
    _add_def_args(parser_dipsm)

    parser_slope = subparsers.add_parser('slope', help='(extension) replace the data by the local slope of the layers, their dip '
                                                       'or the coherence of the estimate')
    parser_slope.set_defaults(func=slope, name='slope')
    parser_slope.add_argument('--kind', type=str, required=True, choices=sorted(SLOPE_NAMES), help='The field that replaces the data')
    parser_slope.add_argument('--sigma', type=float, nargs=2, default=[2.0, 8.0], metavar=('SZ', 'SX'),
                              help='Gaussian neighbourhood in samples and in traces (default 2 8)')
    parser_slope.add_argument('--max_slope', type=float, default=4.0, help='Clamp of the slope, in samples per trace (default 4)')
    _add_def_args(parser_slope)

    parser_interp = subparsers.add_parser('interp', help='Reinterpolate GPS')
    parser_interp.set_defaults(func=interp, name='interp')
    parser_interp.add_argument('spacing', type=float, help='New spacing of radar traces, in meters')
    parser_interp.add_argument('--gps_fn', type=str, default=None,
                               help='File with precision GPS (not accepted here: run `impproc geolocate` first; '
                                    'only the default, the GPS already in the file, is accepted)')
    parser_interp.add_argument('--offset', type=float, default=0.0, help='Offset from GPS time to radar time')
    parser_interp.add_argument('--minmove', type=float, default=1.0e-2, help='Minimum movement to not be stationary')
    parser_interp.add_argument('--extrapolate', action='store_true', help='Extrapolate GPS data beyond bounds')
    _add_def_args(parser_interp)

    parser_geolocate = subparsers.add_parser('geolocate', help='GPS control')
    parser_geolocate.set_defaults(func=geolocate, name='geolocate')
    parser_geolocate.add_argument('gps_fn', type=str,
                                  help='CSV or mat file containing the GPS information. .csv and .txt files are '
                                       'assumed to be csv, .mat are mat.')
    parser_geolocate.add_argument('--extrapolate', action='store_true', help='Extrapolate GPS data beyond bounds')
    parser_geolocate.add_argument('--guess', action='store_true', help='Guess at offset')
    _add_def_args(parser_geolocate)
    return parser


def _add_def_args(parser):
    parser.add_argument('fns', type=str, nargs='+', help='The files to process')
    parser.add_argument('-o', type=str, help='Output to this file (folder if multiple inputs)')
    parser.add_argument('--ftype', type=str, default='mat', help='Type of file to load (default ImpDAR mat)',
                        choices=FILETYPE_OPTIONS)


def main():
    parser = _get_args()
    args = parser.parse_args(sys.argv[1:])
    if not hasattr(args, 'func'):
        parser.parse_args(['-h'])

    if args.name == 'attr':
        args.name = ATTR_NAMES[args.kind]
    if args.name == 'slope':
        args.name = SLOPE_NAMES[args.kind]
    radar_data = load(args.ftype, args.fns)
    if args.name == 'vscan':
        # (its result is a table of focus values, not a radargram: it names and writes its own files)
        for dat, fn in zip(radar_data, args.fns):
            vscan(dat, fn=fn, nfiles=len(radar_data), **vars(args))
        return
    if args.name in ('interp', 'geolocate'):
        args.func(radar_data, **vars(args))
    else:
        for dat in radar_data:
            args.func(dat, **vars(args))

    if args.o is not None:
        if (len(radar_data) > 1) or (args.o[-1] == '/'):
            for d, f in zip(radar_data, args.fns):
                bn = os.path.split(os.path.splitext(f)[0])[1]
                if bn[-4:] == '_raw':
                    bn = bn[:-4]
                d.save(os.path.join(args.o, bn + '_{:s}.mat'.format(args.name)))
        else:
            radar_data[0].save(args.o)
    else:
        for d, f in zip(radar_data, args.fns):
            bn = os.path.splitext(f)[0]
            if bn[-4:] == '_raw':
                bn = bn[:-4]
            d.save(bn + '_{:s}.mat'.format(args.name))


def mig(dat, mtype='stolt', vel=1.69e8, vtaper=100, htaper=100, tmig=0, verbose=0, vel_fn=None, nxpad=1,
        nearfield=False, gpus=0, **kwargs):
    """Migrate data (defaults as the reference's ``impproc.mig``)."""
    if gpus and gpus > 1:
        os.environ['IMPDAR_NGPUS'] = str(gpus)
    dat.migrate(mtype, vel=vel, vtaper=vtaper, htaper=htaper, tmig=tmig, verbose=verbose, vel_fn=vel_fn,
                nxpad=nxpad, nearfield=nearfield)


def hfilt(dat, start_trace=0, end_trace=-1, **kwargs):
    """Subtract the average trace of a range of traces."""
    dat.hfilt(ftype='hfilt', bounds=(start_trace, end_trace))


def ahfilt(dat, window_size=1000, **kwargs):
    """Adaptive horizontal filter.  The parsed ``win`` lands in ``kwargs``, as in the reference."""
    dat.hfilt(ftype='adaptive', window_size=window_size)


def denoise(dat, vert_win=1, hor_win=10, noise=None, filt='wiener', **kwargs):
    """Despeckle.  The reference's CLI spelling 'weiner' (its default) runs the Wiener filter."""
    dat.denoise(vert_win=vert_win, hor_win=hor_win, noise=noise, ftype='wiener' if filt == 'weiner' else filt)


def vbp(dat, low_MHz=1, high_MHz=10000, **kwargs):
    """Vertically bandpass the data."""
    dat.vertical_band_pass(low_MHz, high_MHz)


def hbp(dat, low=1, high=10, **kwargs):
    """Horizontally band pass the data."""
    dat.horizontal_band_pass(low, high)


def lp(dat, low=1, **kwargs):
    """Low pass filter the data."""
    dat.lowpass(low)


def crop(dat, lim=0, top_or_bottom='top', dimension='snum', **kwargs):
    """Crop in the vertical."""
    dat.crop(lim, top_or_bottom=top_or_bottom, dimension=dimension)


def nmo(dat, ant_sep=0.0, uice=1.69e8, uair=3.0e8, rho_profile=None, **kwargs):
    """Normal move-out correction.  The parsed ``const_firn_offset`` lands in ``kwargs``, as in the reference."""
    dat.nmo(ant_sep, uice=uice, uair=uair, rho_profile=rho_profile)


def elev(dat, **kwargs):
    """Move the data to start at the surface elevation (do last)."""
    dat.elev_correct()


def rev(dat, **kwargs):
    """Flip the data horizontally."""
    dat.reverse()


def hcrop(dat, lim=0, left_or_right='left', dimension='tnum', **kwargs):
    """Crop in the horizontal."""
    dat.hcrop(lim, left_or_right=left_or_right, dimension=dimension)


def restack(dat, traces=1, **kwargs):
    """Restack to reduce size and noise."""
    dat.restack(traces)


def rgain(dat, slope=0.1, **kwargs):
    """Range gain."""
    dat.rangegain(slope)


def agc(dat, window=50, scale_factor=50, **kwargs):
    """Automatic gain control.  ``scale_factor`` is forwarded as ``scaling_factor``, as in the reference."""
    dat.agc(window=window, scaling_factor=scale_factor)


def autopick(dat, snums=(), tnums=(), picknums=None, freq=None, pol=None, **kwargs):
    """(extension) Pick one layer per seed on the device and keep the picks for ``save``."""
    dat.pick_layers(snums, tnums, picknums=picknums, freq=freq, pol=pol)


def fk(dat, va_lo=None, va_hi=None, taper=0.1, mode='pass', dip='both', **kwargs):
    """(extension) f-k fan filter."""
    dat.fk_filter(va_lo=va_lo, va_hi=va_hi, taper=taper, mode=mode, dip=dip)


def decon(dat, oplen=None, gap=1, prewhiten=0.1, window=None, design='each', **kwargs):
    """(extension) predictive deconvolution."""
    dat.predictive_decon(oplen, gap=gap, prewhiten=prewhiten, window=None if window is None else tuple(window), design=design)


def attr(dat, kind=None, smooth=1, **kwargs):
    """(extension) complex-trace attribute."""
    if kind == 'frequency':
        dat.instantaneous_frequency(smooth=smooth)
    elif smooth != 1:
        raise ValueError('--smooth goes with --kind frequency alone')
    elif kind == 'phase':
        dat.instantaneous_phase()
    else:
        dat.envelope()


def dipsmooth(dat, half=None, sigma=(2.0, 8.0), max_slope=4.0, **kwargs):
    """(extension) mean along the layers."""
    dat.dip_smooth(half, sigma=tuple(sigma), max_slope=max_slope)


def slope(dat, kind=None, sigma=(2.0, 8.0), max_slope=4.0, **kwargs):
    """(extension) the data replaced by a field of the layers' orientation (float64)."""
    field = dat.layer_slope(sigma=tuple(sigma), kind=kind, max_slope=max_slope)
    if getattr(dat, '_dev', None) is not None:
        dat.from_device()
    dat.data = field


def _out_name(fn, o, nfiles, name):
    """``main``'s output naming for one input file."""
    if o is not None and nfiles == 1 and o[-1] != '/':
        return o
    bn = os.path.splitext(fn)[0]
    if o is not None:
        bn = os.path.join(o, os.path.split(bn)[1])
    if bn[-4:] == '_raw':
        bn = bn[:-4]
    return bn + '_{:s}.mat'.format(name)


def vscan(dat, vmin=1.5e8, vmax=1.9e8, nv=9, htaper=100, vtaper=1000, traces=None, samples=None, gates=None,
          migrate=False, fn='vscan_raw.mat', o=None, nfiles=1, **kwargs):
    """(extension) Stolt velocity scan: one line per velocity, the best one, ``<name>_vscan.mat`` with the velocities,
    the three sums per row, the varimax and the best velocity; ``migrate``: then the ordinary Stolt migration at it."""
    import numpy as np
    from scipy.io import savemat
    vels = np.linspace(vmin, vmax, nv)
    scan = dat.velocity_scan(vels, htaper=htaper, vtaper=vtaper, traces=traces)
    focus = scan.varimax(samples=samples)
    best_i, best_vel = scan.best(samples=samples)
    for v, f in zip(vels, focus):
        print('vel %.6e m/s  varimax %.6g' % (v, f))
    print('best velocity %.6e m/s (index %d)' % (best_vel, best_i))
    out = {'vels': vels, 'l1': scan.l1, 'l2': scan.l2, 'l4': scan.l4, 'varimax': focus, 'best_vel': best_vel,
           'traces': np.array(scan.traces)}
    if gates is not None:
        out['varimax_gates'] = scan.varimax(samples=samples, gates=gates)
        out['best_vel_gates'] = scan.best(samples=samples, gates=gates)[1]
        print('best velocity per gate: ' + ' '.join('%.6e' % v for v in out['best_vel_gates']))
    savemat(_out_name(fn, o, nfiles, 'vscan'), out)
    if migrate:
        dat.migrate('stolt', vel=best_vel, htaper=htaper, vtaper=vtaper)
        # (-o names the scan's file; the image goes beside the input, or into the folder -o names)
        dat.save(_out_name(fn, o if o is not None and (nfiles > 1 or o[-1] == '/') else None, nfiles, 'migrated'))


def interp(dats, spacing, gps_fn=None, offset=0.0, minmove=1.0e-2, extrapolate=False, **kwargs):
    """Move data to constant spacing (the reference's ``gpslib.interp`` without a GPS file: ``impproc geolocate`` attaches
    one)."""
    if gps_fn is not None:
        raise NotImplementedError('impproc interp does not take --gps_fn: run `impproc geolocate` with the file first, '
                                  'then `impproc interp` on its output')
    for dat in dats:
        dat.constant_space(spacing, min_movement=minmove)


def geolocate(dats, gps_fn, extrapolate=False, guess=False, **kwargs):
    """Attach precision GPS."""
    interpdeep(dats, spacing=None, fn=gps_fn, extrapolate=extrapolate, guess_offset=guess)


if __name__ == '__main__':
    main()
