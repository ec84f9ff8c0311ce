"""``RadarData.constant_space``: restack the radargram onto a constant trace spacing (reference
``src/impdar/lib/RadarData/_RadarDataProcessing.py:499-583``).  The stationary-shot bookkeeping and the
per-trace attribute vectors are host NumPy; the (snum, tnum) interpolation runs on the MI355X
(``impdar_trace_lerp``), on the resident copy when the radargram is held in HBM (``to_device``).
``crop``, ``nmo``, ``constant_sample_depth_spacing`` and ``elev_correct`` (``:50-61, 64-236, 238-337, 585-632``)
change the sample axis the same way: bookkeeping here, tables in ``impdar_amd/vaxis.py``, the radargram through
``impdar_row_lerp`` / ``impdar_col_shift`` or a device-to-device copy.  ``reverse``, ``hcrop`` and ``restack``
(``:20-47, 340-453``) change the trace axis (tables in ``impdar_amd/taxis.py``), ``rangegain`` and ``agc``
(``:456-496``) scale the samples (``impdar_amd/gain.py``)."""
import numpy as np

from ... import gain as _gain
from ... import preproc
from ... import taxis
from ... import vaxis
from ..ImpdarError import ImpdarError
from ._resident import data_dtype as _data_dtype, data_shape as _data_shape
from ._resident import replace_data as _replace_data, update_data as _update_data


def picks_struct_holds_picks(struct):
    """True when a loaded ``mat['picks']`` struct has anything in samp1 / samp2 / samp3 (the reference's
    ``Picks.to_struct`` writes a lone 0 for each of them while nothing is picked, Picks.py:344-363)."""
    if struct is None:
        return False
    names = getattr(struct.dtype, 'names', None) or ()
    for key in ('samp1', 'samp2', 'samp3'):
        if key not in names:
            continue
        val = np.asarray(struct[key][0][0])
        if val.size > 1 or (val.size == 1 and val.dtype != object and not (val.flat[0] == 0 or val.flat[0] != val.flat[0])):
            return True
    return False


def constant_space(self, spacing, min_movement=1.0e-2, show_nomove=False):
    """Interpolate data and GPS attributes onto ``spacing`` metres between traces; shots that moved less
    than ``min_movement`` metres are dropped first.  ``show_nomove`` (a plot in the reference) is refused."""
    if show_nomove:
        raise NotImplementedError('show_nomove plotting is not part of the MI355X migration engine')
    # Every file the reference has loaded and saved again carries a `picks` struct (RadarData/__init__.py:239-242,
    # _RadarDataSaving.py:51-52), empty unless somebody picked: only real picks are refused, the empty struct
    # travels on to save() as it is (the reference's constant_space leaves an unpicked Picks object alone too,
    # _RadarDataProcessing.py:555-566).
    if getattr(self, 'picks', None) is not None or picks_struct_holds_picks(getattr(self, '_picks_struct', None)):
        raise NotImplementedError('re-spacing picks is not part of the MI355X migration engine')
    plan = preproc.SpacingPlan(self.dist, spacing, min_movement)
    good_vals, temp_dist, new_dists = plan.good_vals, plan.temp_dist, plan.new_dists

    _replace_data(self, plan.apply_dev, plan.apply_host)
    snum = _data_shape(self)[0]

    for attr in ['lat', 'long', 'x_coord', 'y_coord', 'decday', 'pressure', 'trig']:
        setattr(self, attr, preproc.interp1d_linear(temp_dist, getattr(self, attr)[good_vals], new_dists))
    for attr in ['elev']:
        if getattr(self, attr) is not None:
            setattr(self, attr, preproc.interp1d_linear(temp_dist, getattr(self, attr)[good_vals], new_dists))

    self.snum = snum if self.snum is None else self.snum
    self.tnum = plan.n_new
    self.trace_num = np.arange(self.tnum).astype(int) + 1
    self.dist = new_dists
    self.trace_int = np.hstack((np.array(np.nanmean(np.diff(self.dist))), np.diff(self.dist))) * 1000.
    try:
        self.flags.interp[0] = 1
        self.flags.interp[1] = spacing
    except (IndexError, TypeError):
        self.flags.interp = np.ones((2,))
        self.flags.interp[1] = spacing


# ------------------------------------------------------------------------------------------ the sample axis
def _refuse_picks(self, what):
    """Steps that would have to move picks refuse real ones, as ``constant_space`` does."""
    if getattr(self, 'picks', None) is not None or picks_struct_holds_picks(getattr(self, '_picks_struct', None)):
        raise NotImplementedError('{:s} picks is not part of the MI355X migration engine'.format(what))


def crop(self, lim, top_or_bottom='top', dimension='snum', uice=1.69e8, rezero=True, zero_trig=True):
    """Crop the radargram in the vertical (reference ``:238-337``): take off the top (``lim`` is the first sample
    kept) or the bottom (``lim`` is the first sample dropped), ``lim`` in samples (``snum``), microseconds
    (``twtt``) or metres (``depth``: ``nmo_depth``, or ``uice`` without it), or at the recorded trigger
    (``pretrig``).  A scalar cut keeps the dtype (on the resident path one device-to-device copy of the kept rows);
    a trace-wise pretrigger moves every trace up by its own trigger sample on the MI355X and gives float64 with
    NaN below the shorter traces.  Updates ``travel_time`` (``rezero``), ``trig`` (``zero_trig``), ``nmo_depth``,
    ``snum`` and ``flags.crop`` as the reference does.  A trace-wise pretrigger with a negative entry raises
    ``ValueError`` (the reference fails on it in its per-trace assignment, with a broadcasting error)."""
    ind = vaxis.crop_index(lim, top_or_bottom, dimension, self.travel_time, self.nmo_depth, self.trig, uice)
    if top_or_bottom == 'top':
        _refuse_picks(self, 'cropping')
    snum_old = _data_shape(self)[0]

    if not isinstance(ind, np.ndarray) or (dimension != 'pretrig'):
        lims = [ind, snum_old] if top_or_bottom == 'top' else [0, ind]
        # the data first: if the device step fails, no attribute has moved
        _replace_data(self, lambda dev: vaxis.row_range_dev(dev, lims[0], lims[1]), lambda data: data[lims[0]:lims[1], :])
        if top_or_bottom == 'top':
            self.trig = self.trig - ind
            if zero_trig:
                self.trig = np.zeros_like(self.trig)
        self.travel_time = self.travel_time[lims[0]:lims[1]]
        if rezero:
            self.travel_time = self.travel_time - self.travel_time[0]
        if self.nmo_depth is not None:
            self.nmo_depth = self.nmo_depth[lims[0]:lims[1]]
    else:
        # trace-wise pretrigger: every trace starts at its own trigger sample, the array at the smallest
        mintrig = np.nanmin(ind)
        if mintrig < 0:
            raise ValueError('cannot crop at a negative pretrigger sample')
        lims = [mintrig, snum_old]
        n_out = int(snum_old - mintrig)
        _replace_data(self, lambda dev: vaxis.col_shift_dev(dev, ind, n_out), lambda data: vaxis.col_shift_host(data, ind, n_out))
        self.trig = self.trig - ind
        self.travel_time = self.travel_time[lims[0]:lims[1]]
        if rezero:
            self.travel_time = self.travel_time - self.travel_time[0]
    self.snum = _data_shape(self)[0]

    try:
        self.flags.crop[0] = 1
        self.flags.crop[2] = self.flags.crop[1] + lims[1]
    except (IndexError, TypeError):
        self.flags.crop = np.zeros((3,))
        self.flags.crop[0] = 1
        self.flags.crop[2] = self.flags.crop[1] + lims[1]
    self.flags.crop[1] = self.flags.crop[1] + lims[0]
    print('Vertical samples reduced to subset [{:d}:{:d}] of original'.format(
        int(self.flags.crop[1]), int(self.flags.crop[2])))


def constant_sample_depth_spacing(self):
    """Interpolate the radargram and ``travel_time`` onto equally spaced depths between the first and the last
    ``nmo_depth`` (reference ``:50-61``); the data become float64.  Returns 1 when the depths already are."""
    if self.nmo_depth is None:
        raise AttributeError('Call nmo first...')
    if np.allclose(np.diff(self.nmo_depth), np.ones((self.snum - 1,)) * (self.nmo_depth[1] - self.nmo_depth[0])):
        print('No constant sampling when you already have constant sampling...')
        return 1
    depths = np.linspace(self.nmo_depth[0], self.nmo_depth[-1], len(self.nmo_depth))
    # interp1d of the transposed 2-D array: the slope form whatever the dtype
    tables = vaxis.RowLerpTables(self.nmo_depth, depths, np_interp=False)
    _replace_data(self, lambda dev: vaxis.row_lerp_dev(dev, tables), lambda data: vaxis.row_lerp_host(data, tables))
    self.travel_time = preproc.interp1d_linear(self.nmo_depth, self.travel_time, depths)
    self.nmo_depth = depths


def nmo(self, ant_sep, uice=1.69e8, uair=3.0e8, const_firn_offset=None, rho_profile=None,
        permittivity_model=vaxis.firn_permittivity, const_sample=False):
    """Normal move-out correction (reference ``:64-193``): every sample moves to its vertical two-way travel time
    for antennas ``ant_sep`` metres apart, at ``uice`` or under the density profile in the csv file
    ``rho_profile`` (depth in m, density in kg/m3; ``permittivity_model`` maps density to permittivity, ``uair``
    is the speed of light above).  The traces are interpolated onto a new ``travel_time`` with the old time
    step on the MI355X (float64 out), and ``nmo_depth`` is defined: ``const_sample`` re-spaces it evenly
    afterwards, ``const_firn_offset`` is added to it.  The pretrigger must have been cropped."""
    if np.any(self.trig > 0):
        raise ImpdarError('Crop out the pretrigger before doing the nmo correction.')
    profile = vaxis.load_rho_profile(rho_profile) if rho_profile is not None else None
    nmotime = vaxis.nmo_times(self.travel_time, ant_sep, uice, uair, self.dt, self.snum, profile, permittivity_model)
    travel_time = np.arange(min(self.travel_time), max(nmotime), self.dt * 1e6)
    tables = vaxis.RowLerpTables(nmotime, travel_time, vaxis.np_interp_convention(_data_dtype(self)))
    _replace_data(self, lambda dev: vaxis.row_lerp_dev(dev, tables), lambda data: vaxis.row_lerp_host(data, tables))
    self.travel_time = travel_time
    self.snum = len(self.travel_time)

    if profile is None:
        self.nmo_depth = self.travel_time / 2. * uice * 1.0e-6
    else:
        self.nmo_depth = vaxis.traveltime_to_depth(self.travel_time, self.dt, profile[0], profile[1], c=uair,
                                                   permittivity_model=permittivity_model)
    if const_sample:
        constant_sample_depth_spacing(self)
    if const_firn_offset is not None:
        self.nmo_depth = self.nmo_depth + const_firn_offset
    print('Normal Moveout filter complete.')
    try:
        self.flags.nmo[0] = 1
        self.flags.nmo[1] = ant_sep
    except (IndexError, TypeError):
        self.flags.nmo = np.ones((2, ))
        self.flags.nmo[1] = ant_sep


def elev_correct(self, v_avg=1.69e8):
    """Move every trace down by its surface elevation below the highest point of the profile, in samples of
    ``dt * v_avg / 2`` metres (reference ``:585-632``), on the MI355X: float64 with NaN above and below the moved
    traces.  Needs ``nmo_depth``; sets ``elevation`` and ``flags.elev`` and, as the reference, leaves ``snum``."""
    if self.nmo_depth is None:
        raise ValueError('Run nmo before elev_correct so that we have depth scale')
    _refuse_picks(self, 'elevation-correcting')
    top_inds, max_samp, elevation = vaxis.elev_shifts(self.elev, self.dt, v_avg, self.nmo_depth)
    n_out = _data_shape(self)[0] + max_samp
    _replace_data(self, lambda dev: vaxis.col_shift_dev(dev, -top_inds, n_out),
                  lambda data: vaxis.col_shift_host(data, -top_inds, n_out))
    self.elevation = elevation
    self.flags.elev = 1


# ------------------------------------------------------------------------------------------- the trace axis
def reverse(self):
    """Flip the profile left to right (reference ``:20-47``): the data (``np.fliplr`` on the host, a row-reversal
    kernel on the resident array) and ``x_coord``, ``y_coord``, ``decday``, ``lat``, ``long`` and ``elev``; as in
    the reference ``dist``, ``trig``, ``pressure`` and ``trace_num`` stay.  A second call undoes the first."""
    _refuse_picks(self, 'reversing')
    _update_data(self, taxis.reverse_dev, np.fliplr)
    for attr in taxis.REVERSED_ATTRS:
        if getattr(self, attr) is not None:
            setattr(self, attr, np.flip(getattr(self, attr), 0))
    if self.flags.reverse:
        print('Back to original direction')
        self.flags.reverse = False
    else:
        print('Profile direction reversed')
        self.flags.reverse = True


def hcrop(self, lim, left_or_right='left', dimension='tnum'):
    """Crop the radargram in the horizontal (reference ``:340-402``): take off the left (``lim`` is the first
    trace kept) or the right (``lim`` is the first trace dropped), ``lim`` a 1-indexed trace number (``tnum``;
    negative counts from the end) or a distance (``dist``: the first trace at or past it).  The dtype is kept: a
    slice on the host, one strided device-to-device copy on the resident array.  Subsets every trace-wise
    attribute, re-zeroes ``dist``, renumbers ``trace_num`` and sets ``tnum`` as the reference does."""
    lims = taxis.hcrop_lims(lim, left_or_right, dimension, self.dist, self.tnum)
    _refuse_picks(self, 'cropping')
    # the data first: if the device step fails, no attribute has moved
    _replace_data(self, lambda dev: taxis.col_range_dev(dev, lims[0], lims[1]), lambda data: data[:, lims[0]:lims[1]])
    for attr in taxis.HCROPPED_ATTRS:
        # some of these are optional, and trig may be a float rather than an array
        if isinstance(getattr(self, attr), np.ndarray):
            setattr(self, attr, getattr(self, attr)[lims[0]:lims[1]])
    if self.dist is not None:
        self.dist = self.dist[lims[0]:lims[1]] - self.dist[lims[0]]
    self.trace_num = self.trace_num[lims[0]:lims[1]] - lims[0] + 1
    self.tnum = _data_shape(self)[1]


def restack(self, traces):
    """Average every ``traces`` neighbouring traces into one (reference ``:405-453``); an even count is bumped to
    the next odd one and a remainder at the end is dropped.  The data become float64 whatever they were (a
    resident array is replaced), the means summed in fp64 on the MI355X.  ``dist``, ``pressure``, ``lat``,
    ``long``, ``x_coord``, ``y_coord``, ``elev``, ``decday`` and ``trig`` become block means; ``trace_int`` becomes
    zeros and ``trace_num`` 1..tnum."""
    traces, tnum = taxis.restack_count(traces, self.tnum)
    _refuse_picks(self, 'restacking')
    oned = {attr: taxis.block_means(getattr(self, attr), traces, tnum) if getattr(self, attr) is not None else None
            for attr in taxis.RESTACKED_ATTRS}
    _replace_data(self, lambda dev: taxis.restack_dev(dev, traces), lambda data: taxis.restack_host(data, traces))
    self.tnum = tnum
    self.trace_num = np.arange(self.tnum).astype(int) + 1
    self.trace_int = np.zeros((tnum, ))
    for attr, val in oned.items():
        setattr(self, attr, val)
    self.flags.restack = True


# ------------------------------------------------------------------------------------------------- the gains
def rangegain(self, slope):
    """Multiply every sample after a trace's trigger by ``travel_time * slope`` (reference ``:456-471``), an fp64
    product stored in the data's dtype, on the MI355X.  ``trig`` is a scalar or one value per trace.  Integer
    data raises ``TypeError``, as NumPy does in the reference."""
    _gain.refuse_integers(_data_dtype(self))
    snum, tnum = _data_shape(self)
    gain, start = _gain.rangegain_tables(self.travel_time, self.trig, slope, snum, tnum)
    _update_data(self, lambda dev: _gain.rangegain_dev(dev, gain, start), lambda data: _gain.rangegain_host(data, gain, start))
    self.flags.rgain = True


def agc(self, window=50, scaling_factor=50):
    """Automatic gain control (reference ``:474-496``): every sample row is multiplied by ``scaling_factor`` over
    the largest amplitude of the ``window // 2`` rows above it and the ``window // 2 - 1`` below it (1e-6 where
    that is zero), the scale cast to the data's dtype first.  Both passes run on the MI355X; a NaN makes the rows
    whose window holds it NaN, as in the reference.  ``window`` below 2 raises ``ValueError``."""
    half = _gain.agc_half(window)
    _update_data(self, lambda dev: _gain.agc_dev(dev, half, scaling_factor),
                 lambda data: _gain.agc_host(data, half, scaling_factor))
    self.flags.agc = True
