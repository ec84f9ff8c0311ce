"""The plots of the reference's ``lib/plot.py`` for a radargram -- ``plot_radargram``, ``plot_traces``, ``plot_power``,
``plot_picks`` with ``get_offset`` (``src/impdar/lib/plot.py:102-283, 368-618, 905-917``) and the three spectral plots
``plot_ft``, ``plot_hft`` and ``plot_spectrogram`` (``:286-365, 621-725``) -- with its signatures, defaults, labels,
extents, limits, errors and ``return_plotinfo`` returns.  What reads the whole radargram is computed on the MI355X, on the
resident radargram when there is one: the colour limits and the traces' x-limits (``RadarData.percentiles``), the image
(``window``: only the part that is drawn comes down; ``flattened``: the picked layer made flat) and the spectra
(``vertical_spectrum``, ``horizontal_spectrum``, ``spectrogram``).  The image handed to ``imshow`` is the reference's,
sample for sample.  ``plot`` wraps these kinds for the ``impplot`` executable.  The reference's ApRES plots are not part
of this engine.

matplotlib is imported inside the functions: ``import impdar_amd`` does not pull it in.
"""
import os

import numpy as np

from .load import load
from .RadarData._resident import data_shape

# the colours of picks that are told apart (Paul Tol's, without the greys)
COLORS_NONGRAY = ['#CC6677', '#332288', '#DDCC77', '#117733', '#88CCEE', '#882255', '#44AA99', '#999933', '#AA4499']


def _axes(fig, ax, figsize):
    import matplotlib.pyplot as plt
    if fig is not None:
        if ax is None:
            ax = plt.gca()
    else:
        fig, ax = plt.subplots(figsize=figsize)
    return fig, ax


def plot(fns, tr=None, s=False, ftype='png', dpi=300, xd=False, yd=False, dualy=False, x_range=(0, -1), power=None,
         spectra=None, freq_limit=None, window=None, scaling='spectrum', filetype='mat', pick_colors=None, ft=False,
         hft=False, clims=None, cmap=None, flatten_layer=None, *args, **kwargs):
    """Load every file of ``fns`` and draw one kind of plot of each: the traces ``tr``, the power of pick ``power`` (all
    files on one axis), the vertical spectrum (``ft``), the horizontal spectrum (``hft``), the spectrogram (``spectra``,
    the pair of frequency limits in MHz), the f-k spectrum (keyword ``fk``, an extension), the autocorrelogram (keywords
    ``acorr`` and ``maxlag``, an extension) or, when none of these is asked for, the radargram -- against the distance
    (``xd``), the depth (``yd``) or both time and depth (``dualy``), with picks in ``pick_colors``, colour limits
    ``clims``, colour map ``cmap`` (None: grey) and layer ``flatten_layer`` made flat.  Save next to the input with
    extension ``ftype`` (``s``) or show."""
    import matplotlib.pyplot as plt
    radar_data = load(filetype, fns)
    xdat = 'dist' if xd else 'tnum'
    if yd:
        if dualy:
            raise ValueError('Only one of yd and dualy can be true')
        ydat = 'depth'
    else:
        ydat = 'dual' if dualy else 'twtt'
    if (tr is not None) and (power is not None):
        raise ValueError('Cannot do both tr and power. Pick one')
    if tr is not None:
        figs = [plot_traces(dat, tr, ydat=ydat) for dat in radar_data]
    elif power is not None:
        figs = [plot_power(radar_data, power)]
    elif ft:
        figs = [plot_ft(dat) for dat in radar_data]
    elif hft:
        figs = [plot_hft(dat) for dat in radar_data]
    elif spectra:
        figs = [plot_spectrogram(dat, spectra, window=window, scaling=scaling) for dat in radar_data]
    elif kwargs.get('fk', False):
        figs = [plot_fk(dat) for dat in radar_data]
    elif kwargs.get('acorr', False):
        figs = [plot_acorr(dat, maxlag=kwargs.get('maxlag', None)) for dat in radar_data]
    else:
        figs = [plot_radargram(dat, xdat=xdat, ydat=ydat, x_range=None, pick_colors=pick_colors, clims=clims, cmap=cmap,
                               flatten_layer=flatten_layer) for dat in radar_data]
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


def _picks_of(dat):
    """The picks of ``dat``: its ``Picks`` object, or one built from the struct a file was loaded with (which ``dat``
    keeps as it is until something picks), or None."""
    if dat.picks is None and getattr(dat, '_picks_struct', None) is not None:
        from .Picks import Picks
        return Picks(dat, dat._picks_struct)
    return dat.picks


def _depth_axis(dat):
    """The depth of every sample: the NMO depth where there is one, else the travel time at 1.69e8 m/s."""
    if dat.nmo_depth is not None:
        return dat.nmo_depth
    return dat.travel_time / 2.0 * (1.69e8 * 1.0e-6)


def _first_valid_time(dat):
    """The first sample whose travel time is no NaN (a normal-moveout correction may leave NaNs at the top)."""
    return np.min(np.where(~np.isnan(dat.travel_time))[0])


def _host_clims(dat, data_name, y_range, x_range):
    """The (10, 90) percentiles on the host, for an attribute other than ``data`` or for complex data (in dB): of the
    attribute's window where ``data`` is no NaN, as the reference takes them."""
    shown = np.asarray(getattr(dat, data_name))[y_range[0]:y_range[-1], x_range[0]:x_range[-1]]
    data = dat.window(y_range, x_range)
    if np.iscomplexobj(data):
        shown = 10.0 * np.log10(np.absolute(shown))
    return np.percentile(shown[~np.isnan(data)], (10, 90))


def plot_radargram(dat, xdat='tnum', ydat='twtt', x_range=(0, -1), y_range=(0, -1), cmap=None, fig=None, ax=None,
                   return_plotinfo=False, pick_colors=None, clims=None, data_name='data', flatten_layer=None,
                   middle_picks_only=False):
    """Draw the radargram: traces ``x_range`` and samples ``y_range`` (``(0, -1)``: all) against the trace number or
    the distance (``xdat``: tnum | dist) and the travel time, the depth, both, or the elevation (``ydat``: twtt | depth |
    dual | elev), in ``cmap`` (None: grey) between ``clims`` -- by default the 10th and 90th percentile of the window's
    values that are no NaN, taken on the device.  ``flatten_layer``: shift every trace so that this pick lies flat;
    ``pick_colors``: draw the picks (``plot_picks``; ``middle_picks_only`` as its ``just_middle``); ``data_name``: take
    the colour limits from another attribute.  Returns ``(fig, ax)``, or with ``return_plotinfo`` ``(im, xd, yd, x_range,
    clims)`` with the ranges as they were resolved."""
    import matplotlib.pyplot as plt
    getattr(dat, data_name)                 # (it must exist)
    if xdat not in ['tnum', 'dist']:
        raise ValueError('x axis choices are tnum or dist')
    elif (xdat == 'dist') and dat.dist is None:
        raise ValueError('xdat cannot be dist when the data has no dist')
    if cmap is None:
        cmap = plt.cm.gray
    if x_range is None:
        x_range = (0, -1)
    if x_range[-1] == -1:
        x_range = (x_range[0], dat.tnum)
    if y_range is None:
        y_range = (0, -1)
    if y_range[-1] == -1:
        y_range = (y_range[0], data_shape(dat)[0])
    on_host = getattr(dat, '_dev', None) is None
    is_complex = on_host and np.iscomplexobj(dat.data)

    if clims is None:
        if data_name != 'data' or is_complex:
            clims = _host_clims(dat, data_name, y_range, x_range)
        else:
            clims = dat.percentiles((10, 90), y_range=y_range, x_range=x_range, skip_nan=True)

    fig, ax = _axes(fig, ax, (12, 8))
    if ydat == 'elev':
        if hasattr(dat.flags, 'elev') and dat.flags.elev:
            yd = dat.elevation
            ax.set_ylabel('Elevation (m)')
        else:
            raise ValueError('Elevation plot requested but we have none')
    else:
        ax.invert_yaxis()
        if ydat == 'twtt':
            y_range = (max(y_range[0], _first_valid_time(dat)), y_range[1])
            yd = dat.travel_time
            ax.set_ylabel('Two way travel time (usec)')
        elif ydat == 'depth':
            yd = _depth_axis(dat)
            ax.set_ylabel('Depth (m)')
        elif ydat == 'dual':
            y_range = (max(y_range[0], _first_valid_time(dat)), y_range[1])
            yd = dat.travel_time
            ax.set_ylabel('Two way travel time (usec)')
            ax2 = ax.twinx()
            yd2 = _depth_axis(dat)
            ax2.set_ylabel('Approximate depth (m)')
            ax2.set_ylim(yd2[y_range[-1] - 1], yd2[y_range[0]])
        else:
            raise ValueError('Unrecognized ydat, choices are elev, twtt, \
                             depth, or dual')

    if xdat == 'tnum':
        xd = np.arange(int(dat.tnum))
        ax.set_xlabel('Trace number')
    else:
        xd = dat.dist
        ax.set_xlabel('Distance (km)')

    xs, ys = xd[x_range[0]:x_range[-1]], yd[y_range[0]:y_range[-1]]
    if flatten_layer is not None:
        # (every sample of the shifted traces, whatever y_range: the reference's image)
        image = dat.flattened(flatten_layer, x_range)
        extent = [np.min(xs), np.max(xs), np.max(ys), np.min(ys)]
    else:
        image = dat.window(y_range, x_range)
        if hasattr(dat.flags, 'elev') and dat.flags.elev:
            extent = [np.min(xs), np.max(xs), np.min(ys), np.max(ys)]
        else:
            extent = [np.min(xs), np.max(xs), np.max(ys), np.min(ys)]
    if np.iscomplexobj(image):
        image = 10.0 * np.log10(np.absolute(image))
    im = ax.imshow(image, cmap=cmap, vmin=clims[0], vmax=clims[1], extent=extent, aspect='auto')

    if (pick_colors is not None) and pick_colors:
        plot_picks(dat, xd, yd, fig=fig, ax=ax, colors=pick_colors, flatten_layer=flatten_layer, just_middle=middle_picks_only,
                   x_range=x_range)
    if not return_plotinfo:
        return fig, ax
    return im, xd, yd, x_range, clims


def plot_traces(dat, tr, ydat='twtt', fig=None, ax=None, linewidth=1.0, linestyle='solid'):
    """Draw trace ``tr``, or traces ``tr[0]`` to ``tr[1]``, as amplitude against the travel time, the depth or both
    (``ydat``: twtt | depth | dual).  The amplitude axis runs between the 1st and 99th percentile of these traces, taken
    on the device, symmetric about zero where they straddle it; only these traces come down."""
    if hasattr(tr, '__iter__'):
        if not len(tr) == 2:
            raise ValueError('tr must either be a 2-tuple of bounds for the \
                             traces or a single trace index')
    if type(tr) == int:
        tr = (tr, tr + 1)
    elif tr[0] == tr[1]:
        tr = (tr[0], tr[0] + 1)
    if ydat not in ['twtt', 'depth', 'dual']:
        raise ValueError('y axis choices are twtt or depth')
    fig, ax = _axes(fig, ax, (8, 12))
    lims = dat.percentiles((1, 99), x_range=(tr[0], tr[1]), skip_nan=False)
    if lims[0] == lims[1]:
        lims[1] = lims[0] + 1.
    ax.invert_yaxis()
    if ydat == 'depth':
        yd = dat.nmo_depth if dat.nmo_depth is not None else dat.travel_time / 2.0 * 1.69e8 * 1.0e-6
        ax.set_ylabel('Depth (m)')
    else:
        yd = dat.travel_time
        ax.set_ylabel('Two way travel time (usec)')
        if ydat == 'dual':
            ax2 = ax.twinx()
            yd2 = _depth_axis(dat)
            ax2.set_ylabel('Approximate depth (m)')
            ax2.set_ylim(yd2[-1], yd2[0])
    traces = dat.window((0, -1), (tr[0], tr[1]))
    for j in range(traces.shape[1]):
        ax.plot(traces[:, j], yd, linewidth=linewidth, linestyle=linestyle)
    if lims[0] < 0 and lims[1] > 0:
        ax.set_xlim(lims[0], -lims[0])
    else:
        ax.set_xlim(*lims)
    ax.set_xlabel('Amplitude')
    return fig, ax


def plot_power(dats, idx, fig=None, ax=None, clims=None):
    """Scatter the power returned from pick ``idx`` (a pick number) of one radargram or of a list of them on one axis,
    in dB, at the projected coordinates where the first one has them, else at longitude and latitude.  ``clims``: the
    colour limits, by default the 1st and 99th percentile, spread by 1 % when they coincide."""
    try:
        idx = int(idx)
    except TypeError:
        raise TypeError('Please enter an integer pick number')
    if type(dats) not in [list, tuple]:
        dats = [dats]
    picks = [_picks_of(dat) for dat in dats]
    for pk in picks:
        if (pk is None) or (pk.picknums is None):
            raise ValueError('There are no picks on this radardata, \
                             cannot plot return power')
        if idx not in pk.picknums:
            raise ValueError('Pick number {:d} not found in your file'.format(idx))
    fig, ax = _axes(fig, ax, (8, 12))
    if (dats[0].x_coord is not None) and (dats[0].y_coord is not None):
        lons, lats = [dat.x_coord for dat in dats], [dat.y_coord for dat in dats]
    else:
        lons, lats = [dat.long for dat in dats], [dat.lat for dat in dats]
    lons = np.hstack(lons) if len(dats) > 1 else lons[0]
    lats = np.hstack(lats) if len(dats) > 1 else lats[0]
    pick_power = np.hstack([pk.power[list(pk.picknums).index(idx)].flatten() for pk in picks])
    c = 10 * np.log10(pick_power)
    if clims is None:
        clims = np.percentile(c[~np.isnan(c)], (1, 99))
        # (equal limits would not draw; a pick of constant power still should)
        if (clims[0] - clims[1]) / clims[0] < 1.0e-8:
            clims[0] = 0.99 * clims[0]
            clims[1] = 1.01 * clims[1]
    img = ax.scatter(lons.flatten(), lats.flatten(), c=c.flatten(), vmin=clims[0], vmax=clims[1])
    h = fig.colorbar(img)
    h.set_label('dB')
    ax.set_ylabel('Northing')
    ax.set_xlabel('Easting')
    return fig, ax


def _pick_colors(colors, npicks_stored, picknums, just_middle):
    """``(cl, per_pick)``: the (top, middle, bottom) colours of every pick, or -- ``per_pick`` -- one entry per pick in
    ``colors`` that is resolved pick by pick."""
    if not colors:
        return 'mgm', None
    if type(colors) == str:
        return (colors if len(colors) == 3 else ('none', colors, 'none')), None
    if (type(colors) == bool) and colors:
        return None, (COLORS_NONGRAY * (npicks_stored // len(COLORS_NONGRAY) + 1))[:len(picknums)]
    if not len(colors) == len(picknums):
        if (len(colors) == 3) and not just_middle:
            return colors, None
        raise ValueError('If not a string, must have length 3 or length npicks')
    return None, colors


def plot_picks(rd, xd, yd, colors=None, flatten_layer=None, fig=None, ax=None, just_middle=False, picknums=None,
               x_range=None, **plotting_kwargs):
    """Draw the top, middle and bottom of the picks ``picknums`` (default: all) of ``rd`` over axes whose coordinates
    are ``xd`` and ``yd``, shifted as ``flatten_layer`` shifts the image.  ``colors``: nothing ('mgm': magenta, green,
    magenta), a string of three colour letters (top, middle, bottom), another colour string (the middle alone), True
    (a colour per pick), or one entry per pick -- each a colour or, unless ``just_middle``, a triple."""
    import matplotlib.pyplot as plt
    from matplotlib.colors import is_color_like
    if x_range is None:
        x_range = (0, -1)
    if x_range[-1] == -1:
        x_range = (x_range[0], rd.tnum)
    if ax is None:
        if fig is not None:
            ax = plt.gca()
        else:
            fig, ax = plt.subplots()
    picks = _picks_of(rd)
    if picks is None or picks.samp1 is None:
        return fig, ax
    offset, mask = get_offset(rd, flatten_layer)
    if picknums is None:
        if picks.picknums is None:
            return fig, ax
        picknums = picks.picknums
    cl, per_pick = _pick_colors(colors, picks.samp1.shape[0], picknums, just_middle)
    xs = xd[x_range[0]:x_range[1]]
    for j, pn in enumerate(picknums):
        i = list(picks.picknums).index(pn)      # (j counts the colours, i the stored picks)
        if per_pick is not None:
            if hasattr(per_pick[j], '__len__') and len(per_pick[j]) == 3 and not just_middle:
                cl = per_pick[j]
            elif is_color_like(per_pick[j]):
                cl = ('none', per_pick[j], 'none')
            else:
                raise ValueError('Color ', per_pick[j], ' not defined')
        for rows, color in ((picks.samp2[i, :], cl[1]), (picks.samp1[i, :], cl[0]), (picks.samp3[i, :], cl[2])):
            line = np.full(xd.shape, np.nan)
            keep = ~np.logical_or(mask, np.isnan(rows))
            line[keep] = yd[(rows + offset)[keep].astype(int)]
            ax.plot(xs, line[x_range[0]:x_range[1]], color=color, **plotting_kwargs)
    return fig, ax


def get_offset(dat, flatten_layer=None):
    """``(offset, mask)`` per trace: by how many rows a trace moves so that pick ``flatten_layer`` lies on the row
    ``int(nanmean(its samp2))``, and where the pick misses the trace (the offset is NaN there).  Zeros and no mask
    without a layer."""
    tnum = data_shape(dat)[1]
    if flatten_layer is None:
        return np.zeros((tnum,)), np.zeros((dat.tnum,), dtype=bool)
    picks = _picks_of(dat)
    if flatten_layer not in picks.picknums:
        raise ValueError('That layer is not in existence, cannot flatten')
    layer_depth = picks.samp2[list(picks.picknums).index(flatten_layer), :]
    offset = int(np.nanmean(layer_depth)) - layer_depth
    return offset, np.isnan(layer_depth)


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


def plot_fk(dat, fig=None, ax=None):
    """(extension) Image of the f-k power spectrum in dB below its maximum, ``10 log10(P / max P)``: wavenumber in cycles
    per metre against frequency in MHz -- where the fan of ``fk_filter`` is chosen."""
    import matplotlib.pyplot as plt
    freq_mhz, k_per_m, power = dat.fk_spectrum()
    with np.errstate(divide='ignore', invalid='ignore'):
        db = 10.0 * np.log10(power / np.max(power))
    fig, ax = _axes(fig, ax, (10, 7))
    dk = (k_per_m[-1] - k_per_m[0]) / (len(k_per_m) - 1)
    df = (freq_mhz[-1] - freq_mhz[0]) / (len(freq_mhz) - 1)
    im = ax.imshow(db, origin='lower', aspect='auto', interpolation='nearest',
                   extent=[k_per_m[0] - dk / 2.0, k_per_m[-1] + dk / 2.0, freq_mhz[0] - df / 2.0, freq_mhz[-1] + df / 2.0])
    cbar = plt.colorbar(im, shrink=0.9, orientation='vertical', pad=0.03, ax=ax)
    cbar.set_label('Power (dB below the maximum)')
    ax.set_xlabel('Wavenumber (1/m)')
    ax.set_ylabel('Frequency (MHz)')
    ax.set_title('P(k, f)')
    return fig, ax


def plot_acorr(dat, maxlag=None, fig=None, ax=None):
    """(extension) Image of the normalised autocorrelation of every trace, lag time in nanoseconds against trace number
    -- where ``gap`` and ``oplen`` of ``predictive_decon`` are chosen: ringing and multiples are the bands below the zero
    lag.  ``maxlag`` in samples (None: a quarter of the trace, at most 256)."""
    import matplotlib.pyplot as plt
    if maxlag is None:
        maxlag = max(min(int(dat.snum) // 4, 256), 1) if dat.snum > 1 else 0
    lag_s, A = dat.autocorrelation(maxlag)
    fig, ax = _axes(fig, ax, (10, 7))
    dl = float(dat.dt) * 1.0e9
    im = ax.imshow(A, origin='upper', aspect='auto', interpolation='nearest', vmin=-1.0, vmax=1.0, cmap='RdBu_r',
                   extent=[0.5, A.shape[1] + 0.5, lag_s[-1] * 1.0e9 + dl / 2.0, -dl / 2.0])
    cbar = plt.colorbar(im, shrink=0.9, orientation='vertical', pad=0.03, ax=ax)
    cbar.set_label('Autocorrelation / zero lag')
    ax.set_xlabel('Trace number')
    ax.set_ylabel('Lag (ns)')
    ax.set_title('A(lag, tnum)')
    return fig, ax
