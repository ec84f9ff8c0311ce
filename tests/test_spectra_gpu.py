"""Spectra on the MI355X (csrc/spectrum.hip) against the FS* fixtures: the mean spectra along both axes and the periodogram of
every trace, through the host-buffer and the resident entry points, as float32 and as float64.

The bar comes from the reference alone (tests/golden/make_golden_spectra.py).  The expected values
``*_hi`` are the reference's arithmetic evaluated in longdouble on the data widened to float64 -- the float32 and the
float64 case of a fixture hold the same values, so they share them.  Per output the yardstick is
Y = u (log2 n + log2 m + 2) n mean_m ||x||^2 (u = 2^-53, n the transform length, m the spectra averaged, x the row as it
enters the transform; for the periodogram the window-weighted undetrended trace, times 2 scale, m = 1), and a result
passes where |out - hi| <= C Y on every bin with NaNs in the same places.  C = 30 is 8 x the largest distance, in units
of Y, of the reference's own float64 results from ``*_hi`` over all fixtures (3.73, the horizontal spectrum of 16384 x 2).
On the flat fixtures 99 % of the bins lie above 4 C Y (tests/test_spectra_cpu.py), so one wrong bin cannot pass.
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import spectra_ref as sr
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

NAMES = sr.fixture_names(GOLDEN)
FS = 1.0 / sr.DT
POW2, MIXED, ROCFFT = 0, 1, 2
_CACHE = {}


def fixture(name):
    if name not in _CACHE:
        _CACHE.clear()              # (one at a time: the large ones are MBs)
        _CACHE[name] = sr.load_fixture(GOLDEN, name)
    return _CACHE[name]


def held(out, hi, Y, what):
    """|out - hi| <= C Y on every bin (Y a number, or per trace along the last axis), NaNs in the same places."""
    assert out.dtype == np.float64 and out.shape == hi.shape, what
    assert np.array_equal(np.isnan(out), np.isnan(hi)), what
    ok = ~np.isnan(hi)
    with np.errstate(invalid='ignore'):
        ratio = np.abs(out - hi) / Y
    worst = float(np.max(ratio[ok])) if ok.any() else 0.0
    print('%s: max |out - hi| / Y = %.3g (bar %g)' % (what, worst, sr.C))
    assert worst <= sr.C, what


def results(hip, data, resident):
    """{quantity: array} through the host-buffer or the resident entry points."""
    from impdar_amd import spectra
    out = {}
    if resident:
        d = hip.DeviceArray.from_host(hip.context(), data)
        try:
            out['ft'] = spectra.mean_spectrum_dev(d, 0)
            for i, (win, scaling) in enumerate(sr.PARAMS):
                freq, out['pg%d' % i] = spectra.periodogram_dev(d, FS, window=win, scaling=scaling)
            out['hft'] = spectra.mean_spectrum_dev(d, 1)
            assert np.array_equal(d.to_host(), data, equal_nan=True)           # the radargram stays as it was
        finally:
            d.free()
    else:
        out['ft'] = spectra.mean_spectrum_host(data, 0)
        for i, (win, scaling) in enumerate(sr.PARAMS):
            freq, out['pg%d' % i] = spectra.periodogram_host(data, FS, window=win, scaling=scaling)
        out['hft'] = spectra.mean_spectrum_host(data, 1)
    assert np.array_equal(freq, np.fft.rfftfreq(data.shape[0], 1.0 / FS))
    return out


@pytest.mark.parametrize('name', NAMES)
def test_fixture_through_host_and_resident_entries(hip, name):
    g = fixture(name)
    first = None
    for dtype in (np.float32, np.float64):
        data = g['data'].astype(dtype)
        for resident in (False, True):
            out = results(hip, data, resident)
            for q in ('ft', 'hft', 'pg0', 'pg1', 'pg2'):
                held(out[q], g[q + '_hi'], g['Y_' + q], '%s %s %s %s' % (name, q, np.dtype(dtype).name, 'resident' if resident else 'host'))
            # float32 is widened on load: all four runs are the same float64 computation
            if first is None:
                first = out
            for q in out:
                assert np.array_equal(out[q], first[q], equal_nan=True), (name, q, dtype, resident)
    print('%s: the reference on float32 lies up to %.3g Y (ft), %.3g Y (pg1) from hi' %
          (name, g['rho32_ft'] / max(float(np.min(g['Y_ft'])), 1e-300), g['rho32_pg1'] / max(float(np.min(g['Y_pg1'])), 1e-300)))


def test_nan_fixture_is_what_the_reference_makes_of_it(hip):
    g = fixture('FS27_36x7_nan')
    out = results(hip, g['data'], False)
    assert np.all(np.isnan(out['ft'])) and np.all(np.isnan(out['hft']))
    bad = np.isnan(g['data']).any(axis=0)
    assert bad.sum() == 1
    assert np.all(np.isnan(out['pg0'][:, bad])) and not np.any(np.isnan(out['pg0'][:, ~bad]))


@pytest.mark.parametrize('name', ['FS17_1024x65_flat', 'FS11_7x16384_flat'])
def test_two_calls_give_the_same_bits(hip, name):
    data = fixture(name)['data']
    a, b = results(hip, data, True), results(hip, data, True)
    for q in ('ft', 'hft', 'pg0', 'pg1', 'pg2'):
        assert np.array_equal(a[q], b[q]), (name, q)


def test_route_probe_reports_the_kind_of_every_fixture_shape(hip):
    lib = hip.load()
    kinds = {32: POW2, 36: MIXED, 30: ROCFFT, 63: ROCFFT, 22: ROCFFT, 7: ROCFFT, 100: MIXED, 1022: ROCFFT, 1024: POW2, 4096: POW2,
             16384: POW2, 1: ROCFFT, 5: ROCFFT, 9: ROCFFT, 3: ROCFFT, 33: ROCFFT, 4: ROCFFT, 65: ROCFFT, 17: ROCFFT, 2: ROCFFT}
    out = (4 * [0])
    import ctypes as C
    for name in NAMES:
        snum, tnum = fixture(name)['data'].shape
        for n, rows in ((snum, tnum), (tnum, snum)):
            buf = (C.c_int * 4)(*out)
            hip.check(lib.impdar_spec_route_probe(n, rows, buf), 'impdar_spec_route_probe')
            assert buf[0] == kinds[n], (name, n)
            assert buf[1] >= 1 and (buf[1] - 1) * buf[2] < rows <= buf[1] * buf[2] and buf[3] <= 160 * 1024
    assert lib.impdar_spec_route_probe(0, 4, (C.c_int * 4)()) == hip.ERR_ARG


def test_c_entries_refuse_bad_arguments(hip):
    import ctypes as C
    lib, ctx = hip.load(), hip.context()
    data = np.zeros((8, 4), dtype=np.float32)
    out = np.zeros((8,), dtype=np.float64)
    p, o = data.ctypes.data_as(C.c_void_p), hip.as_dp(out)[1]
    assert lib.impdar_mean_spectrum(ctx, p, hip.F32, 8, 4, 2, o) == hip.ERR_ARG
    assert lib.impdar_mean_spectrum(ctx, p, hip.F32, 0, 4, 0, o) == hip.ERR_ARG
    assert lib.impdar_mean_spectrum(ctx, p, 7, 8, 4, 0, o) == hip.ERR_ARG
    assert lib.impdar_periodogram(ctx, p, hip.F32, 8, 4, None, 0.0, o) == hip.ERR_ARG
    assert lib.impdar_periodogram(ctx, p, hip.F32, 8, 4, None, float('nan'), o) == hip.ERR_ARG
    assert lib.impdar_periodogram(ctx, None, hip.F32, 8, 4, None, 1.0, o) == hip.ERR_ARG


def make_dat(data, interp=(1.0, 2.5)):
    from impdar_amd.lib.RadarData import RadarData
    d = RadarData(None)
    d.data = data.copy()
    d.snum, d.tnum = data.shape
    d.dt = sr.DT
    d.trace_num = np.arange(d.tnum) + 1.0
    d.flags.interp = np.array(interp)
    return d


def test_radardata_methods_resident_and_host(hip):
    g = fixture('FS13_100x33_flat')
    data = g['data']
    host, res = make_dat(data), make_dat(data).to_device()
    for method, args in (('vertical_spectrum', ()), ('horizontal_spectrum', ()), ('spectrogram', ()), ('spectrogram', ('hamming', 'density'))):
        a, b = getattr(host, method)(*args), getattr(res, method)(*args)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), method
    assert res._dev is not None and res.data is None           # the radargram stayed on the device
    # the axes, as the reference forms them (plot.py:312, 318; :350-355, 362; :681)
    freq = np.fft.fftfreq(100) / sr.DT
    f, p = host.vertical_spectrum()
    assert np.array_equal(f, freq[freq >= 0] / 1.0e6)
    held(p, g['ft_hi'][freq >= 0], g['Y_ft'], 'vertical_spectrum')
    hfreq = np.fft.fftfreq(33)
    with np.errstate(divide='ignore'):
        wavelength = 2.5 / hfreq
    wavelength[hfreq == 0.0] = np.inf
    w, p = host.horizontal_spectrum()
    assert np.array_equal(w, wavelength[hfreq >= 0]) and w[0] == np.inf
    held(p, g['hft_hi'][hfreq >= 0], g['Y_hft'], 'horizontal_spectrum')
    y, img = host.spectrogram()
    assert np.array_equal(y, np.fft.rfftfreq(100, 1.0 / FS) / 1.0e6)
    held(img, g['pg0_hi'], g['Y_pg0'], 'spectrogram')                      # the default: boxcar, 'spectrum'
    held(host.spectrogram('hamming', 'density')[1], g['pg1_hi'], g['Y_pg1'], 'spectrogram hamming density')
    res.from_device()
    assert np.array_equal(res.data, data)
    ints = make_dat(np.round(data * 100).astype(np.int16))                 # integers are widened by work_array
    held(ints.vertical_spectrum()[1], sr.mean_spectrum(ints.data.astype(np.float64), 0)[freq >= 0],
         sr.yardstick_mean(ints.data, 0), 'int16 data')
    with pytest.raises(TypeError, match='complex'):
        make_dat(data.astype(np.complex64)).spectrogram()


def test_plots_draw_with_the_references_labels(hip, capsys):
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    from impdar_amd.lib import plot
    g = fixture('FS13_100x33_flat')
    dat = make_dat(g['data'])
    fig, ax = plot.plot_ft(dat, color='r')
    assert (ax.get_xlabel(), ax.get_ylabel()) == ('Freq (MHz)', 'Power spectral density')
    x, y = ax.lines[0].get_data()
    assert len(x) == 50 and np.array_equal(y, dat.vertical_spectrum()[1]) and ax.lines[0].get_color() == 'r'
    fig, ax = plot.plot_hft(dat)
    assert (ax.get_xlabel(), ax.get_ylabel()) == ('Wavelength', 'Power spectral density')
    assert len(ax.lines[0].get_xdata()) == 17
    fig, ax = plot.plot_spectrogram(dat, freq_limit=(0.0, 20.0), window='hann')
    assert (ax.get_xlabel(), ax.get_ylabel(), ax.get_title()) == ('Trace Number', 'Frequency (MHz)', 'PSD(tnum, f)')
    assert ax.get_ylim() == (0.0, 20.0) and capsys.readouterr().out == ''
    # the frequencies run to fs / 2 = 50 MHz
    plot.plot_spectrogram(dat, freq_limit=(0.0, 80.0))
    assert capsys.readouterr().out == 'Warning: y-axis limit large compared to the frequencies plotted\n'
    plot.plot_spectrogram(dat, freq_limit=30.0)
    assert capsys.readouterr().out == 'Frequency limit should be a tuple of low, high. Ignoring.\n'
    with pytest.raises(ValueError, match=r'Y-axis limit -1.0 MHz too low\.'):
        plot.plot_spectrogram(dat, freq_limit=(-2.0, -1.0))
    fig2, ax2 = plt.subplots()
    assert plot.plot_ft(dat, fig=fig2, ax=ax2) == (fig2, ax2)
    with pytest.raises(ValueError, match='Unknown scaling'):
        plot.plot_spectrogram(dat, scaling='power')
    plt.close('all')


def test_impplot_ft_saves_a_file_in_a_fresh_process(hip, tmp_path):
    fn = str(tmp_path / 'line.mat')
    shutil.copy(os.path.join(GOLDEN, 'PK_ref_saved_picked.mat'), fn)
    env = dict(os.environ, MPLBACKEND='Agg')
    for args, ext in ((['ft', '-s', fn], 'png'), (['spectrogram', '-s', '--o_fmt', 'pdf', '-window', 'hann', fn, '0', '40'], 'pdf')):
        out = subprocess.run([sys.executable, '-m', 'impdar_amd.bin.impplot'] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:]
        assert os.path.getsize(str(tmp_path / ('line.' + ext))) > 1000
