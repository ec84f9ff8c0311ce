"""The display unit without a GPU: the restated percentile (tests/display_ref.py: a sort, the two ranks, NumPy's
interpolation) and the product's own interpolation (impdar_amd/display.py) against np.percentile bit for bit; the restated
flatten, offsets, colour limits and image against every FD* fixture (what the reference drew); the host-side header
csrc/display_route.h, compiled by itself with g++, with the whole radix select run on the host; argument errors, raised
before any device call; the routing of plot() and of the impplot parsers; and the C declarations."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import display_ref as dr
from conftest import GOLDEN, ROOT

NAMES = dr.fixture_names(GOLDEN)
CSRC = os.path.join(ROOT, 'impdar_amd', 'csrc')
QS = (0, 1, 10, 50, 90, 99, 100, 33.3)
needs_gxx = pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not installed')


def same(a, b):
    """Equal bit for bit up to the sign of a zero, NaNs in the same places."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def value_sets(dtype):
    rng = np.random.default_rng(7)
    tiny = np.finfo(dtype).smallest_subnormal
    sets = [rng.standard_normal(n).astype(dtype) for n in (1, 2, 3, 7, 100, 1000, 1001)]
    sets.append(rng.integers(0, 3, 1001).astype(dtype))                                 # heavy ties
    sets.append(np.array([-np.inf, np.inf, 1.0, -2.0, np.inf, 0.5, -np.inf], dtype=dtype))
    sets.append(np.array([tiny, -tiny, 3 * tiny, 0.0, 5 * tiny, -7 * tiny, 1.0], dtype=dtype))
    sets.append(np.array([0.0, -0.0, 0.0, -0.0, -0.0, 1.0, -1.0], dtype=dtype))          # zeros of both signs
    sets.append((1.0 + rng.random(513) * 2.0 ** -12).astype(dtype))
    return sets


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_restated_percentile_is_numpys(dtype):
    from impdar_amd import display
    for x in value_sets(dtype):
        with np.errstate(invalid='ignore'):
            want = np.percentile(x, QS)
        assert want.dtype == np.float64
        assert same(dr.percentile(x, QS), want), x[:8]
        # the product's interpolation from the two order statistics of every percentage
        _, _, vals = dr.order_stats(x, QS)
        assert same(display.interpolate(np.asarray(QS, dtype=np.float64), x.size, vals), want), x[:8]
        for q in (0, 37.5, 100):
            with np.errstate(invalid='ignore'):
                assert same(dr.percentile(x, q), np.percentile(x, [q])[0])       # (float64 for a scalar q too)
    x = value_sets(dtype)[4].copy()
    x[::3] = np.nan
    assert same(dr.percentile(x, QS), np.percentile(x[~np.isnan(x)], QS))
    assert np.all(np.isnan(dr.percentile(x, QS, skip_nan=False))) and np.all(np.isnan(np.percentile(x, QS)))
    with pytest.raises(IndexError):
        dr.percentile(np.full(5, np.nan, dtype=dtype), (10, 90))
    with pytest.raises(IndexError):
        np.percentile(np.array([], dtype=dtype), (10, 90))


def test_all_fixtures_are_present():
    assert len(NAMES) == 7
    dtypes = [dr.load_fixture(GOLDEN, n)['data'].dtype for n in NAMES]
    assert dtypes.count(np.dtype(np.float32)) >= 3 and dtypes.count(np.dtype(np.float64)) >= 3
    assert sum(int(dr.load_fixture(GOLDEN, n)['flatten_layer']) >= 0 for n in NAMES) == 4
    for path in os.listdir(GOLDEN):
        if path.startswith('FD'):
            assert os.path.getsize(os.path.join(GOLDEN, path)) < 1000 * 1024, path


def ranges_of(g):
    snum, tnum = g['data'].shape
    x0, x1 = int(g['x_range_in'][0]), int(g['x_range_in'][1])
    y0, y1 = int(g['y_range_in'][0]), int(g['y_range_in'][1])
    return (y0, snum if y1 == -1 else y1), (x0, tnum if x1 == -1 else x1)


@pytest.mark.parametrize('name', NAMES)
def test_restatement_is_what_the_reference_drew(name):
    from impdar_amd import display
    g = dr.load_fixture(GOLDEN, name)
    data = g['data']
    (y0, y1), (x0, x1) = ranges_of(g)
    assert np.array_equal(g['x_range_out'], (x0, x1))
    assert same(dr.percentile(data[y0:y1, x0:x1], (10, 90)), g['clims'])
    first = int(np.min(np.where(~np.isnan(g['travel_time']))[0])) if str(g['ydat']) in ('twtt', 'dual') else 0
    layer = int(g['flatten_layer'])
    if layer >= 0:
        offset, mask = dr.get_offset(g['samp2'][list(g['picknums']).index(layer)])
        assert np.array_equal(mask, np.isnan(offset))
        image = dr.flatten_loop(data, offset)[:, x0:x1]
        shift = dr.shifts(offset, data.shape[0])
        assert same(dr.flatten_gather(data, shift)[:, x0:x1], image)
        assert np.array_equal(display.shifts_from_offset(offset, data.shape[0]), shift)
        if 'wild' in name:
            k = shift[shift != dr.NO_SHIFT]
            assert (k == 0).any() and (k > 0).any() and (k < 0).any() and (np.abs(k) >= data.shape[0]).any()
    else:
        image = data[max(y0, first):y1, x0:x1]
    assert same(image, g['image']) and np.array_equal(np.isnan(image), g['image_mask'])
    # the traces' limits: the (1, 99) percentiles, mirrored where they straddle zero
    t0, t1 = int(g['tr'][0]), int(g['tr'][1])
    t1 = t0 + 1 if t1 == t0 else t1
    lims = dr.percentile(data[:, t0:t1], (1, 99), skip_nan=False)
    want = (lims[0], -lims[0]) if lims[0] < 0 and lims[1] > 0 else tuple(lims)
    assert tuple(g['trace_xlim']) == want


@pytest.fixture(scope='module')
def route(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('displayroute'))
    src, so = os.path.join(tmp, 'display_route_probe.cpp'), os.path.join(tmp, 'libdisplayroute.so')
    with open(src, 'w') as f:
        f.write('#define DISPLAY_ROUTE_PROBE 1\n#include "display_route.h"\n')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-shared', '-fPIC', '-I', CSRC, src, '-o', so])
    lib = C.CDLL(so)
    ll, llp, dp = C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(C.c_double)
    lib.impdar_display_ranks_probe.argtypes = [ll, C.c_double, llp, llp]
    lib.impdar_display_grid_probe.argtypes = [ll, ll, C.c_int, llp]
    lib.impdar_display_select_probe.argtypes = [dp, ll, C.c_int, llp, C.c_int, dp]
    return lib


@needs_gxx
def test_header_forms_numpys_ranks(route):
    lo, hi = C.c_longlong(), C.c_longlong()
    for n in (1, 2, 3, 7, 100, 1001, 40960000, 2 ** 40 + 1):
        for q in QS + (0.1, 99.9, 12.5):
            route.impdar_display_ranks_probe(n, q, C.byref(lo), C.byref(hi))
            want = dr.ranks(n, q)
            assert (lo.value, hi.value) == (int(want[0]), int(want[1])), (n, q)


@needs_gxx
def test_header_grid_covers_the_window(route):
    out = (C.c_longlong * 4)()
    for rows, width, V in ((1, 1, 1), (5, 1, 1), (27, 17, 1), (64, 2, 2), (130, 1030, 2), (512, 2051, 1), (4096, 10000, 4),
                           (4096, 100, 4), (1, 2 ** 24, 4), (2 ** 20, 3, 1), (70000 * 256, 1, 1)):
        assert route.impdar_display_grid_probe(rows, width, V, out) == 0, (rows, width, V)
        log_tx, gx, gy, per_wg = list(out)
        tx, ty, units = 1 << log_tx, 256 >> log_tx, width // V
        assert 1 <= tx <= 256 and gx * tx >= units > (gx - 1) * tx
        assert 1 <= gy <= 65535 and gy <= -(-rows // ty) and gx * gy <= max(2048, gx)
        assert per_wg >= -(-(-(-rows // ty)) // gy) * ty * tx * V and per_wg < 2 ** 32
    assert route.impdar_display_grid_probe(4, 10, 4, out) == 1          # (the width is no multiple of the access)
    assert route.impdar_display_grid_probe(0, 10, 1, out) == 1


@needs_gxx
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_header_select_finds_the_sorted_values(route, dtype):
    """The library's host code around a stand-in for its kernel: histograms counted on the host, one pass per digit."""
    for x in value_sets(dtype):
        n = x.size
        lo, hi, _ = dr.ranks(n, np.asarray(QS, dtype=np.float64))
        ranks = np.ascontiguousarray(np.stack((lo, hi), axis=1).reshape(-1), dtype=np.int64)
        vals = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty(ranks.size, dtype=np.float64)
        rc = route.impdar_display_select_probe(vals.ctypes.data_as(C.POINTER(C.c_double)), n, int(dtype == np.float32),
                                               ranks.ctypes.data_as(C.POINTER(C.c_longlong)), ranks.size,
                                               out.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == 0
        assert np.array_equal(out.astype(dtype), np.sort(x)[ranks]), x[:8]
    # a rank beyond the counted elements is reported, not followed
    one = np.ones(3)
    bad = np.array([5], dtype=np.int64)
    assert route.impdar_display_select_probe(one.ctypes.data_as(C.POINTER(C.c_double)), 3, 0, bad.ctypes.data_as(C.POINTER(C.c_longlong)), 1,
                                             np.empty(1).ctypes.data_as(C.POINTER(C.c_double))) == 1


def test_argument_errors_come_before_any_device_call(monkeypatch):
    from impdar_amd import _hip, display

    def no_device(*a, **k):
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_hip, 'load', no_device)
    monkeypatch.setattr(_hip, 'context', no_device)
    data = np.zeros((12, 5), dtype=np.float32)
    with pytest.raises(ValueError, match=r'Percentiles must be in the range \[0, 100\]'):
        display.percentile_host(data, (10, 101))
    with pytest.raises(ValueError, match=r'Percentiles must be in the range \[0, 100\]'):
        display.percentile_host(data, float('nan'))
    with pytest.raises(ValueError, match='q is empty'):
        display.percentile_host(data, ())
    with pytest.raises(ValueError, match='y_range'):
        display.percentile_host(data, 50, y_range=(9, 3))
    with pytest.raises(ValueError, match='x_range'):
        display.percentile_host(data, 50, x_range=(-2, 3))
    with pytest.raises(TypeError, match='complex'):
        display.percentile_host(data.astype(np.complex64), 50)
    with pytest.raises(ValueError, match=r'\(snum, tnum\)'):
        display.percentile_host(np.zeros(4), 50)
    with pytest.raises(IndexError):
        display.percentile_host(np.zeros((0, 4)), 50)
    with pytest.raises(ValueError, match='one int32 per trace'):
        display.flatten_host(data, np.zeros(4, dtype=np.int32))
    with pytest.raises(ValueError, match='one int32 per trace'):
        display.flatten_host(data, np.zeros(5, dtype=np.int64))
    with pytest.raises(ValueError, match='no traces'):
        display.flatten_host(data, np.zeros(0, dtype=np.int32), x_range=(2, 2))
    with pytest.raises(TypeError, match='complex'):
        display.flatten_host(data.astype(np.complex128), np.zeros(5, dtype=np.int32))
    # a host window needs no device at all
    assert np.array_equal(display.window_host(np.arange(12).reshape(3, 4), (1, -1), (1, 3)), [[5, 6], [9, 10]])
    # ... and neither do the offsets of a layer, nor their refusal
    from impdar_amd.lib import plot
    from impdar_amd.lib.RadarData import RadarData
    dat = dr.fill_dat(RadarData(None), dr.load_fixture(GOLDEN, 'FD04_37x19_f64_flatten_wild'))
    offset, mask = plot.get_offset(dat, 7)
    want = dr.get_offset(dat.picks.samp2[1])
    assert same(offset, want[0]) and np.array_equal(mask, want[1])
    assert np.array_equal(plot.get_offset(dat)[0], np.zeros(19)) and not plot.get_offset(dat)[1].any()
    with pytest.raises(ValueError, match='That layer is not in existence, cannot flatten'):
        dat.flattened(5)


class Recorder(object):
    def __init__(self):
        self.calls = []

    def __call__(self, name):
        def record(*args, **kwargs):
            import matplotlib.pyplot as plt
            self.calls.append((name, args, kwargs))
            return plt.subplots()
        return record


def test_plot_routes_to_the_kind_asked_for(monkeypatch):
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    from impdar_amd.lib import plot
    rec = Recorder()
    dats = [type('D', (), {'fn': None})(), type('D', (), {'fn': None})()]
    monkeypatch.setattr(plot, 'load', lambda filetype, fns: dats)
    monkeypatch.setattr(plt, 'show', lambda *a, **k: None)
    for name in ('plot_radargram', 'plot_traces', 'plot_power', 'plot_ft', 'plot_hft', 'plot_spectrogram'):
        monkeypatch.setattr(plot, name, rec(name))
    plot.plot(['a.mat', 'b.mat'])
    assert [c[0] for c in rec.calls] == ['plot_radargram', 'plot_radargram']
    assert rec.calls[0][1] == (dats[0],)
    assert rec.calls[0][2] == dict(xdat='tnum', ydat='twtt', x_range=None, pick_colors=None, clims=None, cmap=None, flatten_layer=None)
    del rec.calls[:]
    plot.plot(['a.mat'], xd=True, dualy=True, pick_colors=True, clims=[-1.0, 2.0], cmap='magma', flatten_layer=4)
    assert rec.calls[0][2] == dict(xdat='dist', ydat='dual', x_range=None, pick_colors=True, clims=[-1.0, 2.0], cmap='magma',
                                   flatten_layer=4)
    del rec.calls[:]
    plot.plot(['a.mat'], yd=True, tr=(3, 9))
    assert rec.calls == [('plot_traces', (dats[0], (3, 9)), dict(ydat='depth')), ('plot_traces', (dats[1], (3, 9)), dict(ydat='depth'))]
    del rec.calls[:]
    plot.plot(['a.mat'], power=6)
    assert rec.calls == [('plot_power', (dats, 6), {})]           # all files on one axis
    del rec.calls[:]
    plot.plot(['a.mat'], ft=True)
    plot.plot(['a.mat'], hft=True)
    plot.plot(['a.mat'], spectra=(1.0, 5.0), window='hann')
    assert [c[0] for c in rec.calls] == 2 * ['plot_ft'] + 2 * ['plot_hft'] + 2 * ['plot_spectrogram']
    with pytest.raises(ValueError, match='Only one of yd and dualy can be true'):
        plot.plot(['a.mat'], yd=True, dualy=True)
    with pytest.raises(ValueError, match=r'Cannot do both tr and power\. Pick one'):
        plot.plot(['a.mat'], tr=(1, 2), power=3)
    plt.close('all')


def test_impplot_parsers_hand_on_the_references_options(monkeypatch):
    from impdar_amd.bin import impplot
    from impdar_amd.lib import plot
    calls = []
    monkeypatch.setattr(plot, 'plot', lambda *a, **k: calls.append((a, k)))
    parser = impplot._get_args()

    def run(argv):
        args = parser.parse_args(argv)
        args.func(**vars(args))
        return calls.pop()
    a, k = run(['rg', '-s', '-picks', '-flatten_layer', '2', '-clims', '-3', '4.5', '-cmap', 'bone', '-xd', '-dualy', 'x.mat', 'y.mat'])
    assert a == (['x.mat', 'y.mat'],)
    assert k == dict(xd=True, yd=False, s=True, o=None, ftype='png', dpi=300, filetype='mat', pick_colors=True, cmap='bone',
                     clims=[-3.0, 4.5], flatten_layer=2, dualy=True)
    a, k = run(['rg', 'x.mat'])
    assert k['pick_colors'] is False and k['clims'] is None and k['cmap'] == 'gray' and k['flatten_layer'] is None and not k['s']
    a, k = run(['traces', '-yd', '--o_fmt', 'pdf', 'x.mat', '3', '9'])
    assert k == dict(tr=(3, 9), yd=True, s=False, o=None, ftype='pdf', dpi=300, dualy=False, filetype='mat')
    a, k = run(['power', '-dpi', '100', 'x.mat', 'y.mat', '7'])
    assert a == (['x.mat', 'y.mat'],) and k == dict(power=7, s=False, o=None, ftype='png', dpi=100, filetype='mat')
    a, k = run(['ft', 'x.mat'])
    assert k['ft'] is True                                          # (the earlier sub-commands are as they were)
    with pytest.raises(SystemExit):
        parser.parse_args(['traces', 'x.mat', '3'])


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, 'include', 'impdar_hip.h')).read()
    from impdar_amd import _hip
    for name in ('impdar_order_stats', 'impdar_order_stats_dev', 'impdar_flatten', 'impdar_flatten_dev', 'impdar_window_dev'):
        assert re.search(r'\bint %s\(' % name, text), name
        assert name in _hip.SIGNATURES
    assert re.search(r'#define IMPDAR_FLATTEN_NONE \(-2147483647 - 1\)', text)
    from impdar_amd import build, display
    assert 'display.hip' in build.SOURCES and display.NO_SHIFT == -2147483648


def test_radardata_has_the_methods_and_import_stays_light():
    import sys
    code = ('import sys, impdar_amd, impdar_amd.display, impdar_amd.lib.plot, impdar_amd.bin.impplot, impdar_amd.lib.RadarData as R; '
            'assert all(hasattr(R.RadarData, m) for m in ("percentiles", "window", "flattened")); '
            'assert "matplotlib" not in sys.modules')
    subprocess.check_call([sys.executable, '-c', code], cwd=ROOT)
