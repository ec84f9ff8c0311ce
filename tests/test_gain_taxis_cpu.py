"""The gains, the trace-axis steps and winavg_hfilt without a GPU: the host tables (gain and start rows, window
bounds, tapers, crop indices, block means) reproduce every ``G*`` / ``R*`` / ``AW*`` fixture of the reference in NumPy
-- rangegain, agc, reverse and hcrop bit for bit, restack and winavg_hfilt within 1e-12 (float64) and 2e-6 (float32
and int16 input) of max|expected| -- the attribute, flag and message bookkeeping of the ``RadarData`` methods with
the device calls replaced by those NumPy restatements, the reference's errors, the refusal of picks, the ``impproc``
sub-commands with mocked data, and the new symbols of the C ABI."""
import contextlib
import io
import os
import sys
import warnings
from unittest.mock import MagicMock, patch

import numpy as np
import pytest

from conftest import ROOT, golden, golden_names
from impdar_amd import gain, hfilt as hf, taxis
from impdar_amd.bin import impproc
from impdar_amd.lib import process
from impdar_amd.lib.RadarData import RadarData

CASES = [n for p in ('G', 'R', 'AW') for n in golden_names(p) if n != 'GZ_errors']
EXACT = ('rangegain', 'agc', 'reverse', 'hcrop')
VECTORS = ['dist', 'pressure', 'lat', 'long', 'x_coord', 'y_coord', 'elev', 'decday', 'trig', 'trace_num', 'trace_int']
FLAGS = ['rgain', 'agc', 'restack', 'reverse', 'hfilt']


def bar(in_dtype):
    """max|diff| / max|expected| allowed for restack and winavg_hfilt: the bars hfilt and nmo are held to."""
    return 1e-12 if in_dtype == np.float64 else 2e-6


# ------------------------------------------------------------------------------- NumPy stand-ins for the kernels
def np_rangegain(data, g, start):
    data = np.asarray(data)
    gain.refuse_integers(data.dtype)
    rows = np.arange(data.shape[0])[:, None] >= start[None, :]
    return np.where(rows, (data.astype(np.float64) * g[:, None]).astype(data.dtype), data)


def np_agc(data, half, scaling_factor):
    data = np.asarray(data)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        rowmax = np.max(np.abs(data), axis=1).astype(np.float64)
        maxamp = gain.window_max(rowmax, half)
    return data * (scaling_factor / maxamp).astype(data.dtype)[:, None]


def np_restack(data, traces):
    data = np.asarray(data)
    snum, tnum = data.shape
    n = tnum // traces
    return data[:, :n * traces].astype(np.float64).reshape(snum, n, traces).sum(axis=2) / traces


def np_winavg(data, lo, hi, scale):
    data = np.asarray(data)
    work = data if data.dtype in (np.float32, np.float64) else data.astype(np.float64)
    out = np.empty(work.shape, dtype=work.dtype)
    with warnings.catch_warnings(), np.errstate(invalid='ignore'):
        warnings.simplefilter('ignore')
        for i in range(work.shape[1]):
            m = np.mean(work[:, lo[i]:hi[i]].astype(np.float64), axis=1).astype(work.dtype)
            out[:, i] = work[:, i] - m.astype(np.float64) * scale
        return out.astype(data.dtype)


@contextlib.contextmanager
def kernels_in_numpy():
    with patch.object(gain, 'rangegain_host', np_rangegain), patch.object(gain, 'agc_host', np_agc), \
            patch.object(taxis, 'restack_host', np_restack), patch.object(hf, 'winavg_host', np_winavg):
        yield


# ------------------------------------------------------------------------------------------- fixture plumbing
def dat_of(g, resident=False):
    d = RadarData(None)
    d.data = g['in_data'].copy()
    d.snum, d.tnum = d.data.shape
    d.dt = 0.3e-6
    d.travel_time = g['in_travel_time'].copy()
    for k in VECTORS:
        v = g['in_' + k] if 'in_' + k in g else None
        setattr(d, k, None if v is None else (v.copy() if v.ndim else v.item()))
    for k in FLAGS:
        v = g['in_flags_' + k]
        setattr(d.flags, k, v.copy() if v.ndim else bool(v))
    if resident:
        d.to_device()
    return d


def call_of(g):
    kind = g['kind'].item()
    args = [a.item() for a in g['args']]
    if kind in ('restack', 'winavg_hfilt') or (kind == 'hcrop' and g['kw_dimension'].item() == 'tnum'):
        args = [int(a) for a in args]
    kw = {k[3:]: v.item() for k, v in g.items() if k.startswith('kw_')}
    return kind, args, kw


def check_data(got, g):
    want, kind = g['out_data'], g['kind'].item()
    assert got.shape == want.shape and got.dtype == want.dtype
    nan = np.isnan(want.astype(np.float64))
    np.testing.assert_array_equal(np.isnan(got.astype(np.float64)), nan)
    if kind in EXACT:
        np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))
    elif not nan.all():
        ok = ~nan
        err = float(np.max(np.abs(got[ok].astype(np.float64) - want[ok]))) / float(np.max(np.abs(want[ok].astype(np.float64))))
        print('%s: max|diff| / max|expected| = %.3e' % (kind, err))
        assert err <= bar(g['in_data'].dtype), err


def check_state(d, g, data):
    check_data(data, g)
    assert d.tnum == int(g['out_tnum']) and d.snum == int(g['out_snum'])
    np.testing.assert_array_equal(d.travel_time, g['out_travel_time'])
    for k in VECTORS:
        if 'out_' + k in g:
            assert np.shape(getattr(d, k)) == g['out_' + k].shape, k
            np.testing.assert_array_equal(np.asarray(getattr(d, k)), g['out_' + k], err_msg=k)
        else:
            assert getattr(d, k) is None, k
    for k in FLAGS:
        np.testing.assert_array_equal(np.asarray(getattr(d.flags, k), dtype=np.float64), g['out_flags_' + k], err_msg=k)


def run_fixture(g, resident=False):
    """The step of a fixture on a host or resident RadarData; the data after it."""
    d = dat_of(g, resident=resident)
    kind, args, kw = call_of(g)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        for _ in range(int(g['ncalls'])):
            getattr(d, kind)(*args, **kw)
    if resident:
        assert d.data is None
        data = d._dev.to_host()
    else:
        data = d.data
    check_state(d, g, data)
    assert out.getvalue() == g['stdout'].item()
    return d, data


# ------------------------------------------------------------------------------------------------ the tests
def test_fixtures_cover_the_cases():
    gs = {n: golden(n) for n in CASES}
    kinds = [g['kind'].item() for g in gs.values()]
    for kind in ('agc', 'reverse', 'hcrop', 'restack', 'winavg_hfilt'):
        dtypes = {g['in_data'].dtype for g in gs.values() if g['kind'].item() == kind}
        assert dtypes == {np.dtype(np.float64), np.dtype(np.float32), np.dtype(np.int16)}, kind
        assert any(g['in_data'].shape[1] % 2 for g in gs.values() if g['kind'].item() == kind), kind
    assert kinds.count('rangegain') >= 4 and 'rangegain_int16_scalar_trig' in golden('GZ_errors')['label']
    assert gs['G1_rgain_f64_scalar_trig']['in_trig'].ndim == 0 and gs['G2_rgain_f32_vector_trig']['in_trig'].ndim == 1
    assert gs['G3_rgain_f32_trig_minus1_odd_tnum']['in_trig'] == -1
    g = gs['G6_agc_f32_nan_window10_odd_tnum']
    assert list(np.flatnonzero(np.isnan(g['out_data']).all(axis=1))) == list(range(6, 16))       # NaN at row 10, window 10
    assert not g['in_data'][45].any() and int(g['kw_window']) % 2 == 0
    assert int(gs['G7_agc_f32_odd_window']['kw_window']) % 2 == 1
    g = gs['RB_restack_f32_even_request_remainder']
    assert g['args'][0] == 4 and g['out_tnum'] == 9 and 9 * 5 < g['in_tnum'] and g['out_data'].dtype == np.float64
    assert all(g['out_data'].dtype == np.float64 for g in gs.values() if g['kind'].item() == 'restack')
    crops = {(g['kw_left_or_right'].item(), g['kw_dimension'].item()) for g in gs.values() if g['kind'].item() == 'hcrop'}
    assert crops == {('left', 'tnum'), ('right', 'tnum'), ('left', 'dist'), ('right', 'dist')}
    assert gs['R8_hcrop_left_negative_f32_odd_tnum']['args'][0] < 0
    assert gs['AW2_winavg_f32_pexp_even']['kw_taper'].item() == 'pexp' and gs['AW2_winavg_f32_pexp_even']['args'][0] % 2 == 0
    assert gs['AW4_winavg_f64_past_tnum']['args'][0] > gs['AW4_winavg_f64_past_tnum']['in_tnum']
    assert np.isnan(gs['AW5_winavg_f64_window1_nan']['out_data']).all()
    for n in CASES + ['GZ_errors']:
        assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', n + '.npz')) < 300 * 1024


@pytest.mark.parametrize('name', CASES)
def test_host_tables_and_bookkeeping_match_the_reference(name):
    with kernels_in_numpy():
        run_fixture(golden(name))


def test_rangegain_start_rows_follow_python_slicing():
    tt = np.arange(10) * 0.5
    for trig in (-12, -10, -3, -1, 0, 4, 8, 9, 30):
        g, start = gain.rangegain_tables(tt, trig, 2.0, 10, 3)
        want = np.zeros(10, dtype=bool)
        want[int(trig) + 1:] = True
        assert list(start) == [slice(int(trig) + 1, None).indices(10)[0]] * 3
        np.testing.assert_array_equal(np.arange(10) >= start[0], want)
        np.testing.assert_array_equal(g, tt * 2.0)
    _, start = gain.rangegain_tables(tt, np.array([2.9, -1., 0.]), 1.0, 10, 3)
    assert list(start) == [3, 0, 1]


def test_winavg_windows_and_tapers_are_the_references():
    for tnum in (1, 2, 7, 30):
        for win in range(1, 41, 2):
            lo, hi = hf.winavg_windows(tnum, win)
            h = (win - 1) // 2
            for i in range(tnum):
                assert (lo[i], hi[i]) == (max(0, i - h), max(min(i + h, tnum), max(0, i - h)))
                assert hi[i] - lo[i] == len(range(tnum)[max(0, i - h):min(i + h, tnum)])
    with contextlib.redirect_stdout(io.StringIO()) as out:
        assert hf.winavg_window(10, 48) == 11 and hf.winavg_window(130, 48) == 49 and hf.winavg_window(7, 48) == 7
        assert hf.winavg_window(131, 49) == 49
    assert out.getvalue().count('Reducing avg_win to tnum') == 2 and out.getvalue().count('changed to 49') == 1
    tt = np.arange(80) * 0.3 + 0.5
    full = hf.winavg_taper(tt)
    np.testing.assert_array_equal(full, hf.taper(tt))
    pexp = hf.winavg_taper(tt, 'pexp', 40)
    assert pexp[0] == 1.0 and not pexp[40:].any() and (np.diff(pexp[:41]) < 0).all()
    with pytest.raises(NotImplementedError):
        hf.winavg_taper(tt, 'tukey')


def test_errors_are_the_references():
    g = golden('GZ_errors')
    want = {str(l): (str(t), str(m)) for l, t, m in zip(g['label'], g['exc_type'], g['message'])}
    some = golden('R1_reverse_f64')
    tnum = g['data'].shape[1]

    def dat(data=g['data'], trig=None):
        d = dat_of(some)
        d.data = data.copy()
        if trig is not None:
            d.trig = trig
        return d
    calls = {'rangegain_int16_scalar_trig': lambda: dat(g['data_int16'], trig=3).rangegain(0.1),
             'rangegain_int16_vector_trig': lambda: dat(g['data_int16']).rangegain(0.1),
             'agc_window_1': lambda: dat().agc(window=1),
             'hcrop_left_or_right': lambda: dat().hcrop(5, left_or_right='top'),
             'hcrop_dimension': lambda: dat().hcrop(5, dimension='snum'),
             'hcrop_dist_too_large': lambda: dat().hcrop(50., dimension='dist'),
             'hcrop_dist_not_positive': lambda: dat().hcrop(0., dimension='dist'),
             'hcrop_tnum_0': lambda: dat().hcrop(0),
             'hcrop_tnum_1': lambda: dat().hcrop(1),
             'hcrop_tnum_too_large': lambda: dat().hcrop(tnum + 1),
             'hcrop_tnum_minus_1': lambda: dat().hcrop(-1),
             'hcrop_tnum_too_negative': lambda: dat().hcrop(-tnum - 1),
             'winavg_taper': lambda: dat().winavg_hfilt(7, taper='cosine')}
    assert set(calls) == set(want)
    types = {'ValueError': ValueError, 'UFuncTypeError': TypeError}
    for label, fn in calls.items():
        with kernels_in_numpy(), pytest.raises(types[want[label][0]]) as e:
            fn()
        assert str(e.value) == want[label][1], label
    with kernels_in_numpy(), pytest.raises(NotImplementedError):
        dat().winavg_hfilt(7, taper='tukey')
    d = dat()
    before = d.data.copy()
    with kernels_in_numpy(), pytest.raises(ValueError):
        d.agc(window=0)
    assert np.array_equal(d.data, before) and not d.flags.agc


def test_real_picks_are_refused():
    for call in (lambda d: d.reverse(), lambda d: d.hcrop(5), lambda d: d.restack(3)):
        d = dat_of(golden('R1_reverse_f64'))
        d.picks = object()
        before = d.data.copy()
        with kernels_in_numpy(), pytest.raises(NotImplementedError):
            call(d)
        assert np.array_equal(d.data, before) and d.tnum == before.shape[1] and not d.flags.reverse and not d.flags.restack
    d = dat_of(golden('G1_rgain_f64_scalar_trig'))
    d.picks = object()                                 # the gains move nothing
    with kernels_in_numpy():
        d.rangegain(0.1)
        d.agc()
    assert d.flags.rgain and d.flags.agc


def run_impproc(argv, loaded):
    with patch.object(sys, 'argv', ['impproc'] + argv), patch('impdar_amd.bin.impproc.load', return_value=loaded):
        impproc.main()


def test_impproc_sub_commands_forward_and_name_outputs():
    dat = MagicMock()
    run_impproc(['rev', 'line_raw.mat'], [dat])
    dat.reverse.assert_called_with()
    dat.save.assert_called_with('line_rev.mat')
    dat = MagicMock()
    run_impproc(['hcrop', 'right', 'dist', '1.5', 'line_raw.mat'], [dat])
    dat.hcrop.assert_called_with(1.5, left_or_right='right', dimension='dist')
    dat.save.assert_called_with('line_hcropped.mat')
    dat = MagicMock()
    run_impproc(['hcrop', 'left', 'tnum', '20', 'x.mat', '-o', 'y.mat'], [dat])
    dat.hcrop.assert_called_with(20.0, left_or_right='left', dimension='tnum')
    dat.save.assert_called_with('y.mat')
    with pytest.raises(SystemExit):
        run_impproc(['hcrop', 'top', 'tnum', '3', 'x.mat'], [MagicMock()])
    dat = MagicMock()
    run_impproc(['restack', '5', 'line_raw.mat'], [dat])
    dat.restack.assert_called_with(5)
    dat.save.assert_called_with('line_restacked.mat')
    with pytest.raises(SystemExit):
        run_impproc(['restack', '2.5', 'x.mat'], [MagicMock()])
    dat = MagicMock()
    run_impproc(['rgain', 'line_raw.mat'], [dat])
    dat.rangegain.assert_called_with(0.1)
    dat.save.assert_called_with('line_rgain.mat')
    dat = MagicMock()
    run_impproc(['rgain', '-slope', '0.02', 'x.mat'], [dat])
    dat.rangegain.assert_called_with(0.02)
    dat = MagicMock()
    run_impproc(['agc', 'line_raw.mat'], [dat])
    dat.agc.assert_called_with(window=50, scaling_factor=50)
    dat.save.assert_called_with('line_agc.mat')
    dat = MagicMock()
    run_impproc(['agc', '-window', '31', 'a_raw.mat', 'b.mat', '-o', 'out/'], [dat, dat])
    dat.agc.assert_called_with(window=31, scaling_factor=50)
    dat.save.assert_called_with(os.path.join('out/', 'b_agc.mat'))
    with pytest.raises(SystemExit):
        run_impproc(['winavg', '5', 'x.mat'], [MagicMock()])


@pytest.mark.parametrize('step', ['restack', 'hcrop', 'rev'])
def test_process_still_rejects_these_steps(step):
    with pytest.raises(NotImplementedError):
        process.process([MagicMock()], **{step: 3})


def test_abi_declares_the_new_entry_points():
    from impdar_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'impdar_hip.h')).read()
    for name in ('impdar_rangegain', 'impdar_rangegain_dev', 'impdar_agc', 'impdar_agc_dev', 'impdar_row_absmax',
                 'impdar_restack', 'impdar_restack_dev', 'impdar_reverse_dev', 'impdar_hcrop_dev', 'impdar_winavg',
                 'impdar_winavg_dev'):
        assert name + '(' in header and name in _hip.SIGNATURES
