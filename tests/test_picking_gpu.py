"""Layer picking on the MI355X: ``csrc/pick.hip`` against the ``PK*`` fixtures of the reference, every case through
the host-buffer entry and through a resident array, in float32 and float64.

Bars (the reference's, none from this code's output): rows 0-2 of every pick equal as integers, row 3 NaN, NaN
positions of the power equal, |p - p_ref| <= 2 (n + 2) u p_ref over n squared samples; error kind, message and
place equal; continuity index NaN where the reference's is, else within 16 u max(1, max|P| in the windows) (the
reference's float32 result lies within 0.015 of that bar from its own float64 one, so the bar stands as set).
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden, golden_names
from impdar_amd import picking
from impdar_amd.lib import picklib
from impdar_amd.lib.PickParameters import PickParameters
from impdar_amd.lib.Picks import Picks
from impdar_amd.lib.RadarData import RadarData
from picking_ref import assert_continuity, assert_picks, continuity_runs, prm_of

pytestmark = pytest.mark.gpu
DTYPES = [(np.float32, '32'), (np.float64, '64')]
_IP = C.POINTER(C.c_int)
SAVED = os.path.join(GOLDEN, 'PK_ref_saved_picked.mat')
AUTO = [n for n in golden_names('PK') if n[2:4] < '20']
GUIDED = golden_names('PK3')
CONT = golden_names('PK4')


def entries(hip, data):
    """The radargram as the host-buffer entry takes it and as a resident array."""
    return [('host', data), ('resident', hip.DeviceArray.from_host(hip.context(), data))]


def raw_auto(hip, where, snums, tnums, prm):
    """The C entry itself: (picks, status) without the wrapper's raise."""
    s, t = np.asarray(snums, dtype=np.int32), np.asarray(tnums, dtype=np.int32)
    snum, tnum = where.shape
    out = np.zeros((len(s), 5, tnum))
    status = np.full((len(s), 2), 77, dtype=np.int32)
    args = (hip.dtype_code(where.dtype), snum, tnum, len(s), s.ctypes.data_as(_IP), t.ctypes.data_as(_IP), *prm,
            hip.as_dp(out)[1], status.ctypes.data_as(_IP))
    if isinstance(where, np.ndarray):
        rc = hip.load().impdar_auto_pick(hip.context(), where.ctypes.data_as(C.c_void_p), *args)
    else:
        rc = hip.load().impdar_auto_pick_dev(where.ctx, where.ptr, *args)
    hip.check(rc, 'impdar_auto_pick')
    return out, status


def raw_guided(hip, where, t0, mid, prm):
    mid = np.asarray(mid, dtype=np.int32)
    snum, tnum = where.shape
    out = np.zeros((5, len(mid)))
    status = np.full((2,), 77, dtype=np.int32)
    args = (hip.dtype_code(where.dtype), snum, tnum, t0, len(mid), mid.ctypes.data_as(_IP), *prm, hip.as_dp(out)[1],
            status.ctypes.data_as(_IP))
    if isinstance(where, np.ndarray):
        rc = hip.load().impdar_pick_guided(hip.context(), where.ctypes.data_as(C.c_void_p), *args)
    else:
        rc = hip.load().impdar_pick_guided_dev(where.ctx, where.ptr, *args)
    hip.check(rc, 'impdar_pick_guided')
    return out, status


def auto(where, snums, tnums, prm):
    fn = picking.auto_pick_host if isinstance(where, np.ndarray) else picking.auto_pick_dev
    return fn(where, snums, tnums, *prm)


@pytest.mark.parametrize('name', AUTO)
def test_auto_pick_reproduces_the_reference(hip, name):
    g = golden(name)
    prm, code = prm_of(g), int(g['code'])
    for dtype, tag in DTYPES:
        for entry, where in entries(hip, np.ascontiguousarray(g['data'].astype(dtype))):
            what = '%s %s %s' % (name, tag, entry)
            out, status = raw_auto(hip, where, g['snums'], g['tnums'], prm)
            if code == 0:
                assert np.array_equal(status, [[0, -1]] * len(g['snums'])), what
                assert_picks(out, g['out' + tag], dtype, what + ' raw')
                assert_picks(auto(where, g['snums'], g['tnums'], prm), g['out' + tag], dtype, what)
            else:
                k = int(g['fail_seed'])
                assert np.all(status[:k, 0] == 0) and status[k].tolist() == [code, int(g['fail_trace'])], what
                with pytest.raises(ValueError) as e:
                    auto(where, g['snums'], g['tnums'], prm)
                assert str(e.value) == str(g['message']), what
            if 'partial' + tag in g:      # what every seed's chain had picked before it left the data
                assert np.array_equal(status[:, 0], g['seed_codes']) and np.array_equal(status[:, 1], g['seed_traces']), what
                # a seed's two walks are two waves: where the left one fails the right one still runs, which the
                # reference's loop never reaches; every pick the reference's chain made is compared
                want = g['partial' + tag]
                reached = ~np.isnan(want[:, :1, :])
                assert not np.any(np.isnan(out[:, :3][np.broadcast_to(reached, out[:, :3].shape)])), what
                assert_picks(np.where(reached, out, np.nan), want, dtype, what + ' chains')


def test_duplicate_seeds_and_one_layer_from_two_seeds(hip):
    g = golden('PK01_basic_pos')
    out = picking.auto_pick_host(g['data'], g['snums'], g['tnums'], *prm_of(g))
    assert np.array_equal(out[1], out[4], equal_nan=True)          # the duplicate seed
    assert np.array_equal(out[0, :3], out[1, :3])                  # (30, 0) and (35, 35) follow the same layer


def test_steep_dips_follow_the_layer(hip):
    for name, slope in (('PK09_steep3', 3), ('PK10_steep8', 8)):
        g = golden(name)
        out = picking.auto_pick_host(g['data'], g['snums'], g['tnums'], *prm_of(g))
        j = np.arange(70)
        assert np.max(np.abs(out[0, 1] - (40 + slope * j + 2 * np.sin(j / 9.)))) <= 1.3


def test_c_entries_refuse_bad_arguments(hip):
    g = golden('PK15_one_trace')
    data = np.ascontiguousarray(g['data'])
    with pytest.raises(ValueError, match='starts at trace'):
        raw_auto(hip, data, [30], [1], prm_of(g))
    with pytest.raises(ValueError, match='FWW'):
        raw_auto(hip, data, [30], [0], (49, 0, 16, 1))
    with pytest.raises(ValueError, match='pol'):
        raw_auto(hip, data, [30], [0], (49, 17, 16, 2))
    with pytest.raises(ValueError, match='traces'):
        raw_guided(hip, data, 0, [30, 30], prm_of(g))


@pytest.mark.parametrize('name', GUIDED)
def test_guided_pick_reproduces_the_reference(hip, name):
    g = golden(name)
    t0, n, prm = int(g['t0']), int(g['n']), prm_of(g)
    mid = picking.midpoints(n, int(g['snum_start']), int(g['snum_end']))
    for dtype, tag in DTYPES:
        data = np.ascontiguousarray(g['data'].astype(dtype))
        for entry, where in entries(hip, data):
            fn = picking.pick_host if entry == 'host' else picking.pick_dev
            assert_picks(fn(where, t0, mid, *prm), g['out' + tag], dtype, '%s %s %s' % (name, tag, entry))
        pp = PickParameters(type('D', (), dict(dt=float(g['dt']), snum=data.shape[0]))())
        pp.pol = prm[3]
        out = picklib.pick(data[:, t0:t0 + n], int(g['snum_start']), int(g['snum_end']), pp)
        assert_picks(out, g['out' + tag], dtype, '%s %s picklib.pick' % (name, tag))


def test_packet_sweep_single_traces(hip):
    """2000 random packets through impdar_pick_guided with n = 1: every outcome of the packet rule."""
    g = golden('PK20_sweep')
    codes = g['codes']
    assert np.mean(codes == 0) >= 0.40
    for dtype, tag in DTYPES:
        got = np.full((len(codes), 5), np.nan)
        for k in range(len(codes)):
            x = np.ascontiguousarray(g['traces'][k, :g['lens'][k]].astype(dtype)[:, None])
            prm = tuple(int(v) for v in g['prms'][k]) + (int(g['pols'][k]),)
            for entry, where in entries(hip, x):
                out, status = raw_guided(hip, where, 0, [g['mids'][k]], prm)
                assert status.tolist() == [codes[k], -1 if codes[k] == 0 else 0], (k, entry)
                assert codes[k] == 0 or np.all(np.isnan(out)), (k, entry)
                assert entry == 'host' or np.array_equal(out[:, 0], got[k], equal_nan=True), k
                got[k] = out[:, 0]
        assert_picks(got.T, g['out' + tag].T, dtype, 'sweep n = 1 ' + tag)


def test_packet_sweep_lines(hip):
    """The same rule with n = 63 / 64 / 65 traces per call: lanes beyond n, a second workgroup of one trace."""
    g = golden('PK21_sweep_lines')
    for dtype, tag in DTYPES:
        for k in range(len(g['n'])):
            n, snum = int(g['n'][k]), int(g['snum'][k])
            data = np.ascontiguousarray(g['data'][k, :snum, :n].astype(dtype))
            prm = tuple(int(v) for v in g['prms'][k]) + (int(g['pols'][k]),)
            for entry, where in entries(hip, data):
                out, status = raw_guided(hip, where, 0, g['mids'][k, :n], prm)
                bad = np.flatnonzero(g['codes'][k, :n])
                want = [0, -1] if bad.size == 0 else [g['codes'][k, bad[0]], bad[0]]
                assert status.tolist() == want, (k, entry)
                assert_picks(out, g['out' + tag][k, :, :n], dtype, 'line %d %s %s' % (k, tag, entry))


@pytest.mark.parametrize('name', CONT)
def test_continuity_index_reproduces_the_reference(hip, name):
    g = golden(name)
    for ratio, s, b, k in continuity_runs(g):
        for dtype, tag in DTYPES:
            data = np.ascontiguousarray(g['data'].astype(dtype))
            for entry, where in entries(hip, data):
                fn = picking.continuity_host if entry == 'host' else picking.continuity_dev
                assert_continuity(fn(where, s, b, ratio), g['out%s_%d' % (tag, k)], data, s, b, ratio,
                                  '%s %s %s %s' % (name, ratio, tag, entry))


def test_continuity_index_method_resident_and_host(hip):
    g = golden('PK41_continuity_wide_s')
    for resident in (False, True):
        dat = RadarData(SAVED)
        dat.data = g['data'].copy()
        dat.snum, dat.tnum = dat.data.shape
        dat.picks = Picks(dat)
        dat.picks.samp1 = np.vstack((g['spick'], g['bpick']))
        if resident:
            dat.to_device()
        s, b = picking.continuity_bounds(g['spick'], g['bpick'], dat.snum)
        assert_continuity(dat.continuity_index(1, 0, cutoff_ratio=0.1), g['out32_1'], g['data'], s, b, 0.1, 'method')
        assert dat.continuity_index_.shape == (dat.tnum,)


def test_failing_pick_leaves_the_picks_unchanged(hip):
    g = golden('PK11_bottom')
    for resident in (False, True):
        dat = RadarData(SAVED)
        dat.data = g['data'].copy()
        dat._picks_struct = None
        if resident:
            dat.to_device()
        with pytest.raises(ValueError) as e:
            dat.pick_layers(g['snums'], g['tnums'], freq=4)
        assert str(e.value) == str(g['message']) and dat.picks is None


def chain(resident, fn):
    dat = RadarData(SAVED)
    if resident:
        dat.to_device()
    dat.vertical_band_pass(1., 20.)
    out = dat.pick_layers([30, 35], [0, 35], freq=4, pol=1)
    assert (dat._dev is not None) == resident            # picking leaves the radargram where it is
    dat.save(fn)
    return out


def test_round_trip_resident_chain_equals_the_host_chain(hip, tmp_path):
    from scipy.io import loadmat
    fns = [str(tmp_path / n) for n in ('host.mat', 'resident.mat')]
    outs = [chain(resident, fn) for resident, fn in zip((False, True), fns)]
    assert np.array_equal(outs[0], outs[1], equal_nan=True) and not np.any(np.isnan(outs[0][:, :3]))
    a, b = (loadmat(fn) for fn in fns)
    assert np.array_equal(a['data'], b['data'])
    for f in ('samp1', 'samp2', 'samp3', 'time', 'power', 'picknums'):
        assert np.array_equal(a['picks'][f][0][0], b['picks'][f][0][0], equal_nan=True), f
    back = RadarData(fns[1])
    picks = Picks(back, back._picks_struct)
    assert picks.picknums == [1, 2, 3, 4] and np.array_equal(picks.samp2[2:], outs[1][:, 1])
    with pytest.raises(NotImplementedError):
        back.reverse()                                     # picking is the last step of a chain


def test_impproc_autopick_writes_a_picked_file(hip, tmp_path):
    import sys
    from unittest.mock import patch
    from impdar_amd.bin import impproc
    out = str(tmp_path / 'picked.mat')
    with patch.object(sys, 'argv', ['impproc', 'autopick', SAVED, '--snums', '50', '60', '--tnums', '69', '0', '--pol', '1',
                                    '-o', out]):
        impproc.main()
    back = RadarData(out)
    picks = Picks(back, back._picks_struct)
    want = golden('PK01_basic_pos')['out32'][2:4]
    got = np.stack([picks.samp1[2:], picks.samp2[2:], picks.samp3[2:], picks.time[2:], picks.power[2:]], axis=1)
    assert picks.picknums == [1, 2, 3, 4]
    assert_picks(got, want, np.float32, 'impproc autopick')
    assert os.path.getsize(out) > 0 and os.path.dirname(SAVED) == GOLDEN
