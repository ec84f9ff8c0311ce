"""Layer picking without a GPU: the NumPy restatement of ``csrc/pick.hip`` (``tests/picking_ref.py``) reproduces every
``PK*`` fixture of the reference -- pick rows bit for bit, power within 2 (n + 2) u p, the continuity index within
16 u max(1, max|P|), error kinds, messages and places -- the pick data model round-trips the file the reference's
``save()`` wrote, ``PickParameters.freq_update`` gives the reference's window sizes, and the wrappers, the
``RadarData`` methods and ``impproc autopick`` do their bookkeeping with the device calls replaced by the restatement.
"""
import contextlib
import os
import sys
from unittest.mock import patch

import numpy as np
import pytest
from scipy.io import loadmat

import picking_ref as ref
from picking_ref import assert_continuity, assert_picks, continuity_runs, prm_of
from conftest import GOLDEN, ROOT, golden, golden_names
from impdar_amd import picking
from impdar_amd.bin import impproc
from impdar_amd.lib import picklib
from impdar_amd.lib.PickParameters import PickParameters
from impdar_amd.lib.Picks import Picks
from impdar_amd.lib.RadarData import RadarData

SAVED = os.path.join(GOLDEN, 'PK_ref_saved_picked.mat')
DTYPES = [(np.float32, '32'), (np.float64, '64')]
AUTO = [n for n in golden_names('PK') if n[2:4] < '20']
GUIDED = golden_names('PK3')
CONT = golden_names('PK4')


# ---------------------------------------------------------------------------- the restatement against the reference
@pytest.mark.parametrize('name', AUTO)
def test_restatement_reproduces_the_reference_chains(name):
    g = golden(name)
    assert str(g['kind']) == 'auto'
    for dtype, tag in DTYPES:
        out, (code, seed, trace) = ref.auto_pick(g['data'].astype(dtype), g['snums'], g['tnums'], *prm_of(g))
        assert code == int(g['code'])
        if code == 0:
            assert_picks(out, g['out' + tag], dtype, name + tag)
        else:
            assert picking.MESSAGES[code] == str(g['message'])
            assert (seed, trace) == (int(g['fail_seed']), int(g['fail_trace']))
        if 'partial' + tag in g:
            for k in range(len(g['snums'])):
                one, (c, _, j) = ref.auto_pick(g['data'].astype(dtype), g['snums'][k:k + 1], g['tnums'][k:k + 1], *prm_of(g))
                assert (c, j) == (int(g['seed_codes'][k]), int(g['seed_traces'][k]))
                assert_picks(one[0], g['partial' + tag][k], dtype, '%s%s seed %d' % (name, tag, k))


def test_fixture_outcomes_cover_every_kind():
    kinds = sorted(set(str(golden(n)['expect']) for n in AUTO))
    assert kinds == ['argmax', 'argmin', 'picks', 'short']
    assert sum(str(golden(n)['expect']) == 'picks' for n in AUTO) >= 9


@pytest.mark.parametrize('name', GUIDED)
def test_restatement_reproduces_the_reference_guided_picks(name):
    g = golden(name)
    mid = picking.midpoints(int(g['n']), int(g['snum_start']), int(g['snum_end']))
    assert np.array_equal(mid, g['mid'])
    for dtype, tag in DTYPES:
        out, first = ref.pick_guided(g['data'].astype(dtype), int(g['t0']), mid, *prm_of(g))
        assert first == (0, -1)
        assert_picks(out, g['out' + tag], dtype, name + tag)


def test_restatement_reproduces_the_packet_sweep():
    g = golden('PK20_sweep')
    assert np.mean(g['codes'] == 0) >= 0.40
    assert set(np.unique(g['codes'])) == {0, 1, 2, 3}
    for dtype, tag in DTYPES:
        got = np.full((len(g['codes']), 5), np.nan)
        for k in range(len(g['codes'])):
            x = g['traces'][k, :g['lens'][k]].astype(dtype)
            code, pk = ref.packet_pick(x, int(g['mids'][k]), *[int(v) for v in g['prms'][k]], int(g['pols'][k]))
            assert code == g['codes'][k], k
            if code == 0:
                got[k] = pk
        assert_picks(got.T, g['out' + tag].T, dtype, 'sweep' + tag)


def test_restatement_reproduces_the_sweep_lines():
    g = golden('PK21_sweep_lines')
    for dtype, tag in DTYPES:
        for k in range(len(g['n'])):
            n, snum = int(g['n'][k]), int(g['snum'][k])
            out, _ = ref.pick_guided(g['data'][k, :snum, :n].astype(dtype), 0, g['mids'][k, :n], *[int(v) for v in g['prms'][k]],
                                     int(g['pols'][k]))
            assert np.array_equal(np.isnan(out[0]), g['codes'][k, :n] != 0)
            assert_picks(out, g['out' + tag][k, :, :n], dtype, 'line %d %s' % (k, tag))


@pytest.mark.parametrize('name', CONT)
def test_restatement_reproduces_the_continuity_index(name):
    g = golden(name)
    assert float(g['ref32_vs_ref64_over_bar']) <= 0.5     # the reference's own rounding leaves the bar where it is
    some = False
    for ratio, s, b, k in continuity_runs(g):
        for dtype, tag in DTYPES:
            data = g['data'].astype(dtype)
            want = g['out%s_%d' % (tag, k)]
            assert_continuity(ref.continuity(data, s, b, ratio), want, data, s, b, ratio, '%s %s %s' % (name, ratio, tag))
            if ratio == 0.001:
                assert np.all(np.isnan(want))              # cut == 0 leaves nothing
            some = some or np.any(~np.isnan(want))
        if ratio is None:
            want = g['out64_%d' % k]
            assert np.isnan(want[3]) and np.isnan(want[7]) and np.isnan(want[9]) and not np.isnan(want[10])
    assert some


# -------------------------------------------------------------------------------------------------- the data model
def test_freq_update_gives_the_reference_windows():
    class D(object):
        dt, snum = 1.0e-8, 4096
    pp = PickParameters(D())
    assert (pp.freq, pp.plength, pp.FWW, pp.scst, pp.pol) == (4, 49, 17, 16, 1)
    want = {50: (3, 1, 1), 34: (5, 3, 1), 25: (7, 3, 2), 4: (49, 17, 16), 1: (199, 67, 66), 0.1: (1999, 667, 666)}
    for freq, prm in want.items():
        pp.freq_update(freq)
        assert (pp.plength, pp.FWW, pp.scst) == prm == ref.freq_params(freq, D.dt, D.snum), freq
    D.snum = 96                      # the clamp: plength to snum, FWW to half of it made odd, scst as it was
    pp.freq_update(1)
    assert (pp.plength, pp.FWW, pp.scst) == (96, 49, 66) == ref.freq_params(1, D.dt, 96)
    assert set(pp.to_struct()) == set(PickParameters.attrs)


def test_freq_update_matches_every_fixture():
    for name in AUTO + GUIDED:
        if name in ('PK16_staged_190', 'PK17_direct_191'):      # window sizes set by hand, either side of the LDS limit
            continue
        g = golden(name)
        assert ref.freq_params(float(g['freq']), float(g['dt']), g['data'].shape[0]) == prm_of(g)[:3], name


def struct_fields(s):
    return sorted(s.dtype.names)


def test_picks_round_trip_the_file_the_reference_saved(tmp_path):
    dat = RadarData(SAVED)
    assert dat.picks is None and dat._picks_struct is not None         # loading does not change
    picks = Picks(dat, dat._picks_struct)
    assert picks.picknums == [1, 2] and picks.samp1.shape == (2, dat.tnum)
    assert (picks.pickparams.plength, picks.pickparams.FWW, picks.pickparams.scst) == (49, 17, 16)
    assert str(picks).startswith('Pick object with 2 picks:')
    dat.picks = picks
    out = str(tmp_path / 'again.mat')
    dat.save(out)
    a, b = loadmat(SAVED)['picks'], loadmat(out)['picks']
    assert struct_fields(a) == struct_fields(b)
    for sub in ('pickparams', 'lasttrace', 'lt'):
        sa, sb = a[sub][0][0], b[sub][0][0]
        assert struct_fields(sa) == struct_fields(sb), sub
        for f in sa.dtype.names:
            assert sa[f][0][0].shape == sb[f][0][0].shape, (sub, f)
    assert struct_fields(a['lt'][0][0]['crop'][0][0]) == struct_fields(b['lt'][0][0]['crop'][0][0])
    for f in ('samp1', 'samp2', 'samp3', 'time', 'power', 'picknums'):
        assert a[f][0][0].shape == b[f][0][0].shape, f
        assert np.array_equal(a[f][0][0], b[f][0][0], equal_nan=True), f
    again = RadarData(out)
    back = Picks(again, again._picks_struct)
    assert np.array_equal(back.samp2, picks.samp2) and back.picknums == [1, 2]


def test_blank_picks_add_and_update():
    dat = RadarData(SAVED)
    picks = Picks(dat)
    assert str(picks) == 'Empty pick object' and picks.to_struct()['samp1'] == 0
    assert picks.add_pick(3) == 1 and picks.picknums == [3] and np.all(np.isnan(picks.samp1))
    assert picks.add_pick(4) == 1 and picks.picknums == [4]            # a blank last pick is re-used
    info = np.arange(5 * dat.tnum, dtype=np.float64).reshape(5, dat.tnum)
    picks.update_pick(4, info)
    assert picks.add_pick(5) == 2 and picks.lasttrace.snum == [-9999, -9999]
    with pytest.raises(ValueError, match='We already have that pick'):
        picks.update_pick(5, info)
        picks.add_pick(4)
    with pytest.raises(ValueError, match='not a pick'):
        picks.update_pick(9, info)
    with pytest.raises(ValueError, match='5xtnum'):
        picks.update_pick(5, info[:, :-1])
    assert np.array_equal(picks.power[0], info[4])
    for gone in ('reverse', 'hcrop', 'crop', 'restack', 'smooth'):
        assert not hasattr(picks, gone)


# ------------------------------------------------------------------- wrappers, methods, CLI with patched device calls
def np_auto_pick(data, snums, tnums, plength, FWW, scst, pol):
    data = np.asarray(data)
    s, t = picking.check_seeds(snums, tnums, data.shape[1])
    out, (code, _, _) = ref.auto_pick(data, s, t, plength, FWW, scst, pol)
    picking.raise_outcome(code)
    return out


def np_pick(data, t0, mid, plength, FWW, scst, pol):
    out, (code, _) = ref.pick_guided(np.asarray(data), t0, np.asarray(mid), plength, FWW, scst, pol)
    picking.raise_outcome(code)
    return out


def np_continuity(data, s, b, cutoff_ratio=None):
    return ref.continuity(np.asarray(data), s, b, cutoff_ratio)


@contextlib.contextmanager
def kernels_in_numpy():
    with patch.object(picking, 'auto_pick_host', np_auto_pick), patch.object(picking, 'pick_host', np_pick), \
            patch.object(picking, 'continuity_host', np_continuity):
        yield


def test_seed_checks():
    with pytest.raises(ValueError, match='^Snum and tnum must be of equal length$'):
        picking.check_seeds([1, 2], [0], 70)
    with pytest.raises(IndexError):
        picking.check_seeds([30], [70], 70)
    for s, t in (([-1], [0]), ([30], [-1])):      # the documented divergence
        with pytest.raises(ValueError, match='negative'):
            picking.check_seeds(s, t, 70)
    with pytest.raises(ValueError, match='whole'):
        picking.check_seeds([30.5], [0], 70)
    s, t = picking.check_seeds([30., 31], np.array([0, 69]), 70)
    assert s.dtype == t.dtype == np.int32 and s.tolist() == [30, 31] and t.tolist() == [0, 69]


def test_outcome_messages_are_the_reference_texts():
    assert picking.SHORT_MESSAGE == str(golden('PK11_bottom')['message'])
    assert picking.MESSAGES[picking.EMPTY_ARGMIN] == str(golden('PK05_smallest_f34')['message'])
    assert picking.MESSAGES[picking.EMPTY_ARGMAX] == str(golden('PK06_smallest_f50')['message'])
    picking.raise_outcome(0)
    for code in (1, 2, 3):
        with pytest.raises(ValueError) as e:
            picking.raise_outcome(code)
        assert str(e.value) == picking.MESSAGES[code]


def test_midpoint_and_bounds():
    assert np.array_equal(picklib._midpoint(4, 10, 20), [10, 12, 15, 18])
    assert np.array_equal(picklib._midpoint(3, -9999, 7), [7, 7, 7])
    s, b = picking.continuity_bounds([0, 5, np.nan, -3, 2], [10, 200, 4, 50, np.nan], 96)
    assert s.tolist() == [0, 5, -1, 93, -1] and b.tolist() == [10, 96, -1, 50, -1]


def test_picklib_has_the_reference_signatures():
    g = golden('PK30_guided_line')
    dat = RadarData(SAVED)
    pp = PickParameters(dat)
    with kernels_in_numpy():
        out = picklib.pick(g['data'], int(g['snum_start']), int(g['snum_end']), pp)
        assert_picks(out, g['out32'], np.float32, 'picklib.pick')
        one = picklib.packet_pick(g['data'][:, 5], pp, g['mid'][5])
        assert isinstance(one, list) and one[:3] == g['out32'][:3, 5].tolist() and np.isnan(one[3])
        with pytest.raises(ValueError, match='single, flat trace'):
            picklib.packet_pick(g['data'], pp, 30)
    packet, top = picklib.packet_power(g['data'][:, 5], 49, 30)
    assert top == 5 and np.array_equal(packet, g['data'][5:54, 5])
    with pytest.raises(ValueError, match='single, flat trace'):
        picklib.packet_power(g['data'], 49, 30)


def test_pick_layers_bookkeeping_and_refusals(tmp_path):
    g = golden('PK01_basic_pos')
    dat = RadarData(SAVED)                       # carries picks 1 and 2 in its struct
    with kernels_in_numpy():
        out = dat.pick_layers([50, 60], [69, 0], pol=1)
        assert dat.picks.picknums == [1, 2, 3, 4]            # the defaults continue from the largest present
        assert_picks(out, g['out32'][2:4], np.float32, 'pick_layers')
        assert np.array_equal(dat.picks.samp2[2:], out[:, 1]) and np.array_equal(dat.picks.power[3], out[1, 4])
        before = dat.picks.samp1.copy()
        with pytest.raises(ValueError, match='We already have that pick'):
            dat.pick_layers([30], [0], picknums=[2])
        with pytest.raises(ValueError) as e:                  # a failing pick leaves the picks as they were
            dat.pick_layers([30], [10], freq=50)
        assert str(e.value) == picking.MESSAGES[picking.EMPTY_ARGMAX]
        assert np.array_equal(dat.picks.samp1, before, equal_nan=True) and dat.picks.pickparams.freq == 4
        assert dat.picks.pickparams.plength == 49
    for step in (dat.reverse, lambda: dat.hcrop(3), lambda: dat.restack(3), lambda: dat.constant_space(1.)):
        with pytest.raises(NotImplementedError):
            step()
    fn = str(tmp_path / 'picked.mat')
    dat.save(fn)
    again = RadarData(fn)
    assert again.picks is None
    back = Picks(again, again._picks_struct)
    assert back.picknums == [1, 2, 3, 4] and np.array_equal(back.samp3, dat.picks.samp3)

    fresh = RadarData(SAVED)
    fresh._picks_struct = None
    with kernels_in_numpy():
        fresh.pick_layers([30, 35], [0, 35], freq=4)
        assert fresh.picks.picknums == [1, 2]
        with pytest.raises(ValueError, match='^Snum and tnum must be of equal length$'):
            fresh.pick_layers([30, 35], [0])
        nothing = RadarData(SAVED)
        nothing._picks_struct = None
        with pytest.raises(ValueError):
            nothing.pick_layers([30], [10], freq=50)
        assert nothing.picks is None                          # nothing was written


def test_continuity_index_method_sets_its_own_attribute():
    g = golden('PK40_continuity_small_s')
    dat = RadarData(SAVED)
    dat.data = g['data']
    dat.picks = Picks(dat)
    dat.picks.samp1 = np.vstack((g['spick'], g['bpick']))
    with kernels_in_numpy():
        out = dat.continuity_index(1, 0)
        assert out is dat.continuity_index_ and callable(dat.continuity_index)
        s, b = picking.continuity_bounds(g['spick'], g['bpick'], 96)
        assert_continuity(out, g['out32_0'], g['data'], s, b, None, 'method')
        dat.continuity_index(1, cutoff_ratio=0.001)
        assert np.all(np.isnan(dat.continuity_index_))


def test_impproc_autopick_forwards_its_arguments(tmp_path):
    out = str(tmp_path / 'line_picked.mat')
    argv = ['impproc', 'autopick', SAVED, '--snums', '50', '60', '--tnums', '69', '0', '--freq', '4', '--pol', '1',
            '--picknums', '7', '9', '-o', out]
    with patch.object(sys, 'argv', argv), kernels_in_numpy():
        impproc.main()
    again = RadarData(out)
    picks = Picks(again, again._picks_struct)
    assert picks.picknums == [1, 2, 7, 9]
    assert_picks(np.stack([picks.samp1[2:], picks.samp2[2:], picks.samp3[2:], picks.time[2:], picks.power[2:]], axis=1),
                 golden('PK01_basic_pos')['out32'][2:4], np.float32, 'impproc autopick')

    seen = {}
    args = impproc._get_args().parse_args(['autopick', 'a_raw.mat', '--snums', '3', '--tnums', '4'])
    assert args.name == 'picked' and args.freq is None and args.pol is None and args.picknums is None

    class Spy(object):
        def pick_layers(self, snums, tnums, **kw):
            seen.update(snums=snums, tnums=tnums, **kw)
    args.func(Spy(), **vars(args))
    assert seen == dict(snums=[3], tnums=[4], picknums=None, freq=None, pol=None)


def test_abi_declares_and_binds_the_picking_entry_points():
    from impdar_amd import _hip, build
    header = open(os.path.join(ROOT, 'include', 'impdar_hip.h')).read()
    for name in ('impdar_auto_pick', 'impdar_pick_guided', 'impdar_continuity'):
        for form in (name, name + '_dev'):
            assert form + '(' in header and form in _hip.SIGNATURES
    assert 'pick.hip' in build.SOURCES
