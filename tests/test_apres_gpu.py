"""ApRES range conversion, stacking and phase difference on the GPU: every ``AP_*`` fixture through the Python functions
at the bars of ``test_apres_cpu.py`` (spec, data: E = 64 u log2(N) ||reference spectrum of the chirp||_2 per kept bin;
Rfine: |diff| |den_k| <= E / |data_k| + 8 u for every bin; stacking bit for bit; co 4 W u with NaN positions equal);
both phase-difference kernels on either side of their threshold; the resident chain against the two calls, the chunk
size, the resident entries against the host-buffer ones, bit for bit; the ABI's refusals; the hand-over to
``quadpol.rotational_transform``."""
import copy

import numpy as np
import pytest

import apres_ref as ref
from conftest import golden
from impdar_amd import apres as apm
from impdar_amd import quadpol as qpm
from test_apres_cpu import (DIFF, RANGE, STACK, check_diff, check_range, check_stack, diff_holder, holder, range_args,
                            run_range, same_bits, stack_holder)

pytestmark = pytest.mark.gpu

A1, A5 = RANGE[0], RANGE[4]


@pytest.fixture(scope='module')
def a1(hip):
    """A1's tables, chirps and the three products of the host-buffer entry at the library's own chunk size."""
    g = golden(A1)
    t = apm.range_tables(holder(g), *range_args(g))
    raw = apm.raw_rows(holder(g))
    return g, t, raw, apm.range_host(raw, t)


@pytest.mark.parametrize('name', RANGE)
def test_range_matches_the_reference(hip, name):
    g = golden(name)
    check_range(run_range(g), g)


@pytest.mark.parametrize('name', STACK)
def test_stacking_matches_the_reference_bit_for_bit(hip, name):
    g = golden(name)
    dat, num_chirps = stack_holder(g)
    apm.stacking(dat, num_chirps)
    check_stack(dat, g)


@pytest.mark.parametrize('name', DIFF)
def test_phase_diff_matches_the_reference(hip, name):
    g = golden(name)
    diff, win, step, range_ext = diff_holder(g)
    apm.phase_diff(diff, win, step, range_ext=range_ext)
    check_diff(diff, g)


@pytest.mark.parametrize('win,step', [(64, 3), (65, 3), (66, 3), (67, 1), (200, 7), (713, 1), (714, 1), (1, 50)])
def test_phase_diff_on_both_sides_of_the_wavefront_threshold(hip, win, step):
    """A thread sums a window of up to 64 terms, a wavefront a longer one: 64 and 65 (64 terms), 66 (66 terms), a
    window of several strides per lane, one that leaves a single window, one that leaves none, one without terms."""
    g = golden(DIFF[2])                                   # the vectors with a run of zeros: NaN windows up to 60 terms
    got = apm.phase_diff_host(g['data'], g['data2'], win, step)
    want = ref.phase_diff(g['data'], g['data2'], win, step)
    assert got.shape == want.shape == (len(apm.phase_diff_windows(714, win, step)),)
    nan = np.isnan(want.real)
    np.testing.assert_array_equal(np.isnan(got.real), nan)
    np.testing.assert_array_equal(np.isnan(got.imag), nan)
    if (~nan).any():
        assert float(np.max(np.abs(got[~nan] - want[~nan]))) <= 4 * 2 * (win // 2) * ref.U
    assert nan.all() if win == 1 else True


def test_first_order_fine_range(hip, a1):
    """A header without a chirp gradient: phase2range's first-order branch, lambdac phi / (4 pi), on the device."""
    g, t, raw, (spec, data, rfine) = a1
    dat = holder(g)
    dat.header.chirp_grad = 0.
    t1 = apm.range_tables(dat, *range_args(g))
    assert t1.first_order
    apm.apres_range(dat, *range_args(g))
    t_all = copy.copy(t1)
    t_all.n = t1.nf
    mag = np.abs(ref.range_rows(raw, t_all)[1]).reshape(2, 3, 1001)
    want = ref.range_rows(raw, t1)[2].reshape(2, 3, 1001)
    bar = ref.spectrum_bar(2002, g['spec_norm']).reshape(2, 3, 1) / mag + 8 * ref.U
    assert (np.abs(dat.Rfine - want) * (4. * np.pi / t1.lambdac) <= bar).all()
    assert same_bits(dat.spec, spec.reshape(2, 3, 714))          # phiref without the gradient changes data, not spec


@pytest.mark.parametrize('name,num_chirps', [(A1, None), (A1, 3), (A1, 4), (A5, None), (RANGE[5], 2)])
def test_chain_equals_the_two_calls_bit_for_bit(hip, name, num_chirps):
    g = golden(name)
    want = run_range(g)
    kept = {k: getattr(want, k) for k in ('spec', 'Rcoarse', 'Rfine', 'phiref', 'snum', 'data_dtype')}
    apm.stacking(want, num_chirps)
    dat = holder(g)
    apm.chain(dat, *range_args(g), num_chirps=num_chirps)
    for k in ('spec', 'Rcoarse', 'Rfine', 'phiref'):
        assert same_bits(getattr(dat, k), kept[k]), k
    assert same_bits(dat.data, want.data)
    assert (dat.snum, dat.bnum, dat.cnum, dat.data_dtype) == (want.snum, want.bnum, want.cnum, kept['data_dtype'])
    assert dat.flags.range == want.flags.range and dat.flags.stack == want.flags.stack


@pytest.mark.parametrize('chunk', [1, 4, 6, 100])
def test_chunk_size_changes_no_bit(hip, a1, chunk):
    """One chirp at a time, four with a tail of two, all six, more than there are."""
    g, t, raw, want = a1
    got = apm.range_host(raw, t, chunk=chunk)
    for a, b, k in zip(got, want, ('spec', 'data', 'Rfine')):
        assert same_bits(a, b), k


def test_resident_entries_back_to_back_equal_the_host_buffer_entries(hip, a1):
    """``*_dev`` range conversion, stacking of its data and phase difference of two stacks with no host
    synchronisation in between: the stream orders them."""
    g, t, raw, (spec, data, rfine) = a1
    ctx = hip.context()
    d_raw = hip.DeviceArray.from_host(ctx, raw)
    d_spec, d_data, d_rfine = apm.range_dev(d_raw, t)
    d_all = apm.stack_dev(d_data, 1, 6)
    d_burst = apm.stack_dev(d_data, 2, 3)
    d_first = apm.stack_dev(d_data, 1, 3)
    d_all.shape, d_first.shape = (714,), (714,)
    d_co = apm.phase_diff_dev(d_all, d_first, 20, 7)
    assert same_bits(d_spec.to_host(), spec) and same_bits(d_data.to_host(), data) and same_bits(d_rfine.to_host(), rfine)
    assert same_bits(d_burst.to_host(), apm.stack_host(data, 2, 3))
    s_all, s_first = apm.stack_host(data, 1, 6)[0], apm.stack_host(data, 1, 3)[0]
    assert same_bits(d_all.to_host(), s_all) and same_bits(d_first.to_host(), s_first)
    assert same_bits(d_co.to_host(), apm.phase_diff_host(s_all, s_first, 20, 7))
    assert same_bits(apm.stack_host(raw, 2, 3), ref.stack(raw, 2, 3))
    prep, fft, post = apm.range_last_ms(ctx)
    assert prep > 0 and fft > 0 and post > 0
    for d in (d_raw, d_spec, d_data, d_rfine, d_all, d_burst, d_first, d_co):
        d.free()


def test_the_abi_refuses_before_any_device_work(hip, a1):
    g, t, raw, _ = a1
    lib, ctx = hip.load(), hip.context()
    sentinel = -7.25
    spec, data = np.full((6, 714), sentinel + 0j), np.full((6, 714), sentinel + 0j)
    rfine = np.full((6, 1001), sentinel)
    args, keep = apm._range_args(t, 0)

    def call(rows=6, snum=1001, p=2, n=714, win=args[2], comp=args[3], den=args[4], chunk=0):
        return lib.impdar_apres_range(ctx, hip.as_dp(raw)[1], rows, snum, p, n, win, comp, den, args[5], args[6], 0, 0., chunk,
                                      apm._cdp(spec), apm._cdp(data), hip.as_dp(rfine)[1])
    for kw, word in ((dict(snum=1), 'samples'), (dict(p=0), 'pad factor'), (dict(n=1002), 'bins kept'), (dict(n=-1), 'bins kept'),
                     (dict(win=None), 'null'), (dict(den=None), 'null'), (dict(rows=0), 'chirps'), (dict(chunk=-1), 'chunk')):
        assert call(**kw) == hip.ERR_ARG, kw
        assert 'impdar_apres_range' in hip.last_error() and word in hip.last_error(), (kw, hip.last_error())
    assert (spec == sentinel).all() and (data == sentinel).all() and (rfine == sentinel).all()
    with pytest.raises(ValueError):
        apm.stack_host(raw, 3, 3)                 # 9 chirps of 6
    with pytest.raises(ValueError):
        apm.stack_host(raw, 1, 0)
    ones, co = np.ones(30, dtype=complex), np.full(30, sentinel + 0j)
    for win, step in ((4, 0), (-2, 1)):
        assert lib.impdar_apres_phase_diff(ctx, apm._cdp(ones), apm._cdp(ones), 30, win, step, apm._cdp(co)) == hip.ERR_ARG
    assert (co == sentinel).all()
    assert len(apm.phase_diff_host(np.ones(30, dtype=complex), np.ones(30, dtype=complex), 40, 1)) == 0
    assert call() == 0                            # the same arguments unchanged go through
    assert (rfine != sentinel).all()


def test_converted_stacked_data_feeds_the_quadpol_rotation(hip):
    """The hand-over that the module exists for: a converted, stacked profile as the four measured vectors."""
    g = golden(A1)
    profiles = []
    for scale in (1., 0.05 + 0.02j, 0.05 + 0.021j, 0.8 - 0.1j):
        dat = holder(g)
        apm.chain(dat, *range_args(g))
        profiles.append((dat, scale * np.squeeze(dat.data)))
    qp = qpm.QuadPol()
    qp.shh, qp.shv, qp.svh, qp.svv = [v for _, v in profiles]
    qp.range = profiles[0][0].Rcoarse
    qp.snum = profiles[0][0].snum
    qp.flags.cpe = False
    qpm.rotational_transform(qp, n_thetas=9)
    assert qp.HH.shape == (714, 9) and qp.HH.dtype == np.complex128
    assert np.isfinite(qp.HH.view(np.float64)).all() and np.isfinite(qp.VV.view(np.float64)).all()
    np.testing.assert_array_equal(qp.flags.rotation, [1, 9])
