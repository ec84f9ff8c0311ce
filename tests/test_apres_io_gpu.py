"""The decode of an ApRES burst's counts on the GPU, and the flow through files.

Decode: bit for bit NumPy's ``counts.astype(float) * 2.5 / 2**16.`` (``/ divisor``), on the host-buffer and the
resident entry, uint16 and uint32, divisors 1, 2 and 6, at lengths that are a head only, a tail only, one vector with
and without a tail, and an odd total of several upload pieces (the piece forced small with the resident entry's ``piece`` argument); with the
counts at an odd address; into every alignment of the output, with the elements around it untouched.

Flow: two synthetic ``.DAT`` files of 6 x 1001 through ``load_apres`` / ``apdar``, held to ``AI_F1_flow`` (the
reference's load, ``apres_range(2, 4000)``, ``stacking``, ``phase_uncertainty``) at the bars of ``test_apres_cpu.py``:
  spec, data, Rfine   ``check_range`` as it stands
  stacked profile     |diff| <= Es = the mean over the stacked chirps of their bars E, plus 4 u |stacked|
  uncertainty         x = M sin(angle(m) - angle(noise)) / |m| with the median magnitude M below the bed: |d angle| and
                      |d |m|| / |m| are at most Es / |m|, and |d M| <= Es (a median moves no more than its elements), so
                      |d x| <= (Es / |m|) (1 + 2 M / |m|) to first order (Es / |m| < 1e-8 here); that, plus the 32 u of the host steps
                      (``test_apres_flows_cpu.py``), on sin(uncertainty) = |x|; NaN (|x| > 1) positions equal where |x|
                      is further than the bar from 1
The counts route and the float64 route of ``chain`` leave the same bits.

Pair and quad: ``apdar diffproc`` and ``apdar qpproc`` against ``AI_B1_diffproc`` / ``AI_B2_qpproc``, the reference's
``time_diff_processing`` and ``quadpol_processing`` on synthetic sites with a bed: on the files the reference saved at the
existing bars as they stand, on the outputs of ``apdar proc`` with the inputs' share added (``check_pair``,
``check_quad``)."""
import ctypes as C
import os

import numpy as np
import pytest

import apres_io_ref as io
import apres_ref as ref
from conftest import GOLDEN, golden
from impdar_amd import apres as apm
from impdar_amd.bin import apdar
from impdar_amd.lib.ApresData import ApresData, ApresQuadPol, ApresTimeDiff, load_apres
from test_apres_cpu import check_range, holder, same_bits
from test_apres_flows_cpu import wraps_of
from test_quadpol_cpu import chhvv_bar, rotation_bar

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LENGTHS = (0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4097, 3 * 40001)
KINDS = ('<u2', '<u4')
DIVISORS = (1, 2, 6)


def counts_of(n, dtype, seed=0):
    rng = np.random.RandomState(1000 + n + seed)
    top = 2**16 if dtype == '<u2' else 2**32
    c = rng.randint(0, top, size=n, dtype=np.uint64).astype(dtype)
    for i, v in enumerate((0, 65535, top - 1)[:n]):
        c[(i * 5) % n] = v
    if n > 2:
        c[-1] = top - 1
    return c


SMALL = 1001                         # counts per upload piece (rounded up to 1008 by the library)


def both_entries(counts, divisor, piece=0):
    host = apm.decode_host(counts, divisor)
    d = apm.decode_dev(counts, divisor, piece=piece)
    try:
        dev = d.to_host() if d.nbytes else np.empty(d.shape)
    finally:
        d.free()
    return host, dev.reshape(counts.shape)


@pytest.mark.parametrize('n', LENGTHS)
def test_decode_is_numpys_bits(hip, n):
    for dtype in KINDS:
        counts = counts_of(n, dtype)
        for divisor in DIVISORS:
            want = io.decode(counts, divisor)
            host, dev = both_entries(counts, divisor)
            assert same_bits(host, want), (dtype, divisor)
            assert same_bits(dev, want), (dtype, divisor)


@pytest.mark.parametrize('n', (1007, 1008, 1009, 4097, 3 * 40001))
def test_decode_in_several_pieces(hip, n):
    for dtype in KINDS:
        counts = counts_of(n, dtype, seed=7)
        for divisor in (1, 6):
            host, dev = both_entries(counts, divisor, piece=SMALL)
            assert same_bits(host, io.decode(counts, divisor)) and same_bits(dev, host), (dtype, divisor)


def test_decode_takes_the_values_at_both_ends(hip):
    for dtype, top in (('<u2', 65535), ('<u4', 2**32 - 1)):
        counts = np.array([0, 1, top, top - 1, 65535, 32768] * 3, dtype=dtype)
        for divisor in DIVISORS:
            got = apm.decode_host(counts, divisor)
            assert same_bits(got, io.decode(counts, divisor))
            assert got[0] == 0. and got[2] == (float(top) * 2.5 / 65536.) / divisor


def test_decode_of_counts_at_an_odd_address(hip):
    """A 663-byte header puts a file's payload at an odd offset: the counts are uploaded from where they are."""
    n = 5000
    for dtype in KINDS:
        counts = counts_of(n, dtype, seed=3)
        image = np.zeros(663 + 2 + counts.nbytes, dtype=np.uint8)
        offset = 663 + (image.ctypes.data + 663 + 1) % 2            # the next odd address from byte 663 on
        image[offset:offset + counts.nbytes] = np.frombuffer(counts.tobytes(), dtype=np.uint8)
        view = np.frombuffer(image, dtype=dtype, count=n, offset=offset)
        assert view.ctypes.data % 2 == 1
        host, dev = both_entries(view, 6, piece=SMALL)
        assert same_bits(host, io.decode(counts, 6)) and same_bits(dev, host)


@pytest.mark.parametrize('dtype', KINDS)
def test_decode_into_every_output_alignment_touches_nothing_else(hip, dtype):
    """The resident entry with the output 1 ... 7 elements past a 64-byte boundary (a scalar head), lengths around
    the head and one vector: the decoded run is NumPy's, the guard elements before and after it keep their bits."""
    lib, ctx = hip.load(), hip.context()
    guard = -123.456
    for n in (1, 5, 7, 8, 9, 16, 23, 1030):
        counts = counts_of(n, dtype, seed=n)
        want = io.decode(counts, 6)
        for off in range(0, 8):
            d = hip.DeviceArray.from_host(ctx, np.full(n + 16, guard))
            try:
                rc = lib.impdar_apres_decode_dev(ctx, counts.ctypes.data_as(C.c_void_p), KINDS.index(dtype), n, 6.,
                                                 C.c_void_p(d.ptr.value + 8 * off))
                hip.check(rc, 'impdar_apres_decode_dev')
                got = d.to_host()
            finally:
                d.free()
            assert same_bits(got[off:off + n], want), (n, off)
            assert (got[:off] == guard).all() and (got[off + n:] == guard).all(), (n, off)


def test_decode_refusals(hip):
    lib, ctx = hip.load(), hip.context()
    counts = counts_of(16, '<u2')
    out = np.full(16, 7.)
    d = hip.DeviceArray.from_host(ctx, out)
    cp, op = counts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.POINTER(C.c_double))
    try:
        for args in ((cp, 0, -1, 1.), (cp, 2, 16, 1.), (cp, -1, 16, 1.), (None, 0, 16, 1.), (cp, 0, 16, 0.), (cp, 0, 16, -2.),
                     (cp, 0, 16, float('inf')), (cp, 0, 16, float('nan'))):
            assert lib.impdar_apres_decode(ctx, args[0], args[1], args[2], args[3], op) == hip.ERR_ARG, args
            assert 'impdar_apres_decode' in hip.last_error()
            assert lib.impdar_apres_decode_dev(ctx, args[0], args[1], args[2], args[3], d.ptr) == hip.ERR_ARG, args
        assert lib.impdar_apres_decode(ctx, cp, 0, 16, 1., None) == hip.ERR_ARG
        assert lib.impdar_apres_decode_dev(ctx, cp, 0, 16, 1., None) == hip.ERR_ARG
        assert lib.impdar_apres_decode_dev(ctx, cp, 0, 16, 1., C.c_void_p(d.ptr.value + 4)) == hip.ERR_ARG
        assert lib.impdar_apres_decode(None, cp, 0, 16, 1., op) == hip.ERR_ARG
        # nothing of the refused calls reached the output; an empty run succeeds, null pointers and all
        assert (out == 7.).all() and (d.to_host() == 7.).all()
        assert lib.impdar_apres_decode(ctx, None, 0, 0, 1., None) == 0
        assert lib.impdar_apres_decode_dev(ctx, None, 1, 0, 6., None) == 0
        assert lib.impdar_apres_decode_pieces_dev(ctx, cp, 0, 16, 1., d.ptr, -1) == hip.ERR_ARG
    finally:
        d.free()
    with pytest.raises(TypeError):
        apm.decode_host(np.zeros(4, dtype=np.int16))
    with pytest.raises(ValueError):
        apm.decode_dev(counts, shape=(3, 5))


def test_resident_decode_feeds_range_conversion(hip):
    """2 x 3 x 1001 with p = 2, the shape and header of ``AP_A1``: ``range_dev`` of the resident decode equals
    ``range_host`` of the rows decoded on the host, bit for bit."""
    g = golden('AP_A1_odd_snum_2x3x1001_p2')
    counts = io.chirp_counts(5, 6, 1001).reshape(2, 3, 1001)
    dat = holder(g, data=io.decode(counts))
    t = apm.range_tables(dat, 2, float(g['max_range']))
    want = apm.range_host(apm.raw_rows(dat), t)
    held = [apm.decode_dev(counts, shape=(6, 1001))]
    try:
        held.extend(apm.range_dev(held[0], t))
        assert same_bits(held[0].to_host(), io.decode(counts).reshape(6, 1001))
        for got, w in zip(held[1:], want):
            assert same_bits(got.to_host(), w)
    finally:
        for d in held:
            d.free()
    assert all(same_bits(a, b) for a, b in zip(apm.range_counts(counts, 1., t), want))


# ------------------------------------------------------------------------------------------------ the flow through files
def stacked_bar(g):
    N = int(g['p']) * g['raw'].shape[2]
    return float(np.mean(ref.spectrum_bar(N, g['spec_norm'])))


def test_loaded_files_convert_to_the_references_range_products(hip, tmp_path):
    g = golden('AI_F1_flow')
    dat = load_apres.load_apres(io.flow_files(str(tmp_path)))
    assert dat.raw_counts() is not None and same_bits(io.decode(dat.raw_counts()[0]), g['raw'])
    dat.apres_range(int(g['p']), float(g['max_range']))
    assert dat.raw_counts() is None
    check_range(dat, g)
    # the same bits from the float64 chirps
    again = holder(g)
    apm.apres_range(again, int(g['p']), float(g['max_range']))
    for k in ('spec', 'data', 'Rfine'):
        assert same_bits(getattr(dat, k), getattr(again, k)), k


def test_counts_route_and_float_route_of_chain_leave_the_same_bits(hip, tmp_path):
    fns = io.flow_files(str(tmp_path))
    a, b = load_apres.load_apres(fns), load_apres.load_apres(fns)
    b.data = b.data.copy()
    assert a.raw_counts() is not None and b.raw_counts() is None
    apm.chain(a, 2, 4000.)
    apm.chain(b, 2, 4000.)
    c = load_apres.load_apres(fns)
    d_raw = apm.decode_dev(c.raw_counts()[0], shape=(12, 1001))
    try:
        apm.chain(c, 2, 4000., d_raw=d_raw)
        assert same_bits(d_raw.to_host(), b_raw(fns))               # still there, still the caller's
    finally:
        d_raw.free()
    for k in ('data', 'spec', 'Rfine', 'Rcoarse', 'phiref'):
        assert same_bits(getattr(a, k), getattr(b, k)) and same_bits(getattr(c, k), getattr(b, k)), k
    assert a.data.shape == (1, 1, a.snum) and a.flags.stack == 12 == c.flags.stack and a.raw_counts() is None
    with pytest.raises(ValueError, match='d_raw is'):
        bad = apm.decode_dev(np.zeros(8, dtype='<u2'))
        try:
            apm.chain(load_apres.load_apres(fns), 2, 4000., d_raw=bad)
        finally:
            bad.free()


def b_raw(fns):
    return load_apres.load_apres(fns).data.reshape(12, 1001)


def test_apdar_load_and_proc_against_the_reference(hip, tmp_path):
    g = golden('AI_F1_flow')
    fns = io.flow_files(str(tmp_path))
    apdar.main(['load', '-acq_type', 'single'] + fns)
    raw = str(tmp_path / 'flow_0_apraw.mat')
    assert same_bits(ApresData(raw).data, g['raw'])
    np.random.seed(5)
    with np.errstate(invalid='ignore'):
        apdar.main(['proc', raw])
    proc = ApresData(str(tmp_path / 'flow_0_proc.mat'))
    want = g['stacked']
    assert proc.data.shape == want.shape and proc.data.dtype == np.complex128
    assert (proc.bnum, proc.cnum, proc.snum, proc.flags.stack, proc.flags.range) == (1, 1, int(g['snum']), 12, 4000.)
    assert same_bits(proc.Rcoarse, g['Rcoarse'])
    Es = stacked_bar(g)
    err = np.abs(proc.data - want)
    print('stacked: max |diff| / bar = %.3e' % float(np.max(err / (Es + 4 * U * np.abs(want)))))
    assert (err <= Es + 4 * U * np.abs(want)).all()
    # the same from the .DAT files directly (the counts route) as from the saved float64 chirps
    np.random.seed(5)
    with np.errstate(invalid='ignore'):
        apdar.main(['proc'] + fns + ['-o', str(tmp_path / 'direct.mat')])
    direct = ApresData(str(tmp_path / 'direct.mat'))
    assert same_bits(direct.data, proc.data) and same_bits(direct.uncertainty, proc.uncertainty)
    # uncertainty
    m = np.abs(np.squeeze(want))
    M = float(np.nanmedian(m[np.argwhere(g['Rcoarse'] > io.FLOW['noise_bed_range'])]))
    noise = M * (np.cos(g['noise_phase']) + 1j * np.sin(g['noise_phase']))
    x = M * np.sin(np.angle(np.squeeze(want)) - np.angle(noise)) / m
    bar = (Es / m) * (1. + 2. * M / m) + 32 * U
    got, ref_unc = proc.uncertainty, g['uncertainty']
    assert got.shape == ref_unc.shape and proc.flags.uncertainty
    assert (np.abs(np.abs(x) - 1.) > bar).all()                      # a condition on the fixture: no |x| within its bar of 1
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref_unc))
    ok = ~np.isnan(ref_unc)
    ratio = np.abs(np.sin(got[ok]) - np.sin(ref_unc[ok])) / bar[ok]
    print('uncertainty: max |sin diff| / bar = %.3e over %d of %d' % (float(ratio.max()), int(ok.sum()), ok.size))
    assert int(ok.sum()) == 323 and ratio.max() <= 1.                # every bin of the fixture that is no NaN


# ------------------------------------------------------------------------------------------------ pair and quad flows
def mat(name):
    return os.path.join(GOLDEN, 'AI_%s.mat' % name)


def check_pair(diff, g, moved=None):
    """The products of ``apdar diffproc`` against the reference's, at the bars of ``check_diff`` (co) and
    ``check_time_diff`` (phi and wraps, w, w_err, eps_zz, bed) as they stand; ``moved`` adds, per product, what its
    inputs' own distance from the reference's may move it by.  (``w0`` is not among the attributes a pair saves;
    ``w`` carries it.)"""
    moved = moved or {}
    win = int(g['win'])
    assert same_bits(diff.ds, g['ds']) and np.array_equal(diff.flags.phase_diff, g['flags_phase_diff'])
    bars = {'co': 4 * 2 * (win // 2) * U, 'phi': 8 * U * np.max(np.abs(g['phi'])), 'w': 16 * U * np.max(np.abs(g['w'])),
            'w_err': 16 * U * np.nanmax(np.abs(g['w_err']))}
    for k, bar in bars.items():
        got, want = getattr(diff, k), g[k]
        assert got.shape == want.shape, k
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        err = float(np.nanmax(np.abs(got - want)))
        print('%s: max|diff| = %.3e, bar %.3e' % (k, err, bar + moved.get(k, 0.)))
        assert err <= bar + moved.get(k, 0.), k
    assert wraps_of(diff.phi, diff.co) == int(g['wraps']) and int(g['wraps']) > 0
    bar = max(8 * float(g['strain_sens'][0]), 1e-12 * abs(float(g['eps_zz']))) + moved.get('eps_zz', 0.)
    print('eps_zz: |diff| = %.3e, bar %.3e' % (abs(float(diff.eps_zz) - float(g['eps_zz'])), bar))
    assert abs(float(diff.eps_zz) - float(g['eps_zz'])) <= bar
    np.testing.assert_array_equal(diff.bed[:2], g['bed'][:2])
    assert (np.abs(diff.bed[2:] - g['bed'][2:]) <= 16 * U * np.abs(g['bed'][2:]) + moved.get('bed', 0.)).all()


def check_quad(done, g, moved=None):
    """The products of ``apdar qpproc`` against the reference's at the bars of ``test_quadpol_cpu.py`` (rotation 8 u of
    the summed magnitudes, coherence 4 N u with equal NaN positions) and ``test_apres_flows_cpu.py`` (``cpe_idxs`` equal
    wherever the gap to the runner-up exceeds 1000 x the filter's sensitivity: every row of this fixture)."""
    moved = moved or {}
    rows = g['rows_kept']
    np.testing.assert_array_equal(done.thetas, g['thetas'])
    for k in ('HH', 'HV', 'VH', 'VV'):
        got = getattr(done, k)
        assert got.dtype == np.complex128 and got.shape == (len(g['range']), int(g['n_thetas']))
        assert (np.abs(got[rows] - g[k]) <= rotation_bar(g)[rows] + moved.get('image', 0.)).all(), k
    got, want = done.chhvv[rows], g['chhvv']
    np.testing.assert_array_equal(np.isnan(got.real), np.isnan(want.real))
    ok = ~np.isnan(want.real)
    err = float(np.max(np.abs(got[ok] - want[ok])))
    print('chhvv: max|diff| = %.3e, bar %.3e' % (err, chhvv_bar(g) + moved.get('chhvv', 0.)))
    assert err <= chhvv_bar(g) + moved.get('chhvv', 0.)
    decided = g['gap'] > 1000 * max(float(g['filt_sens']), moved.get('filt', 0.))
    assert decided.all()                                             # a condition on the committed fixture
    np.testing.assert_array_equal(np.asarray(done.cpe_idxs)[decided], g['cpe_idxs'][decided])
    assert same_bits(np.asarray(done.cpe, dtype=float), done.thetas[np.asarray(done.cpe_idxs)].astype(float))
    np.testing.assert_array_equal(done.flags.rotation, g['flags_rotation'])
    np.testing.assert_array_equal(done.flags.coherence, g['flags_coherence'])


def test_apdar_diffproc_on_the_references_pair(hip, tmp_path):
    """``apdar diffproc`` with its defaults on the pair the reference saved: the reference's full time-difference flow on
    the same bits, at the existing bars as they stand."""
    out = str(tmp_path / 'pair_diffproc.mat')
    apdar.main(['diffproc', mat('bed_tdraw'), '-o', out])
    check_pair(ApresTimeDiff(out), golden('AI_B1_diffproc'))
    # -window and -step arrive: other windows, other products
    apdar.main(['diffproc', mat('bed_tdraw'), '-window', '40', '-step', '10', '-o', out])
    other = ApresTimeDiff(out)
    assert np.array_equal(other.flags.phase_diff, [40, 10]) and len(other.co) == len(apm.phase_diff_windows(other.snum, 40, 10)) == 296


def test_apdar_qpproc_on_the_references_quad(hip, tmp_path):
    out = str(tmp_path / 'quad_qpproc.mat')
    apdar.main(['qpproc', mat('bed_qpraw'), '-nthetas', '24', '-o', out])
    check_quad(ApresQuadPol(out), golden('AI_B2_qpproc'))


@pytest.fixture(scope='module')
def bed_outputs(tmp_path_factory):
    """``apdar proc`` on the two ``.DAT`` bursts of each of the six synthetic sites with a bed."""
    folder = str(tmp_path_factory.mktemp('bed'))
    outs = {}
    for name, fns in io.bed_files(folder).items():
        outs[name] = os.path.join(folder, 'site_%s.mat' % name)
        np.random.seed(5)
        with np.errstate(invalid='ignore'):
            apdar.main(['proc'] + fns + ['-o', outs[name]])
    return folder, outs


def test_apdar_diffproc_on_two_outputs_of_apdar_proc(hip, bed_outputs):
    """From the ``.DAT`` files on: each profile is within Es of the reference's (the stacked bar above), so every product
    gets, on top of its existing bar, 8 x the largest change that the reference's own flow showed when both of its
    profiles were moved by Es (1 + i) N(0, 1) a sample (``in_sens`` of the fixture).  Wraps and bed sample are equal."""
    folder, outs = bed_outputs
    g = golden('AI_B1_diffproc')
    for k, name in (('data', 'time1'), ('data2', 'time2')):
        got = ApresData(outs[name]).data.flatten()
        assert (np.abs(got - g[k]) <= float(g['Es']) + 4 * U * np.abs(g[k])).all(), k
    out = os.path.join(folder, 'pair_diffproc.mat')
    apdar.main(['diffproc', outs['time1'], outs['time2'], '-o', out])
    moved = {str(k): 8. * float(v) for k, v in zip(g['in_sens_names'], g['in_sens'])}
    check_pair(ApresTimeDiff(out), g, moved)


def test_apdar_qpproc_on_four_outputs_of_apdar_proc(hip, bed_outputs):
    folder, outs = bed_outputs
    g = golden('AI_B2_qpproc')
    raw = os.path.join(folder, 'site_qpraw.mat')
    apdar.main(['load', '-acq_type', 'quadpol'] + [outs[k] for k in ('HH', 'HV', 'VH', 'VV')] + ['-o', raw])
    qp = ApresQuadPol(raw)
    for k in ('shh', 'shv', 'svh', 'svv'):
        assert (np.abs(getattr(qp, k) - g['in_' + k]) <= float(g['Es']) + 4 * U * np.abs(g['in_' + k])).all(), k
    assert same_bits(qp.range, g['range'])
    apdar.main(['qpproc', raw, '-nthetas', '24'])
    moved = {'image': 8. * float(g['image_in_sens']), 'chhvv': 8. * float(g['chhvv_in_sens']), 'filt': 8. * float(g['filt_in_sens'])}
    check_quad(ApresQuadPol(os.path.join(folder, 'site_qpproc.mat')), g, moved)
