"""The complex-trace attributes without a GPU: ``check_attr`` refuses what csrc/attr_route.h refuses without a library call, the
yardstick of tests/attr_ref.py is sound (its transform against NumPy's, ``ref`` within its own bars of ``hi``, the 1 % condition
of the smoothed frequency on the chosen seeds), and ``impproc attr`` parses what it should."""
import sys
from unittest.mock import patch

import numpy as np
import pytest

import attr_ref as R


def test_check_attr_refuses_without_a_library_call():
    from impdar_amd import attributes as A
    with patch.object(A._hip, 'load', side_effect=AssertionError('no library call')):
        assert A.check_attr((100, 8), 'envelope') == (1, 1, 1.0)
        assert A.check_attr((100, 8), 'frequency', 9, 2.0e-9) == (3, 9, 2.0e-9)
        assert A.check_attr((100, 8), 2, 1, float('nan')) == (2, 1, 1.0)            # dt is read for the frequency alone
        assert [A.check_attr((1, 1), k)[0] for k in R.KINDS] == [0, 1, 2, 3]
        for kind in ('amplitude', 4, -1, None, 1.5, True):
            with pytest.raises(ValueError, match='kind must be 0'):
                A.check_attr((100, 8), kind)
        for smooth in (0, 2, 256, 257, -3, 2.5):
            with pytest.raises(ValueError, match='smooth must be odd and lie in 1 .. 255'):
                A.check_attr((100, 8), 'frequency', smooth)
        for kind in ('quadrature', 'envelope', 'phase'):
            with pytest.raises(ValueError, match='smooth above 1 goes with kind 3'):
                A.check_attr((100, 8), kind, 3)
        for dt in (0.0, -1.0, float('nan'), float('inf')):
            with pytest.raises(ValueError, match='dt must be finite and positive'):
                A.check_attr((100, 8), 'frequency', 1, dt)
        for shape in ((0, 8), (100, 0), (100,)):
            with pytest.raises(ValueError, match='empty radargram'):
                A.check_attr(shape, 'envelope')


def test_methods_are_bound_and_refuse_before_the_library():
    from impdar_amd import attributes as A
    from impdar_amd.lib.RadarData import RadarData
    for name in ('envelope', 'instantaneous_phase', 'instantaneous_frequency', 'complex_attribute', 'analytic_signal'):
        assert getattr(RadarData, name) is getattr(A, name)
    d = RadarData(None)
    d.data, d.snum, d.tnum, d.dt = np.zeros((16, 4), dtype=np.float32), 16, 4, 1.0e-9
    with patch.object(A._hip, 'load', side_effect=AssertionError('no library call')):
        with pytest.raises(ValueError, match='smooth must be odd'):
            d.instantaneous_frequency(smooth=4)
        with pytest.raises(ValueError, match='kind must be'):
            d.complex_attribute('power')
        d.dt = 0.0
        with pytest.raises(ValueError, match='dt must be finite and positive'):
            d.instantaneous_frequency()
        d.data = d.data.astype(np.complex64)
        with pytest.raises(TypeError, match='complex'):
            d.envelope()


@pytest.mark.parametrize('n', [1, 2, 3, 30, 33, 44, 60, 126, 2048, 5462])
def test_the_longdouble_transform_is_a_transform(n):
    rng = np.random.default_rng(n)
    x = (rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))).astype(R.CLD)
    X = R.fft_ld(x)
    want = np.fft.fft(x.astype(np.complex128), axis=0)
    assert np.max(np.abs(X.astype(np.complex128) - want)) <= 1e-12 * np.sqrt(n) * np.max(np.abs(want))
    back = R.fft_ld(X, +1) / R.LD(n)
    assert float(np.max(np.abs(back - x))) <= 1e-17 * n


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('case', [c for c in R.CASES if c[0] * c[1] <= 20000], ids=R.case_id)
def test_ref_is_near_hi(case, dtype):
    """``ref`` sits a few units of the data's precision from ``hi``: the bars 8 x that distance are neither zero where the
    device may differ nor wide enough to hide a wrong formula (a sign, a missing zero of the multiplier, an off-by-one step)."""
    n, tnum = case[:2]
    eps = float(np.finfo(dtype).eps)
    for name in R.FIXTURES:
        x = R.FIXTURES[name](n, tnum, dtype, seed=n + tnum)
        Y = R.Yard(x)
        amp = float(np.max(np.abs(x))) + 1.0
        for kind in R.KINDS:
            e, _ = Y.distance(R.attr_ref(x, kind), kind)
            scale = amp * eps * (np.log2(n) + 4) * (n if kind == 'frequency' else 1)       # (unwrap adds up n roundings)
            assert e <= 8 * scale, (name, kind, e, scale)
        # the restatement is the contract: the quadrature of a cosine on a bin is the sine
        if n >= 30 and n % 2 == 0:
            k = np.arange(n)[:, None]
            c = np.cos(2 * np.pi * 3 * k / n) * np.ones((1, 2))
            assert float(np.max(np.abs(R.quadrature_hi(c) - np.sin(2 * np.pi * 3 * k / n)))) < 1e-13


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('shape', R.SMOOTH_CASES + [(n - 1, t) for n, t in R.SMOOTH_CASES], ids=lambda s: '%dx%d' % s)      # (odd: the rocFFT route)
def test_smoothed_frequency_condition_on_the_chosen_seeds(shape, dtype):
    """The bar of the smoothed frequency leaves out the windows with a step within 1e-6 rad of +-pi: on the fixtures' seeds that
    is at most 1 % of the samples, and ``ref`` is inside its own bar there."""
    n, tnum = shape
    x = R.fixture(n, tnum, dtype)
    Y = R.Yard(x)
    for W in R.SMOOTHS:
        ref = R.attr_ref(x, 'frequency', W)
        e, out = Y.distance(ref, 'frequency', W)
        assert out <= 0.01, (W, out)
        assert np.isfinite(e) and R.held('ref %dx%d W %d' % (n, tnum, W), Y, ref, ref, 'frequency', W) <= 1.0
    # W = 1 of the window sum is the identity, and a window longer than the trace is the whole trace's mean
    f = Y.hi('frequency', 1)
    w = Y.xl * Y.xl + Y.q * Y.q
    whole = Y.hi('frequency', 255) if n <= 127 else None
    if whole is not None:
        want = np.sum(w * f, axis=0) / np.sum(w, axis=0)
        assert float(np.max(np.abs(whole - want[None, :]) / np.max(np.abs(want)))) < 1e-15


def test_non_finite_and_zero_traces_in_the_restatement():
    x = R.fixture(60, 6, np.float64).copy()
    x[7, 1] = np.nan
    x[9, 3] = -np.inf
    x[:, 4] = 0
    for kind in R.KINDS:
        for f in (R.attr_hi, R.attr_ref):
            y = f(x, kind)
            assert np.all(np.isnan(y[:, [1, 3]])) and np.all(y[:, 4] == 0) and np.all(np.isfinite(y[:, [0, 2, 5]])), (kind, f.__name__)


def test_impproc_attr_parser():
    from impdar_amd.bin import impproc
    p = impproc._get_args()
    a = p.parse_args(['attr', '--kind', 'envelope', 'a.mat', 'b.mat'])
    assert a.func is impproc.attr and a.kind == 'envelope' and a.smooth == 1 and a.fns == ['a.mat', 'b.mat'] and a.ftype == 'mat' and a.o is None
    a = p.parse_args(['attr', '--kind', 'frequency', '--smooth', '9', '-o', 'out/', 'a.mat'])
    assert a.kind == 'frequency' and a.smooth == 9 and a.o == 'out/'
    assert impproc.ATTR_NAMES == {'envelope': 'env', 'phase': 'phase', 'frequency': 'ifreq'}
    for argv in (['attr', 'a.mat'], ['attr', '--kind', 'quadrature', 'a.mat'], ['attr', '--kind', 'envelope'],
                 ['attr', '--kind', 'frequency', '--smooth', 'x', 'a.mat']):
        with pytest.raises(SystemExit):
            with patch.object(sys, 'stderr'):
                p.parse_args(argv)

    class Dat(object):
        called = None

        def envelope(self):
            self.called = ('envelope',)

        def instantaneous_phase(self):
            self.called = ('phase',)

        def instantaneous_frequency(self, smooth=1):
            self.called = ('frequency', smooth)

    for kind, smooth, want in (('envelope', 1, ('envelope',)), ('phase', 1, ('phase',)), ('frequency', 9, ('frequency', 9))):
        d = Dat()
        impproc.attr(d, kind=kind, smooth=smooth, fns=['a.mat'], o=None)
        assert d.called == want
    with pytest.raises(ValueError, match='--smooth'):
        impproc.attr(Dat(), kind='envelope', smooth=3)
