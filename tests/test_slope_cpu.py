"""The yardstick of the layer-slope steps against itself, without a GPU: ``ref`` (NumPy / SciPy in float64) against ``hi`` (the
contract in longdouble) on every case of the fixture, the conditions the fixture has to meet, every ValueError of the checks
with no device call, the impproc parsers and output names, and two facts about what the slope field is for."""
import sys
from unittest.mock import patch

import numpy as np
import pytest

import slope_ref as R


@pytest.mark.parametrize('sigma', R.CPU_SIGMAS, ids=str)
@pytest.mark.parametrize('shape', R.CPU_SHAPES, ids=R.case_id)
def test_ref_against_hi_and_the_fixture_conditions(shape, sigma):
    """ref sits within a few 1e-16 .. 1e-15 of hi in every kind (relative to the tensor's size); the fixture leaves no sample out
    of the slope's distance and has no sample with d < 0, b = 0."""
    for dtype in (np.float32, np.float64):
        x = R.fixture(shape[0], shape[1], dtype)
        Y = R.Yard(x, sigma)
        assert not Y.left_out().any() and not Y.vertical().any()
        scale = float(np.max(Y.hi('jzz') + Y.hi('jxx')))
        for kind in R.KINDS:
            e, out = Y.distance(R.slope_ref(x, kind, sigma), kind)
            print('%s %s %s: ref %.3e of %.3e' % (kind, shape, sigma, e, scale))
            assert out == 0.0 and 0 < e <= 1e-14 * scale, (kind, e, scale)
        slope = Y.given_slope()
        for half in R.HALVES:
            hi = R.dipsmooth_hi(x, half, slope)
            e = float(np.max(np.abs(R.dipsmooth_ref(x, half, slope).astype(R.LD) - hi)))
            # the position k + p i carries 2^-53 (n + |p i|), |p i| <= 4 x 32, into the fraction, which multiplies a difference of
            # two samples; the interpolation and the mean add a few roundings of the samples' size; float32 rounds the result
            bound = 2.0 ** -52 * (shape[0] + 136) * float(np.max(np.abs(x))) + (2.0 ** -24 if dtype == np.float32 else 0) * float(np.max(np.abs(hi)))
            assert e <= bound, (half, e, bound)


def test_ref_equals_numpy_gradient_and_the_contracts_weights():
    x = R.fixture(33, 70, np.float64)
    assert np.array_equal(R.gradient(np.array(x), 0), np.gradient(x, axis=0)) and np.array_equal(R.gradient(np.array(x), 1), np.gradient(x, axis=1))
    for sigma in (0.5, 1.0, 3.0, 16.0):
        w = R.weights(sigma)
        assert len(w) == 2 * int(4 * sigma + 0.5) + 1 and abs(w.sum() - 1) < 1e-15


def test_non_finite_samples_become_nan_within_reach():
    x = np.array(R.fixture(60, 31, np.float64))
    x[20, 10] = np.inf
    sigma = (1.0, 1.0)
    bad = np.isnan(R.slope_hi(x, 'slope', sigma))
    rz, rx = R.radius(sigma[0]) + 1, R.radius(sigma[1]) + 1
    want = np.zeros_like(bad)
    want[20 - rz:20 + rz + 1, 10 - rx:10 + rx + 1] = True
    assert bad.any() and not (bad & ~want).any()
    for kind in R.KINDS:
        assert np.array_equal(np.isnan(R.slope_hi(x, kind, sigma)), np.isnan(R.slope_ref(x, kind, sigma)))
    p = np.zeros((60, 31))
    p[5, 5] = np.nan
    y = R.dipsmooth_ref(x, 2, p)
    # (row 19 reads x[19] + 0 (x[20] - x[19]): NaN by IEEE arithmetic, as the contract has it)
    assert np.isnan(y[5, 5]) and np.isnan(y[19:21, 8:13]).all() and not np.isnan(y[20, 7]) and np.isnan(y).sum() == 11


def test_a_dipping_layer_has_its_slope_and_is_coherent():
    k, j = np.meshgrid(np.arange(96.0), np.arange(80.0), indexing='ij')
    x = np.cos(2 * np.pi * (k - 0.5 * j) / 16)
    inner = (slice(16, -16), slice(16, -16))
    p = R.slope_ref(x, 'slope', (3.0, 3.0))[inner]
    assert abs(np.median(p) - 0.5) < 0.05
    assert R.slope_ref(x, 'coherence', (3.0, 3.0))[inner].min() > 0.99
    assert np.allclose(np.tan(R.slope_ref(x, 'dip', (3.0, 3.0))[inner]), p, atol=1e-9)


def test_steering_the_mean_keeps_what_the_row_mean_cancels():
    """A 16-sample-period layer of slope 0.6 with noise of sigma 0.5: the 9-trace mean along the estimated slope leaves a smaller
    rms error than the same mean along the rows, and both less than the noise."""
    rng = np.random.default_rng(7)
    k, j = np.meshgrid(np.arange(128.0), np.arange(160.0), indexing='ij')
    clean = np.cos(2 * np.pi * (k - 0.6 * j) / 16)
    x = clean + 0.5 * rng.standard_normal(clean.shape)
    inner = (slice(16, -16), slice(16, -16))
    steered = R.dipsmooth_ref(x, 4, R.slope_ref(x, 'slope', (2.0, 8.0)))

    def rms(y):
        return float(np.sqrt(np.mean((y - clean)[inner] ** 2)))
    print('rms raw %.3f rows %.3f steered %.3f' % (rms(x), rms(R.rowmean_ref(x, 4)), rms(steered)))
    assert rms(steered) < rms(R.rowmean_ref(x, 4)) < rms(x) and rms(steered) < 0.2


def test_every_value_error_of_the_checks_without_a_device_call():
    from impdar_amd import _hip, slope as S
    with patch.object(_hip, 'load', side_effect=AssertionError('the library was reached')):
        assert S.check_slope((100, 8)) == (0, 2.0, 8.0, 4.0)
        assert S.check_slope((100, 8), 'coherence', (0, 16), 1.5, np.float32) == (2, 0.0, 16.0, 1.5)
        assert S.check_dipsmooth((100, 8), 4) == (4, 2.0, 8.0, 4.0)
        given = np.zeros((100, 8))
        assert S.check_dipsmooth((100, 8), 32, (99, 99), -1, given)[0] == 32                # (sigma and max_slope are not read)
        bad = [lambda: S.check_slope((100, 8), 'power'), lambda: S.check_slope((100, 8), 6), lambda: S.check_slope((100, 8), True),
               lambda: S.check_slope((100, 8), 0, (-1, 1)), lambda: S.check_slope((100, 8), 0, (1, 16.5)),
               lambda: S.check_slope((100, 8), 0, (float('nan'), 1)), lambda: S.check_slope((100, 8), 0, 2.0),
               lambda: S.check_slope((100, 8), 0, (2, 8), 0), lambda: S.check_slope((100, 8), 0, (2, 8), float('inf')),
               lambda: S.check_slope((0, 8)), lambda: S.check_slope((100, 0)), lambda: S.check_slope((100, 8), dtype=np.int16),
               lambda: S.check_slope((100, 8), dtype=np.complex64),
               lambda: S.check_dipsmooth((100, 8), 0), lambda: S.check_dipsmooth((100, 8), 33), lambda: S.check_dipsmooth((100, 8), 2.5),
               lambda: S.check_dipsmooth((100, 8), 4, (17, 1)), lambda: S.check_dipsmooth((100, 8), 4, (2, 8), -2),
               lambda: S.check_dipsmooth((0, 8), 4), lambda: S.check_dipsmooth((100, 8), 4, dtype=np.int32),
               lambda: S.check_dipsmooth((100, 8), 4, slope=np.zeros((8, 100))), lambda: S.check_dipsmooth((100, 8), 4, slope=np.zeros((100, 8), np.float32))]
        for call in bad:
            with pytest.raises(ValueError):
                call()


def test_impproc_parsers_and_output_names(tmp_path):
    from impdar_amd.bin import impproc
    parser = impproc._get_args()
    a = parser.parse_args(['dipsmooth', '4', 'a.mat'])
    assert (a.func, a.name, a.half, a.sigma, a.max_slope, a.fns) == (impproc.dipsmooth, 'dipsm', 4, [2.0, 8.0], 4.0, ['a.mat'])
    a = parser.parse_args(['dipsmooth', '9', '--sigma', '1', '3.5', '--max_slope', '2', 'a.mat', 'b.mat'])
    assert (a.half, a.sigma, a.max_slope, a.fns) == (9, [1.0, 3.5], 2.0, ['a.mat', 'b.mat'])
    a = parser.parse_args(['slope', '--kind', 'dip', '--sigma', '0', '2', 'a.mat'])
    assert (a.func, a.name, a.kind, a.sigma, a.max_slope) == (impproc.slope, 'slope', 'dip', [0.0, 2.0], 4.0)
    assert impproc.SLOPE_NAMES == {'slope': 'slope', 'dip': 'dip', 'coherence': 'coh'}
    for argv in (['slope', 'a.mat'], ['slope', '--kind', 'jzz', 'a.mat'], ['dipsmooth', 'a.mat'], ['dipsmooth', '4', '--sigma', '1', 'a.mat']):
        with pytest.raises(SystemExit), patch.object(sys, 'stderr'):
            parser.parse_args(argv)

    # what main() does with them: the methods it calls and the names it saves under
    class Dat(object):
        calls, saved, _dev = [], [], None

        def dip_smooth(self, half, **kw):
            self.calls.append(('dip_smooth', half, kw))

        def layer_slope(self, **kw):
            self.calls.append(('layer_slope', kw))
            return np.zeros((3, 2))

        def save(self, fn):
            self.saved.append(fn)
    fn = str(tmp_path / 'line_raw.mat')
    for argv, suffix in ((['dipsmooth', '4'], 'dipsm'), (['slope', '--kind', 'slope'], 'slope'), (['slope', '--kind', 'dip'], 'dip'),
                         (['slope', '--kind', 'coherence', '--sigma', '1', '2'], 'coh')):
        d = Dat()
        with patch.object(sys, 'argv', ['impproc'] + argv + [fn]), patch.object(impproc, 'load', return_value=[d]):
            impproc.main()
        assert d.saved[-1] == str(tmp_path / ('line_%s.mat' % suffix))
    assert Dat.calls[0] == ('dip_smooth', 4, dict(sigma=(2.0, 8.0), max_slope=4.0))
    assert Dat.calls[-1] == ('layer_slope', dict(sigma=(1.0, 2.0), kind='coherence', max_slope=4.0))
    assert d.data.dtype == np.float64 and d.data.shape == (3, 2)


def test_methods_are_bound_and_documented():
    from impdar_amd.lib import RadarData as pkg
    from impdar_amd import slope as S
    assert pkg.RadarData.layer_slope is S.layer_slope and pkg.RadarData.dip_smooth is S.dip_smooth
    assert 'layer_slope' in pkg.__doc__ and 'dip_smooth' in pkg.__doc__
    c = pkg.RadarData(None)
    c.data, c.snum, c.tnum = np.zeros((4, 3), dtype=np.complex64), 4, 3
    with pytest.raises(TypeError):
        c.layer_slope()
    with pytest.raises(TypeError):
        c.dip_smooth(2)
