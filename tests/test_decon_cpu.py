"""Predictive deconvolution without a GPU: the Levinson recursion of csrc/decon_core.h (its host instantiation, compiled here with
g++) against the longdouble restatement of tests/decon_ref.py, the restatement against an analytic case, and the refusals of
``impdar_amd.decon.check_decon`` / ``check_acorr``, which never load the library."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import decon_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, 'impdar_amd', 'csrc')
needs_gxx = pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not installed')

PROBE = r'''
#include "decon_core.h"
#include <vector>
extern "C" int decon_probe_levinson(const double *c, const double *rhs, int n, double *a)
{
    std::vector<double> work(2 * (size_t)n);
    return decon_levinson_host(c, rhs, n, a, work.data()) ? 1 : 0;
}
'''


@pytest.fixture(scope='module')
def core(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('deconcore'))
    src, so = os.path.join(tmp, 'decon_core_probe.cpp'), os.path.join(tmp, 'libdeconcore.so')
    with open(src, 'w') as f:
        f.write(PROBE)
    # the contract's sums are fmas: -ffp-contract=off keeps the compiler from making more of them, as the library's flags do
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-Werror', '-shared', '-fPIC', '-I', CSRC, src, '-o', so])
    return C.CDLL(so)


def header_levinson(core, c, b):
    c, b = np.ascontiguousarray(c, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    a = np.full(len(b), np.nan)
    dp = C.POINTER(C.c_double)
    ok = core.decon_probe_levinson(c.ctypes.data_as(dp), b.ctypes.data_as(dp), len(b), a.ctypes.data_as(dp))
    return bool(ok), a


# (snum, gap, oplen, eps) of the prototype's cases, and two with a gap
SYSTEMS = [(64, 1, 8, 1e-3), (200, 1, 64, 1e-3), (128, 1, 32, 1e-5), (200, 7, 64, 1e-3), (128, 40, 32, 1e-3)]


@needs_gxx
@pytest.mark.parametrize('snum,gap,oplen,eps', SYSTEMS, ids=['%d-g%d-n%d-e%g' % s for s in SYSTEMS])
@pytest.mark.parametrize('fixture', sorted(R.FIXTURES))
def test_header_levinson_against_the_longdouble_recursion(core, fixture, snum, gap, oplen, eps):
    """max|a - a_hi| <= 8 max|a_ref - a_hi| on one float64 system: a the header's host recursion, a_ref SciPy's solve_toeplitz,
    a_hi the longdouble recursion -- the project's 8x rule for a different order of the same sums."""
    from scipy.linalg import solve_toeplitz
    x = R.FIXTURES[fixture](snum, 1, np.float64)[:, 0]
    r = R.lags_1d(x, 0, snum, R.lag_list(oplen, gap), 'ref')
    c = np.array([r[l] for l in range(oplen)])
    c[0] *= 1.0 + eps
    b = np.array([r[gap + m] for m in range(oplen)])
    a_hi = R.levinson_hi(c, b)
    a_ref = solve_toeplitz(c, b)
    ok, a = header_levinson(core, c, b)
    assert ok and a_hi is not None
    e_dev, e_ref = R.err(a, a_hi), R.err(a_ref, a_hi)
    print('levinson %s snum %d gap %d oplen %d eps %g: header %.3e scipy %.3e ratio %.2f' % (fixture, snum, gap, oplen, eps, e_dev, e_ref,
                                                                                           e_dev / e_ref))
    assert e_dev <= 8 * e_ref


@needs_gxx
def test_header_levinson_dead_systems(core):
    """A zero lag that is zero, negative, NaN or Inf, and an error power that reaches zero exactly: zeros and `false`."""
    for c0 in (0.0, -1.0, np.nan, np.inf):
        ok, a = header_levinson(core, [c0, 0.5, 0.25], [0.5, 0.25, 0.125])
        assert not ok and np.all(a == 0), c0
    ok, a = header_levinson(core, [1.0, 1.0, 1.0], [1.0, 1.0, 1.0])         # v' = 1 - 1 = 0 at the first step
    assert not ok and np.all(a == 0)
    ok, a = header_levinson(core, [2.0], [1.0])
    assert ok and a[0] == 0.5


def test_longdouble_recursion_solves_its_system():
    rng = np.random.default_rng(2)
    x = rng.standard_normal(300)
    r = R.lags_1d(x, 0, 300, range(40), 'hi')
    c = np.array([r[l] for l in range(20)], dtype=R.LD)
    c[0] *= 1 + R.LD(1e-3)
    b = np.array([r[3 + m] for m in range(20)], dtype=R.LD)
    a = R.levinson_hi(c, b)
    T = np.array([[c[abs(i - j)] for j in range(20)] for i in range(20)], dtype=R.LD)
    assert float(np.max(np.abs(T @ a - b))) <= 1e-15 * float(np.max(np.abs(b)))


@pytest.mark.parametrize('rho,T,k1,amp', [(0.5, 8, 3, 4.0), (-0.75, 8, 5, 0.5), (0.75, 8, 0, -2.0)])
def test_analytic_spike_train(rho, T, k1, amp):
    """x = sum_m rho^m s[k - m T] with s one spike of height amp at k1: x[k1 + m T] = amp rho^m, m = 0 .. M, M the last echo inside
    the 256 samples.  Then r[0] = amp^2 sum_{m <= M} rho^2m and r[T] = amp^2 rho sum_{m < M} rho^2m (the echo M has no partner),
    so with gap = T, oplen = 1, eps = 0 the operator is a = r[T] / r[0] = rho (1 - rho^2M) / (1 - rho^(2M + 2)): rho but for the
    truncation term rho^(2M + 1) (1 - rho^2) / (1 - rho^(2M + 2)).  y = x - a x[k - T] is then the spike, plus (rho - a) x[k - T].
    The powers of 0.5 and 0.75 up to M = 31 are exact in float64, so the data is the train exactly."""
    snum = 256
    M = (snum - 1 - k1) // T
    x = np.zeros((snum, 1))
    x[k1 + T * np.arange(M + 1), 0] = amp * np.array([rho ** m for m in range(M + 1)])
    y, ops = R.decon(x, 1, gap=T, prewhiten=0.0, kind='hi')
    rl = R.LD(rho)
    want = rl * (1 - rl ** (2 * M)) / (1 - rl ** (2 * M + 2))
    eps_ld = float(np.finfo(R.LD).eps)
    assert abs(float(ops[0, 0] - want)) <= 8 * eps_ld * abs(rho)
    trunc = abs(rho) ** (2 * M + 1) * (1 - rho ** 2) / (1 - abs(rho) ** (2 * M + 2))
    assert abs(float(ops[0, 0]) - rho) <= trunc * (1 + 1e-6) + 8 * eps_ld
    spike = np.zeros(snum)
    spike[k1] = amp
    assert float(np.max(np.abs(y[:, 0] - spike))) <= (trunc + 8 * eps_ld) * abs(amp)
    # float64 reference: the same within its own rounding -- r[0] and r[T] each carry at most M + 1 roundings of 2^-53 (the
    # products and the additions of M + 1 terms of one sign pattern), the quotient one more
    u64 = 2 * (M + 2) * 2.0 ** -53
    y64, ops64 = R.decon(x, 1, gap=T, prewhiten=0.0, kind='ref')
    assert abs(ops64[0, 0] - float(want)) <= u64 and np.max(np.abs(y64[:, 0] - spike)) <= (trunc + u64) * abs(amp)


def test_reference_and_restatement_agree_on_the_fixtures():
    for name, make in sorted(R.FIXTURES.items()):
        x = make(120, 3, np.float64)
        for design in ('each', 'mean'):
            yh, ah = R.decon(x, 16, gap=4, prewhiten=0.1, window=(10, 110), design=design, kind='hi')
            yr, ar = R.decon(x, 16, gap=4, prewhiten=0.1, window=(10, 110), design=design, kind='ref')
            assert R.err(ar, ah) <= 1e-9 * float(np.max(np.abs(ah))) and R.err(yr, yh) <= 1e-9 * float(np.max(np.abs(yh))), (name, design)
    A = R.acorr(R.noise(50, 2, np.float32), 10, kind='ref')
    assert A.shape == (11, 2) and np.all(A[0] == 1.0)


def test_dead_traces_in_the_restatement():
    x = R.ringing(80, 5, np.float64)
    x[:, 1] = 0.0
    x[30, 2] = np.nan
    x[40, 3] = np.inf
    for kind in ('hi', 'ref'):
        y, ops = R.decon(x, 8, gap=2, kind=kind)
        for j in (1, 2, 3):
            assert np.array_equal(np.asarray(y[:, j], dtype=np.float64), x[:, j], equal_nan=True) and np.all(ops[:, j] == 0)
        assert np.any(ops[:, 0] != 0) and np.any(ops[:, 4] != 0)
        A = R.acorr(x, 5, kind=kind)
        assert np.all(np.isnan(np.asarray(A[:, 1:4], dtype=np.float64))) and np.all(np.isfinite(np.asarray(A[:, [0, 4]], dtype=np.float64)))
        ym, om = R.decon(x, 8, gap=2, design='mean', kind=kind)
        assert np.all(om[:, 0] == om[:, 4]) and np.all(om[:, 1:4] == 0)


def test_check_decon_refuses_without_the_library(monkeypatch):
    from impdar_amd import _hip, decon

    def no_library(*a, **k):
        raise AssertionError('the checks must not reach the library')
    monkeypatch.setattr(_hip, 'load', no_library)
    monkeypatch.setattr(_hip, 'context', no_library)
    shape = (100, 8)
    assert decon.check_decon(shape, 8) == (0, 100, 8, 1, 0.1, 0)
    assert decon.check_decon(shape, 8, gap=2, prewhiten=0, window=(10, 20), design='mean') == (10, 20, 8, 2, 0.0, 1)
    assert decon.check_decon((600, 2), 256) == (0, 600, 256, 1, 0.1, 0)
    bad = [dict(oplen=0), dict(oplen=257), dict(oplen=8, gap=0), dict(oplen=8, window=(-1, 50)), dict(oplen=8, window=(50, 50)),
           dict(oplen=8, window=(0, 101)), dict(oplen=8, gap=3, window=(10, 20)), dict(oplen=9, gap=2, window=(10, 20)),
           dict(oplen=8, prewhiten=-0.1), dict(oplen=8, prewhiten=float('nan')), dict(oplen=8, prewhiten=float('inf')),
           dict(oplen=8, design='all'), dict(oplen=2.5), dict(oplen=8, gap=1.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            decon.check_decon(shape, **kw)
    with pytest.raises(ValueError, match='oplen must lie in 1 .. 256'):
        decon.check_decon(shape, 300)
    with pytest.raises(ValueError, match="gap \\+ oplen must not exceed the window's length"):
        decon.check_decon(shape, 60, gap=41)
    assert decon.check_acorr(shape, 99) == (0, 100, 99) and decon.check_acorr(shape, 19, window=(10, 30)) == (10, 30, 19)
    for kw in (dict(maxlag=100), dict(maxlag=-1), dict(maxlag=20, window=(10, 30)), dict(maxlag=5, window=(30, 30))):
        with pytest.raises(ValueError):
            decon.check_acorr(shape, **kw)


def test_the_unit_is_built_and_bound():
    from impdar_amd import _hip, build
    from impdar_amd.lib.RadarData import RadarData
    assert 'decon.hip' in build.SOURCES
    assert {'impdar_decon', 'impdar_decon_dev', 'impdar_acorr', 'impdar_acorr_dev'} <= set(_hip.SIGNATURES)
    assert all(hasattr(RadarData, m) for m in ('predictive_decon', 'decon_operators', 'autocorrelation'))
