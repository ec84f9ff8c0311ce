"""The filtfilt designs the GPU tests sweep (tests/filtfilt_ref.py) are well conditioned: SciPy's float64
``filtfilt`` is within 1e-13 * max|y| of the same filter run in long double, from SciPy's own ``lfilter_zi``.  A
kernel that misses the GPU bar on one of them is therefore wrong, not the design."""
import numpy as np
import pytest

import filtfilt_ref as fr
from oracle import preproc_oracle as po

pytestmark = pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63,
                                reason='the long-double twin needs a 64-bit significand (x87 extended precision)')

BAR = 1e-13


def _conditioning(b, a):
    from scipy import signal
    # the twin starts from the same float64 steady state as SciPy (and as the kernels, which receive it)
    np.testing.assert_array_equal(po.lfilter_zi(b, a), signal.lfilter_zi(b, a))
    x = np.random.default_rng(0).standard_normal((400, 8))
    want = fr.filtfilt_ld(b, a, x)
    assert want.dtype == np.longdouble
    got = signal.filtfilt(b, a, x, axis=0)
    return fr.rel_err(got, want)


@pytest.mark.parametrize('ncoef', range(fr.NCOEF_MIN, fr.VERT_MAX + 1))
def test_sweep_design_is_well_conditioned(ncoef):
    b, a = fr.design(ncoef)
    assert b.shape == a.shape == (ncoef,) and a[0] == 1.0
    err = _conditioning(b, a)
    assert err <= BAR, (ncoef, err)


@pytest.mark.parametrize('filttype,order', fr.API_DESIGNS)
def test_public_api_design_is_well_conditioned(filttype, order):
    kind, b, a = po.design(1e-8, *fr.API_BAND, order=order, filttype=filttype)
    assert kind == 'iir' and len(b) == len(a) == 2 * order + 1
    err = _conditioning(b, a)
    assert err <= BAR, (filttype, order, err)


def test_long_double_twin_changes_only_the_precision():
    """The oracle runs in float64 unless asked; dtype=np.longdouble returns the same filter in long double, which
    differs from the float64 result by rounding only."""
    b, a = fr.design(7)
    x = np.random.default_rng(1).standard_normal((60, 3)).astype(np.float32)   # extension formed in float32 by both
    y64 = po.filtfilt(b, a, x)
    assert y64.dtype == np.float64
    np.testing.assert_array_equal(y64, po.filtfilt(b, a, x, dtype=np.float64))
    yld = fr.filtfilt_ld(b, a, x)
    assert yld.dtype == np.longdouble and yld.shape == y64.shape == x.shape
    assert 0.0 < fr.rel_err(y64, yld) < 1e-14
