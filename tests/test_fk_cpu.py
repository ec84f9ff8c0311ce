"""The f-k fan filter without a GPU: the yardstick (tests/fk_ref.py) against an analytic case and its own Hermitian
symmetry, the weight header (csrc/fk_weight.h, compiled here by itself with g++) against the yardstick's longdouble weight
at every seam, and the refusals of the Python layer.
"""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import fk_ref
from conftest import ROOT

CSRC = os.path.join(ROOT, 'impdar_amd', 'csrc')
U = 2.0 ** -53
SHAPES = ((64, 64), (66, 130), (63, 65), (100, 96), (2, 64), (128, 3))

PROBE = r'''
#include "fk_weight.h"
extern "C" void fk_probe_weight(double va_lo, double va_hi, double taper, int mode, int dip, int n, const double *w, const double *kx,
                                const int *nyq, double *out)
{
    const FkFan fan = fk_fan_make(va_lo, va_hi, taper, mode, dip);
    for (int i = 0; i < n; ++i) out[i] = fk_weight(fan, w[i], kx[i], nyq[i] != 0);
}
'''


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('fkweight'))
    src, lib = os.path.join(tmp, 'fk_weight_probe.cpp'), os.path.join(tmp, 'libfkweight.so')
    with open(src, 'w') as f:
        f.write(PROBE)
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-ffp-contract=off', '-shared', '-fPIC', '-I', CSRC, src, '-o', lib])
    return C.CDLL(lib)


def header_weight(lib, w, kx, nyq, va_lo, va_hi, taper, mode, dip):
    w = np.ascontiguousarray(w, dtype=np.float64)
    kx = np.ascontiguousarray(kx, dtype=np.float64)
    nyq = np.ascontiguousarray(nyq, dtype=np.int32)
    out = np.empty(len(w), dtype=np.float64)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    nan = float('nan')
    lib.fk_probe_weight(C.c_double(nan if va_lo is None else va_lo), C.c_double(nan if va_hi is None else va_hi), C.c_double(taper),
                        fk_ref.MODES.index(mode), fk_ref.DIPS.index(dip), len(w), w.ctypes.data_as(dp), kx.ctypes.data_as(dp),
                        nyq.ctypes.data_as(ip), out.ctypes.data_as(dp))
    return out


def ref_weight(w, kx, nyq, **fan):
    return fk_ref.weight_at(w, kx, nyq, **fan)


# ---- the yardstick itself -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', fk_ref.MODES)
@pytest.mark.parametrize('dip', fk_ref.DIPS)
def test_yardstick_separates_two_plane_events(mode, dip):
    """128 x 128, two plane events of period 16 samples and slopes +0.5 (down_right, slowness 0.5) and -1 (down_left, slowness
    1) sample per trace; the fan va_lo = 1 / (1.5 * 0.5) passes slownesses up to 0.75 (1 +- 0.1).  What survives comes back to
    1e-12 of its amplitude (1), what is removed is removed to the same bar."""
    a, b = fk_ref.two_events()
    w, kx = fk_ref.axes(128, 128, 1.0, 1.0)
    y = fk_ref.fan(a + b, w, kx, 'ref', va_lo=1.0 / 0.75, taper=0.1, mode=mode, dip=dip)
    # the fan holds event a (on the down_right side); event b is outside it on either side
    in_fan = dip in ('both', 'down_right')
    keep_a = in_fan if mode == 'pass' else not in_fan
    keep_b = mode == 'reject'
    want = (a if keep_a else 0.0) + (b if keep_b else 0.0)
    assert np.max(np.abs(y - want)) <= 1e-12
    if dip == 'down_left' and mode == 'pass':
        assert abs(np.max(np.abs(y - a)) - 1.0) <= 1e-12        # the residual against the removed event is its amplitude


@pytest.mark.parametrize('shape', SHAPES)
def test_yardstick_weight_is_hermitian(shape):
    """|Im ifft2(M fft2 x)| <= 1e-15 max|y| in longdouble, every dip and both modes: the Nyquist rule keeps the result real."""
    snum, tnum = shape
    x = fk_ref.radargram(snum, tnum, np.float64)
    w, kx = fk_ref.axes(snum, tnum, 1.0e-8, 2.0)
    va = 0.5 * (2.0 / 1.0e-8)
    for mode, dip in itertools.product(fk_ref.MODES, fk_ref.DIPS):
        y = fk_ref.fan_full(x, w, kx, 'hi', va_lo=va, taper=0.25, mode=mode, dip=dip)
        assert np.max(np.abs(y.imag)) <= 1e-15 * np.max(np.abs(y.real)), (mode, dip)
    y = fk_ref.fan_full(x, w, kx, 'hi', va_lo=va, va_hi=8 * va, taper=0.25, dip='down_left')
    assert np.max(np.abs(y.imag)) <= 1e-15 * np.max(np.abs(y.real))


# ---- the weight header at its seams ----------------------------------------------------------------------------------

def seam_elements(pcs, taper):
    """(w, kx, nyq) lists: the axes' zeros, Nyquist elements, the slownesses lo, pc and hi of every edge exactly (w a power of
    two, so that kx = p w and kx / w are exact) with one float64 on either side of each, and both signs of either axis."""
    up, down = np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0)
    els = [(0.0, 0.0, 0), (0.0, 0.5, 0), (0.0, -0.5, 0), (4.0, 0.0, 0), (-4.0, 0.0, 0), (0.0, 0.0, 1)]
    for pc in pcs:
        for p in (pc * (1.0 - taper), pc, pc * (1.0 + taper)):
            for q in (p * down, p, p * up):
                for sw, sk, nyq in itertools.product((1.0, -1.0), (1.0, -1.0), (0, 1)):
                    els.append((sw * 4.0, sk * q * 4.0, nyq))
    w, kx, nyq = zip(*els)
    return np.array(w), np.array(kx), np.array(nyq)


FANS = [dict(va_lo=4.0), dict(va_hi=32.0), dict(va_lo=4.0, va_hi=32.0)]


@pytest.mark.parametrize('taper', [0.5, 0.25, 0.125, 0.0])
@pytest.mark.parametrize('fan', FANS, ids=['lo', 'hi', 'both'])
def test_header_weight_at_the_seams(probe, fan, taper):
    """Edges whose reciprocals are powers of two (pc = 1/4, 1/32) and tapers that are, so lo = pc (1 - taper), pc and hi are
    exact in float64: E is exactly 1 at lo, exactly 0 at hi and 1/2 to 2 u at pc; everywhere else the header agrees with the
    yardstick's longdouble weight to the bar of test_header_weight_elsewhere; with taper = 0 the weight is 0 or 1, the
    yardstick's."""
    pcs = [1.0 / v for v in fan.values()]
    w, kx, nyq = seam_elements(pcs, taper)
    for mode, dip in itertools.product(fk_ref.MODES, fk_ref.DIPS):
        got = header_weight(probe, w, kx, nyq, fan.get('va_lo'), fan.get('va_hi'), taper, mode, dip)
        want = ref_weight(w, kx, nyq, taper=taper, mode=mode, dip=dip, **fan)
        bar = 0.0 if taper == 0.0 else (8.0 / taper + 8.0) * U
        assert np.max(np.abs(got.astype(fk_ref.LD) - want)) <= bar, (mode, dip)
    # the exact values on the down_right side (w > 0, kx < 0), mode pass, dip both: A = E(p; 1/va_lo), B = 1 - E(p; 1/va_hi)
    for name, pc in zip(fan.keys(), pcs):
        other = [q for q in pcs if q != pc]
        p = np.array([pc * (1.0 - taper), pc, pc * (1.0 + taper)])
        got = header_weight(probe, np.full(3, 4.0), -p * 4.0, np.zeros(3), fan.get('va_lo'), fan.get('va_hi'), taper, 'pass', 'both')
        # the other edge is flat there (the fans' tapers do not overlap: 1/32 (1 + 1/2) < 1/4 (1 - 1/2))
        assert not other or (pc * 1.5 < other[0] * 0.5 or other[0] * 1.5 < pc * 0.5)
        e = got if name == 'va_lo' else 1.0 - got
        if taper > 0.0:
            assert e[0] == 1.0 and e[2] == 0.0
            assert abs(e[1] - 0.5) <= 2 * U
        else:
            assert np.all(e == 1.0)     # lo == pc == hi: the hard edge keeps p == pc (the test for p <= lo comes first)


@pytest.mark.parametrize('taper', [0.5, 0.125, 0.01])
def test_header_weight_elsewhere(probe, taper):
    """|w - hi| <= (8 / taper + 8) 2^-53 over random elements, in and around the tapers.

    Where the bar comes from: in the taper W = (1 + cos a) / 2 with a = pi (p - lo) / (hi - lo), so an error da of the
    argument moves W by |sin a| da / 2 <= da / 2.  The float64 slowness p = |kx| / |w| carries half an ulp, at most hi u
    with u = 2^-53, and the division by the taper's width hi - lo = 2 taper pc turns it into (1 + taper) / (2 taper) u of
    the ratio: pi times that, halved, is below 1.6 u / taper.  lo and hi carry up to three roundings each from 1 / va,
    1 -+ taper and their product (none for the powers of two of the seam test), which the same division amplifies to below
    6 u / taper in all; the subtraction, the division, the product with pi, the cosine and the last two operations add a
    few u that no taper amplifies.  8 / taper + 8 leaves a margin over both sums."""
    rng = np.random.default_rng(7)
    n = 4000
    va_lo, va_hi = 3.7, 41.0
    for pc in (1.0 / va_lo, 1.0 / va_hi):
        w = rng.uniform(0.5, 8.0, n) * rng.choice([-1.0, 1.0], n)
        p = pc * rng.uniform(1.0 - 1.5 * taper, 1.0 + 1.5 * taper, n)
        kx = p * np.abs(w) * rng.choice([-1.0, 1.0], n)
        nyq = rng.integers(0, 2, n)
        for mode, dip in itertools.product(fk_ref.MODES, fk_ref.DIPS):
            for fan in (dict(va_lo=va_lo), dict(va_hi=va_hi), dict(va_lo=va_lo, va_hi=va_hi)):
                if len(fan) == 2 and (1.0 / va_hi) * (1.0 + taper) > (1.0 / va_lo) * (1.0 - taper):
                    continue
                got = header_weight(probe, w, kx, nyq, fan.get('va_lo'), fan.get('va_hi'), taper, mode, dip)
                want = ref_weight(w, kx, nyq, taper=taper, mode=mode, dip=dip, **fan)
                assert np.max(np.abs(got.astype(fk_ref.LD) - want)) <= (8.0 / taper + 8.0) * U, (mode, dip, fan)


# ---- refusals, without a device ----------------------------------------------------------------------------------------

class _Dat(object):
    def __init__(self, data, dt=1.0e-8, dx=2.0):
        self.data = data
        self.snum, self.tnum = data.shape
        self.dt = dt
        self.trace_int = np.full(self.tnum, dx)
        self.dist = np.arange(self.tnum) * dx * 1.0e-3
        self.flags = None
        self._dev = None


@pytest.mark.parametrize('kwargs', [
    dict(),                                             # neither edge
    dict(va_lo=0.0), dict(va_lo=-1.0), dict(va_hi=float('inf')), dict(va_lo=float('nan')), dict(va_hi=0.0),
    dict(va_lo=1.0e8, taper=-0.1), dict(va_lo=1.0e8, taper=1.0), dict(va_lo=1.0e8, taper=float('nan')),
    dict(va_lo=1.0e8, va_hi=1.1e8, taper=0.1),          # overlapping tapers
    dict(va_lo=2.0e8, va_hi=1.0e8, taper=0.0),          # the edges the wrong way round
    dict(va_lo=1.0e8, mode='stop'), dict(va_lo=1.0e8, dip='up'),
])
def test_fk_filter_refuses_before_any_device_work(kwargs, monkeypatch):
    from impdar_amd import _hip, fk

    def no_library():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_hip, 'load', no_library)
    dat = _Dat(np.zeros((8, 8)))
    with pytest.raises(ValueError):
        fk.fk_filter(dat, **kwargs)


@pytest.mark.parametrize('shape', [(1, 8), (8, 1)])
def test_fk_refuses_a_single_row_or_column(shape, monkeypatch):
    from impdar_amd import _hip, fk
    monkeypatch.setattr(_hip, 'load', lambda: (_ for _ in ()).throw(AssertionError('the library was reached')))
    dat = _Dat(np.zeros(shape))
    with pytest.raises(ValueError):
        fk.fk_filter(dat, va_lo=1.0e8)
    with pytest.raises(ValueError):
        fk.fk_spectrum(dat)


def test_touching_tapers_are_accepted():
    from impdar_amd import fk
    # (1 / va_hi) (1 + taper) == (1 / va_lo) (1 - taper): only a larger left side is an overlap
    assert fk.check_fan((8, 8), va_lo=4.0, va_hi=4.0, taper=0.0) == (4.0, 4.0, 0.0, 0, 0)


def test_radardata_has_the_methods_and_the_cli_its_command():
    from impdar_amd.bin import impproc, impplot
    from impdar_amd.lib.RadarData import RadarData
    from impdar_amd.lib import plot
    assert callable(RadarData.fk_filter) and callable(RadarData.fk_spectrum) and callable(plot.plot_fk)
    args = impproc._get_args().parse_args(['fk', '--va_lo', '1e8', '--dip', 'down_left', '--mode', 'reject', 'x_raw.mat'])
    assert (args.name, args.va_lo, args.va_hi, args.taper, args.mode, args.dip) == ('fk', 1.0e8, None, 0.1, 'reject', 'down_left')
    assert impproc._out_name('x_raw.mat', None, 1, args.name) == 'x_fk.mat'
    assert impplot._get_args().parse_args(['fk', 'x.mat']).func is impplot.plot_fk
