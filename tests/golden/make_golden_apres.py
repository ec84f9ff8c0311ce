#!/usr/bin/env python3
"""Generate the ``AP_*`` golden vectors of ApRES range conversion, stacking and phase difference by running the
REFERENCE's ``apres_range``, ``stacking`` (``src/impdar/lib/ApresData/_ApresDataProcessing.py``) and ``phase_diff``
(``_TimeDiffProcessing.py``), imported -- never copied.  ``impdar.lib.ApresData`` imports ``h5py`` for its loaders;
where that is not installed an empty stand-in module is registered under the name before the import, which the three
steps never touch.  (The files carry the prefix ``AP_`` because other suites collect every golden file whose name
starts with ``S`` or ``P1``.)

Raw chirps: a DC offset 1.25 + white noise 0.3 + three tones (0.013, 0.071 and 0.19 cycles per sample, amplitudes 1,
0.5, 0.2) with a random phase per chirp, drawn again until bin 0 of every chirp is positive (see ``chirps``).  The
header is an instrument's: 200 MHz bandwidth around 300 MHz in a second, ice of relative permittivity 3.18.

Range conversion, ``bnum x cnum x snum``, ``p``, ``max_range``:
  A1  2 x 3 x 1001, p 2, 150 m: odd snum, N = 2002 = 2 7 11 13, n = 714 of 1001
  A2  1 x 4 x 362, p 3, 60 m: N = 1086 = 2 3 181, a large prime factor, 0 < n < nf
  A3  3 x 2 x 1001, p 1, 100 m: odd N
  A4  3 x 2 x 1024, p 1, 100 m: a power of two, n = 238 of 512
  A5  A2 with max_range 1e9: every bin within it, so n = argmin of an all-True array = 0
  A6  5 x 2 x 64, p 1, 1 m: n = 3 < bnum, the crop of Rfine on the burst axis
  A7  A1 with winfun 'hanning'
Each stores the raw chirps, the arguments, the header constants, every product of the reference, ``spec_norm`` (per
chirp the 2-norm of the full nf-bin spectrum, from the restatement in ``apres_ref.py`` that the kept bins pin to the
reference), ``ref_err`` (the relative 2-norm distance of the reference's kept bins from a direct DFT sum in long
double, in units of u = 2**-53; NaN where no bin is kept) and ``data_min_over_max``.

Stacking:  S1 4 x 5 x 300 real, num_chirps 5 (per burst);  S2 the same, num_chirps 7 (across bursts);  S3 the default
on A1's converted complex data.
Phase difference:  P1 two stacked A1 profiles, the second rotated by a phase ramp with 1 % noise, win 20, step 7;
P2 odd win 21, step 1;  P3 P1 with samples 300 ... 359 of both vectors zero (NaN windows);  P4 P1 with range_ext.
``AP_AZ_errors`` holds the reference's exception types and messages.

Usage:  python tests/golden/make_golden_apres.py <root of the reference's source tree>
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('IMPDAR_REFERENCE_ROOT')
if not REF:
    sys.exit(__doc__)
sys.path.insert(0, os.path.join(REF, 'src'))
try:
    import h5py          # noqa: F401
except ImportError:
    sys.modules['h5py'] = types.ModuleType('h5py')

from impdar.lib.ApresData import ApresData, ApresTimeDiff           # noqa: E402

import apres_ref                                                   # noqa: E402
from impdar_amd import apres as apm                                # noqa: E402

HEADER = dict(fs=4.e4, bandwidth=2.e8, fc=3.e8, chirp_grad=2. * np.pi * 2.e8, er=3.18, ci=3.e8 / np.sqrt(3.18))
HEADER['lambdac'] = HEADER['ci'] / HEADER['fc']


def chirps(bnum, cnum, snum, seed, positive_bin0=True):
    """The recipe above from ``RandomState(seed)``, ``seed + 1000`` ... : the first draw whose chirps all have a
    positive bin 0 under both windows used here.  Bin 0 of a real chirp is real; a negative one sits on atan2's branch
    cut, where the sign of the reference's +-pi is the rounding noise of its transform (its complex FFT leaves 1e-15
    in the imaginary part) and no other transform can be asked to share it."""
    t = np.arange(snum)
    while True:
        rng = np.random.RandomState(seed)
        x = 1.25 + 0.3 * rng.standard_normal((bnum, cnum, snum))
        for f, a in ((0.013, 1.), (0.071, 0.5), (0.19, 0.2)):
            x += a * np.cos(2 * np.pi * f * t + rng.uniform(-np.pi, np.pi, (bnum, cnum, 1)))
        y = x - x.mean(axis=2, keepdims=True)
        if not positive_bin0 or min((y * w(snum)).sum(axis=2).min() for w in (np.blackman, np.hanning)) > 1e-3 * np.abs(y).sum(axis=2).max():
            return x
        seed += 1000


def apres(raw):
    dat = ApresData(None)
    dat.data = np.array(raw)
    dat.bnum, dat.cnum, dat.snum = raw.shape
    for k, v in HEADER.items():
        setattr(dat.header, k, v)
    return dat


def save(name, g):
    path = os.path.join(HERE, 'AP_' + name + '.npz')
    np.savez_compressed(path, **g)
    assert os.path.getsize(path) < 1 << 20, name
    return os.path.getsize(path)


def make_range(name, raw, p, max_range, winfun='blackman'):
    dat = apres(raw)
    dat.apres_range(p, max_range, winfun=winfun)
    g = {'raw': raw, 'p': p, 'max_range': max_range, 'winfun': winfun}
    g.update({'header_' + k: v for k, v in HEADER.items()})
    for k in ('data', 'spec', 'Rcoarse', 'Rfine', 'phiref'):
        g[k] = getattr(dat, k)
    g.update(snum=dat.snum, flags_range=dat.flags.range, data_dtype=str(dat.data_dtype))
    t = apm.range_tables(apres(raw), p, max_range, winfun)
    rows = raw.reshape(-1, raw.shape[2])
    N = p * raw.shape[2]
    full = np.fft.rfft((rows - rows.mean(axis=1, keepdims=True)) * t.win, N, axis=1)[:, :t.nf] * t.scale_mul / t.scale_div
    g['spec_norm'] = np.linalg.norm(full, axis=1)
    if t.n:
        ld = rows.astype(np.longdouble)
        y = (ld - ld.mean(axis=1, keepdims=True)) * t.win.astype(np.longdouble)
        exact = apres_ref.dft_exact(y, N, t.n) * np.longdouble(t.scale_mul) / np.longdouble(t.scale_div)
        got = dat.spec.reshape(-1, t.n).astype(np.clongdouble)
        g['ref_err'] = float(np.max(np.linalg.norm(got - exact, axis=1) / np.linalg.norm(exact, axis=1)) / apres_ref.U)
        mag = np.abs(dat.data)
        g['data_min_over_max'] = float(mag.min() / mag.max())
    else:
        g['ref_err'] = np.nan
        mag = np.abs(t.comp * full)
        g['data_min_over_max'] = float(mag.min() / mag.max())
    size = save(name, g)
    print('%-26s %s p %d  N %5d  n %4d of %4d  Rfine %s  ref_err %.2f u  min/max |data| %.1e  %7d bytes'
          % (name, raw.shape, p, N, t.n, t.nf, dat.Rfine.shape, g['ref_err'], g['data_min_over_max'], size))
    return dat


def make_stack(name, dat, data_in, num_chirps):
    g = {'data_in': np.array(data_in), 'num_chirps': -1 if num_chirps is None else num_chirps}
    dat.stacking(num_chirps)
    g.update(data=dat.data, bnum=dat.bnum, cnum=dat.cnum, flags_stack=dat.flags.stack)
    size = save(name, g)
    print('%-26s %s -> %s %s flags.stack %r  %7d bytes' % (name, g['data_in'].shape, dat.data.shape, dat.data.dtype, dat.flags.stack, size))
    return dat


def make_diff(name, s1, s2, rng_axis, win, step, range_ext=None):
    diff = ApresTimeDiff(None)
    diff.data, diff.data2, diff.range = s1.copy(), s2.copy(), rng_axis.copy()
    diff.snum = len(s1)
    with np.errstate(invalid='ignore', divide='ignore'):
        diff.phase_diff(win, step, range_ext=range_ext)
    g = {'data': s1, 'data2': s2, 'range': rng_axis, 'win': win, 'step': step, 'ds': diff.ds, 'co': diff.co,
         'flags_phase_diff': np.asarray(diff.flags.phase_diff)}
    if range_ext is not None:
        g['range_ext'] = range_ext
    size = save(name, g)
    print('%-26s %d samples win %d step %d: %d windows, %d NaN  %7d bytes'
          % (name, len(s1), win, step, len(diff.co), int(np.isnan(diff.co.real).sum()), size))


def errors():
    labels, types_, messages = [], [], []

    def record(label, fn):
        try:
            fn()
        except (ValueError, TypeError) as e:
            labels.append(label), types_.append(type(e).__name__), messages.append(str(e))
        else:
            raise AssertionError(label)
    raw = chirps(1, 2, 64, 9)
    dat = apres(raw)
    dat.apres_range(1, 10.)
    record('range_twice', lambda: dat.apres_range(1, 10.))
    record('window_unknown', lambda: apres(raw).apres_range(1, 10., winfun='boxcar'))
    record('window_kaiser', lambda: apres(raw).apres_range(1, 10., winfun='kaiser'))
    save('AZ_errors', {'label': np.array(labels), 'exc_type': np.array(types_), 'message': np.array(messages), 'raw': raw})
    for row in zip(labels, types_, messages):
        print('AP_AZ_errors: %s %s %r' % row)


def main():
    a1 = chirps(2, 3, 1001, 1)
    a2 = chirps(1, 4, 362, 2)
    d1 = make_range('A1_odd_snum_2x3x1001_p2', a1, 2, 150.)
    make_range('A2_prime181_1x4x362_p3', a2, 3, 60.)
    make_range('A3_odd_N_3x2x1001_p1', chirps(3, 2, 1001, 3), 1, 100.)
    make_range('A4_pow2_3x2x1024_p1', chirps(3, 2, 1024, 4), 1, 100.)
    make_range('A5_all_within_n0_1x4x362_p3', a2, 3, 1.e9)
    make_range('A6_n3_below_bnum_5x2x64_p1', chirps(5, 2, 64, 6), 1, 1.)
    make_range('A7_hanning_2x3x1001_p2', a1, 2, 150., winfun='hanning')

    s = chirps(4, 5, 300, 7, positive_bin0=False)          # (stacking reads no phase)
    make_stack('S1_per_burst_4x5x300', apres(s), s, 5)
    make_stack('S2_across_bursts_7_4x5x300', apres(s), s, 7)
    converted = d1.data.copy()
    d1 = make_stack('S3_default_complex_2x3x714', d1, converted, None)

    rng = np.random.RandomState(8)
    s1 = np.squeeze(d1.data).copy()
    n = len(s1)
    noise = 0.01 * np.abs(s1).mean() * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    s2 = s1 * np.exp(1j * 0.002 * np.arange(n)) + noise
    ax = d1.Rcoarse.copy()
    make_diff('P1_win20_step7', s1, s2, ax, 20, 7)
    make_diff('P2_odd_win21_step1', s1, s2, ax, 21, 1)
    z1, z2 = s1.copy(), s2.copy()
    z1[300:360] = 0.
    z2[300:360] = 0.
    make_diff('P3_zeros_nan_win20_step7', z1, z2, ax, 20, 7)
    make_diff('P4_range_ext_win20_step7', s1, s2, ax, 20, 7, range_ext=ax * 1.01 + 0.5)
    errors()


if __name__ == '__main__':
    main()
