#!/usr/bin/env python3
"""Generate the ``Q*`` golden vectors of the quad-pol chain by running the REFERENCE's ``rotational_transform``,
``coherence2d(force_python=True)`` and ``phase_gradient2d`` (``src/impdar/lib/ApresData/_QuadPolProcessing.py``),
imported -- never copied.  ``impdar.lib.ApresData`` imports ``h5py`` for its loaders; where that is not installed
an empty stand-in module is registered under the name before the import, which the three steps never touch.
``flags.cpe`` is set False: the cpe gathers are the tests' own matter.

Every file stores the four measured vectors, ``range``, ``dt``, the arguments, the reference's ``thetas``, images,
``chhvv`` and ``dphi_dz``, the window sizes it used, and ``dphi_ref_err``: max |dphi_dz - the same formula evaluated
in longdouble on the reference's chhvv| / max |that|, the reference's own rounding, to which the tests scale their
bar (for the filtered case the filter stays SciPy's float64 one and what follows it is longdouble).  No committed
file may pass 1 MiB, so the two large cases leave images out: Q4 keeps HH and VV, Q6 the two final products.
``QZ_errors`` holds the reference's exception types and messages.

  Q1  257 x 24, nrange 23, ntheta 2: amplitudes 10**(-3 j / n) x complex normal, svv a phase-ramped shh plus noise,
      small correlated cross terms; range on a 4.2 m step (not bit-uniform: numpy.gradient's uneven formula)
  Q2  64 x 8, nrange 100: every window clipped at both ends; integer range (the uniform formula)
  Q3  130 x 5, nrange 1, ntheta 5: the window wraps the whole circle
  Q4  400 x 40, nrange 95, ntheta 10: Q1's recipe on a jittered range axis
  Q5  Q1 with rows 90 ... 169 of all four vectors zero (shh and svv alone would leave the cross terms in every
      window): NaN where a window holds nothing else
  Q6  the first 1200 bins of the reference's test/input_data/quadpol_fujita.mat, 40 azimuths, default windows
  Q7  Q1 with filt='lowpass', Wn a tenth of Nyquist

Usage:  python tests/golden/make_golden_quadpol.py <root of the reference's source tree>
"""
import contextlib
import io
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

from impdar.lib.ApresData import ApresQuadPol                      # noqa: E402
from impdar.lib.ImpdarError import ImpdarError                     # noqa: E402

import quadpol_ref                                                 # noqa: E402

DT = 1.0e-8


def vectors(n, seed):
    rng = np.random.RandomState(seed)

    def cnormal():
        return rng.standard_normal(n) + 1j * rng.standard_normal(n)
    amp = 10. ** (-3. * np.arange(n) / n)
    shh = amp * cnormal()
    svv = shh * np.exp(1j * 0.03 * np.arange(n)) + 0.3 * amp * cnormal()
    shv = 0.05 * amp * (cnormal() + (2. + 2.j))          # the offset keeps the reference's sign check of the cross terms quiet
    svh = shv + 0.01 * amp * cnormal()
    return shh, shv, svh, svv


def quadpol(vecs, rng_axis, dt=DT):
    qp = ApresQuadPol(None)
    qp.shh, qp.shv, qp.svh, qp.svv = [np.array(v, dtype=np.cdouble) for v in vecs]
    qp.range = np.array(rng_axis, dtype=np.float64)
    qp.snum = len(qp.range)
    qp.dt = dt
    qp.flags.cpe = False
    return qp


def make(name, vecs, rng_axis, n_thetas, delta_theta, delta_range, filt=None, Wn=0, keep=('HH', 'HV', 'VH', 'VV', 'chhvv', 'dphi_dz')):
    qp = quadpol(vecs, rng_axis)
    g = {'in_' + k: getattr(qp, k).copy() for k in ('shh', 'shv', 'svh', 'svv')}
    g.update(range=qp.range.copy(), dt=qp.dt, n_thetas=n_thetas, delta_theta=delta_theta, delta_range=delta_range,
             filt='' if filt is None else filt, Wn=Wn)
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(invalid='ignore', divide='ignore'):
        qp.rotational_transform(n_thetas=n_thetas)
        qp.coherence2d(delta_theta=delta_theta, delta_range=delta_range, force_python=True)
        qp.phase_gradient2d(filt=filt, Wn=Wn)
    g['nrange'] = int(delta_range // abs(qp.range[0] - qp.range[1]))
    g['ntheta'] = int(delta_theta // abs(qp.thetas[0] - qp.thetas[1]))
    g['thetas'] = qp.thetas
    spec = None
    if filt is not None:
        from impdar_amd.quadpol import lowpass_spec
        spec = lowpass_spec(Wn, 1. / qp.dt)
    exact = quadpol_ref.dphi_dz(qp.chhvv, qp.range, spec, dtype=np.longdouble)
    g['dphi_ref_err'] = quadpol_ref.rel_err(qp.dphi_dz.astype(np.longdouble), exact)
    for k in keep:
        g[k] = getattr(qp, k)
    for k in ('rotation', 'coherence', 'phasegradient'):
        g['flags_' + k] = np.asarray(getattr(qp.flags, k))
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **g)
    print('%-28s %4d x %-3d nrange %3d ntheta %2d  NaN %5d  dphi_ref_err %.2e  %7d bytes'
          % (name, len(qp.range), n_thetas, g['nrange'], g['ntheta'], int(np.isnan(qp.chhvv).sum()), g['dphi_ref_err'],
             os.path.getsize(path)))
    assert os.path.getsize(path) < 1 << 20, name


def errors():
    labels, types_, messages = [], [], []

    def record(label, fn):
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                fn()
        except (ImpdarError, ValueError, TypeError) as e:
            labels.append(label), types_.append(type(e).__name__), messages.append(str(e))
        else:
            raise AssertionError(label)
    v = vectors(40, 9)
    ax = np.arange(40.) * 2.
    record('coherence_before_rotation', lambda: quadpol(v, ax).coherence2d(force_python=True))
    qp = quadpol(v, ax)
    qp.rotational_transform(n_thetas=12)
    record('gradient_before_coherence', lambda: qp.phase_gradient2d())
    qp.coherence2d(delta_range=10., force_python=True)
    record('filter_unknown', lambda: qp.phase_gradient2d(filt='highpass'))
    flipped = (v[0], v[1], -v[2], v[3])
    record('cross_pol_opposite_sign', lambda: quadpol(flipped, ax).rotational_transform(n_thetas=12))
    record('flip_force', lambda: quadpol(v, ax).rotational_transform(n_thetas=12, flip_force=True))
    out = {'label': np.array(labels), 'exc_type': np.array(types_), 'message': np.array(messages)}
    for k, x in zip(('shh', 'shv', 'svh', 'svv'), flipped):
        out['flipped_' + k] = x
    out['range'] = ax
    # what the two flips leave behind
    for which in ('HV', 'VH'):
        qp = quadpol(flipped, ax)
        qp.rotational_transform(n_thetas=12, cross_pol_flip=which)
        out['flip_%s_HH' % which], out['flip_%s_HV' % which] = qp.HH, qp.HV
        out['flip_%s_shv' % which], out['flip_%s_svh' % which] = qp.shv, qp.svh
    np.savez_compressed(os.path.join(HERE, 'QZ_errors.npz'), **out)
    for row in zip(labels, types_, messages):
        print('QZ_errors: %s %s %r' % row)


def main():
    dth = lambda n_thetas: np.pi / (n_thetas - 1)                  # noqa: E731
    q1 = vectors(257, 1)
    ax1 = np.arange(257) * 4.2
    default = 20.0 * np.pi / 180.
    make('Q1_decay_257x24', q1, ax1, 24, default, 100.)
    make('Q2_clipped_both_ends_64x8', vectors(64, 2), np.arange(64.), 8, 1.5 * dth(8), 100.)
    make('Q3_whole_circle_130x5', vectors(130, 3), np.arange(130) * 0.7, 5, 5.5 * dth(5), 1.5 * 0.7)
    jitter = 1.05 * (np.arange(400) + 0.2 * np.sin(np.arange(400) * 1.7))
    jitter[:2] = [0., 1.05]
    make('Q4_decay_400x40_uneven_range', vectors(400, 4), jitter, 40, 10.5 * dth(40), 100., keep=('HH', 'VV', 'chhvv', 'dphi_dz'))
    zeroed = [v.copy() for v in q1]
    for v in zeroed:
        v[90:170] = 0.
    make('Q5_zero_rows_nan_257x24', zeroed, ax1, 24, default, 100.)
    from scipy.io import loadmat
    mat = loadmat(os.path.join(REF, 'test', 'input_data', 'quadpol_fujita.mat'))
    fuj = [np.squeeze(mat[k])[:1200] for k in ('shh', 'shv', 'svh', 'svv')]
    make('Q6_fujita_1200x40', fuj, np.squeeze(mat['range'])[:1200], 40, default, 100., keep=('chhvv', 'dphi_dz'))
    make('Q7_lowpass_257x24', q1, ax1, 24, default, 100., filt='lowpass', Wn=0.1 * 0.5 / DT)
    errors()


if __name__ == '__main__':
    main()
