#!/usr/bin/env python3
"""Generate the ``AF_*`` golden vectors of the three full ApRES flows by running the REFERENCE's ``find_cpe``,
``power_anomaly``, ``lowpass``, ``phase_gradient_to_fabric``, ``azimuthal_rotation``
(``src/impdar/lib/ApresData/_QuadPolProcessing.py``), ``phase_unwrap``, ``range_diff``, ``strain_rate``, ``bed_pick``
(``_TimeDiffProcessing.py``) and ``phase_uncertainty`` (``_ApresDataProcessing.py``), imported -- never copied -- with
the same ``h5py`` stand-in as ``make_golden_quadpol.py``, whose ``vectors()`` recipe and holder the quad-pol cases
reuse.  (The files carry the prefix ``AF_`` because other suites collect every golden file whose name starts with
``Q`` or ``C``.)

Quad-pol, cpe axis (window pi/4 ... 3 pi/4):
  QC1  257 x 24, Wn a tenth of Nyquist; coherence and phase gradient done first, so ``find_cpe`` makes both gathers:
       stores ``chhvv_cpe``, ``dphi_dz_cpe`` and ``e2e1``
  QC2  400 x 40 on the jittered range axis, the same Wn; rotation only: no gathers
  QC3  1200 x 100, the same Wn; rotation only; the three images do not fit a committed file, so every 40th row is kept
       (``rows_kept``)
  QC4  QC1's input at Wn = 0.004 of Nyquist, a low corner; rotation only
The input is drawn again (seed + 1000 ...) until no element of HV^2 lies within 1e-9 |HV^2| of the negative real axis:
there the sign of the imaginary part of the reference's log10 is rounding noise.  Each file stores the four vectors,
``range``, ``dt``, the arguments, the reference's ``HV``, ``power_anomaly`` and its filtered image (complex128), ``cpe_idxs``,
``cpe``, ``idx_start``, ``idx_stop`` and
  pa_ref_err  max |reference's anomaly - the same formula in longdouble|, real and imaginary part apart
  filt_sens   max |filtered(anomaly of HV (1 + 4 u N(0, 1))) - filtered(anomaly of HV)|: what input rounding does
  gap         per row, second-smallest minus smallest real part of the filtered anomaly in the window
and the script checks that no index moves under that perturbation, that the real-part argmin is the lexicographic
one, and that every gap exceeds 1000 filt_sens.  QC1 also stores three ``azimuthal_rotation`` results.

Time difference: two synthetic acquisitions of 6000 bins on a 0.21 m step: complex normal times an envelope whose
power decays 2.5 decades along the record, a bed return near bin 4200 (a Gaussian of sigma 260 bins, 30 x the local
level) followed by a floor 50 x lower; the second is the first with phase -4 pi (-2e-3 range) / lambdac; 2 % noise
of the local level on each; ``unc1``, ``unc2`` given.
  TD1  win 20, step 20, thresh 0.95, strain_window (200, 800)
  TD2  TD1 with uncertainty='CR'
  TD3  TD1 with unc1 = None: no w_err
Each stores the reference's ``co``, ``ds``, ``phi``, ``w``, ``w_err``, ``eps_zz``, ``w0``, ``bed``, the wrap count and
``strain_sens``: |change of (eps_zz, w0)| when ``co`` is perturbed by 4 u in modulus and phase.

  AU1  the first acquisition as a (1, 1, 6000) stack, bed_range 900, ``np.random.seed(5)`` (the next seed at which no
       |noise_orth / |data|| lies within 1e-9 of 1): ``noise_phase`` as drawn, ``uncertainty``, ``x``.
  CZ_errors  the reference's exception types and messages.

Usage:  python tests/golden/make_golden_apres_flows.py <root of the reference's source tree>
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_quadpol as mq                                   # noqa: E402  (sets up the paths and the stand-in)
from make_golden_apres import HEADER                               # noqa: E402

from impdar.lib.ApresData import ApresData, ApresTimeDiff, _QuadPolProcessing as refqp   # noqa: E402
from impdar.lib.ImpdarError import ImpdarError                     # noqa: E402

U = 2.0 ** -53
DT = mq.DT


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def save(name, g):
    path = os.path.join(HERE, 'AF_' + name + '.npz')
    np.savez_compressed(path, **g)
    assert os.path.getsize(path) < 1 << 20, (name, os.path.getsize(path))
    return os.path.getsize(path)


# ------------------------------------------------------------------------------------------------ quad-pol
def rotated(n, seed, rng_axis, n_thetas):
    """The first draw of the recipe whose HV^2 keeps clear of the negative real axis."""
    while True:
        qp = mq.quadpol(mq.vectors(n, seed), rng_axis)
        vecs = [getattr(qp, k).copy() for k in ('shh', 'shv', 'svh', 'svv')]
        with quiet():
            qp.rotational_transform(n_thetas=n_thetas)
        sq = qp.HV.astype(np.clongdouble) ** 2
        if not np.any((sq.real < 0) & (np.abs(sq.imag) < 1e-9 * np.abs(sq))):
            return qp, vecs, seed
        seed += 1000


def anomaly_exact(HV):
    z = HV.astype(np.clongdouble)
    P = np.longdouble(10.) * np.log10(z * z)
    return P - np.nanmean(P, axis=1)[:, None]


def make_qc(name, n, seed, rng_axis, n_thetas, wn_of_nyquist, products_first=False, rows_kept=None, extra=None):
    qp, vecs, seed = rotated(n, seed, rng_axis, n_thetas)
    Wn = wn_of_nyquist * 0.5 / DT
    g = dict(zip(('in_shh', 'in_shv', 'in_svh', 'in_svv'), vecs))
    g.update(range=qp.range.copy(), dt=qp.dt, n_thetas=n_thetas, Wn=Wn, seed=seed, products_first=products_first)
    if products_first:
        with quiet():
            qp.coherence2d(force_python=True)
            qp.phase_gradient2d()
    pa = refqp.power_anomaly(qp.HV.copy())
    filt = refqp.lowpass(pa.copy(), Wn, 1. / qp.dt)
    qp.find_cpe(Wn=Wn)
    i0, i1 = int(np.argmin(abs(qp.thetas - np.pi / 4.))), int(np.argmin(abs(qp.thetas - 3. * np.pi / 4.)))
    window = filt[:, i0:i1]
    np.testing.assert_array_equal(np.argmin(window.real, axis=1) + i0, qp.cpe_idxs)        # real part decides
    two = np.sort(window.real, axis=1)[:, :2]
    gap = two[:, 1] - two[:, 0]
    exact = anomaly_exact(qp.HV)
    err = pa.astype(np.clongdouble) - exact
    pa_ref_err = np.array([float(np.max(np.abs(err.real))), float(np.max(np.abs(err.imag)))])
    rng = np.random.RandomState(seed + 7)
    pert = qp.HV * (1. + 4. * U * rng.standard_normal(qp.HV.shape))
    filt2 = refqp.lowpass(refqp.power_anomaly(pert), Wn, 1. / qp.dt)
    filt_sens = float(np.max(np.abs(filt2 - filt)))
    np.testing.assert_array_equal(np.array([np.argmin(r) for r in filt2[:, i0:i1]]) + i0, qp.cpe_idxs)
    assert gap.min() > 1000 * filt_sens, (name, gap.min(), filt_sens)
    keep = slice(None) if rows_kept is None else rows_kept
    g.update(thetas=qp.thetas, HV=qp.HV[keep], power_anomaly=pa[keep], filtered=filt[keep], cpe_idxs=qp.cpe_idxs, cpe=qp.cpe, idx_start=i0,
             idx_stop=i1, pa_ref_err=pa_ref_err, filt_sens=filt_sens, gap=gap, flags_cpe=qp.flags.cpe,
             has_chhvv_cpe=hasattr(qp, 'chhvv_cpe'), has_dphi_dz_cpe=hasattr(qp, 'dphi_dz_cpe'))
    if rows_kept is not None:
        g['rows_kept'] = np.arange(n)[rows_kept]
    if products_first:
        refqp.phase_gradient_to_fabric(qp)
        g.update(chhvv_cpe=qp.chhvv_cpe, dphi_dz_cpe=qp.dphi_dz_cpe, e2e1=qp.e2e1)
    if extra:
        extra(qp, g)
    size = save(name, g)
    print('%-22s %4d x %-3d seed %5d Wn %.3g Nyq  window [%d, %d)  min gap %.2e  filt_sens %.1e  pa_ref_err %.1e %.1e  %7d bytes'
          % (name, n, n_thetas, seed, wn_of_nyquist, i0, i1, gap.min(), filt_sens, pa_ref_err[0], pa_ref_err[1], size))


def rolls(qp, g):
    image = np.arange(5 * len(qp.thetas), dtype=float).reshape(5, -1)
    for label, azi in (('neg', -0.3), ('pos', 0.4), ('zero', 0.)):
        thetas = qp.thetas.copy()
        g['roll_%s' % label] = refqp.azimuthal_rotation(image.copy(), thetas, azi)
        g['roll_%s_azi' % label] = azi
        g['roll_%s_thetas' % label] = thetas


# ------------------------------------------------------------------------------------------------ time difference
N_TD, STEP_TD, BED = 6000, 0.21, 4200


def acquisitions(seed):
    rng = np.random.RandomState(seed)

    def cnormal():
        return rng.standard_normal(N_TD) + 1j * rng.standard_normal(N_TD)
    j = np.arange(N_TD)
    base = 10. ** (-1.25 * j / N_TD)
    env = np.where(j < BED, base, base / 50.) + 30. * base[BED] * np.exp(-(j - BED) ** 2. / (2. * 260. ** 2.))
    ax = j * STEP_TD
    s1 = env * cnormal()
    s2 = s1 * np.exp(1j * (-4. * np.pi * (-2e-3 * ax) / HEADER['lambdac']))
    s1 = s1 + 0.02 * env * cnormal()
    s2 = s2 + 0.02 * env * cnormal()
    unc1 = 0.02 * (1. + 0.5 * rng.uniform(size=N_TD))
    unc2 = 0.02 * (1. + 0.5 * rng.uniform(size=N_TD))
    return s1, s2, ax, unc1, unc2


def time_diff(s1, s2, ax, unc1, unc2):
    diff = ApresTimeDiff(None)
    diff.data, diff.data2, diff.range = s1.copy(), s2.copy(), ax.copy()
    diff.snum = len(s1)
    diff.unc1 = None if unc1 is None else unc1.copy()
    diff.unc2 = None if unc2 is None else unc2.copy()
    for k, v in HEADER.items():
        setattr(diff.header, k, v)
    return diff


def after_phase_diff(diff, args, co=None):
    win, step, thresh, strain_window, uncertainty = args
    if co is not None:
        diff.co = co
    with quiet():
        diff.phase_unwrap(win, thresh)
        diff.range_diff(uncertainty=uncertainty)
        diff.strain_rate(strain_window=strain_window, w_surf=-0.15)
        diff.bed_pick()


def make_td(name, acq, uncertainty='noise_phasor', with_unc=True):
    s1, s2, ax, unc1, unc2 = acq
    if not with_unc:
        unc1 = unc2 = None
    args = (20, 20, 0.95, (200, 800), uncertainty)
    diff = time_diff(s1, s2, ax, unc1, unc2)
    diff.phase_diff(args[0], args[1])
    co = diff.co.copy()
    after_phase_diff(diff, args)
    wraps = int(np.sum(np.abs(np.diff(np.round((diff.phi - np.angle(co)) / (2. * np.pi)))) > 0))
    rng = np.random.RandomState(11)
    again = time_diff(s1, s2, ax, unc1, unc2)
    again.phase_diff(args[0], args[1])
    after_phase_diff(again, args, co=co * (1. + 4. * U * (rng.standard_normal(co.shape) + 1j * rng.standard_normal(co.shape))))
    strain_sens = np.array([abs(again.eps_zz - diff.eps_zz), abs(again.w0 - diff.w0)])
    dphi = np.abs(np.diff(np.angle(co)))
    g = {'data': s1, 'data2': s2, 'range': ax, 'win': args[0], 'step': args[1], 'thresh': args[2],
         'strain_window': np.array(args[3]), 'w_surf': -0.15, 'uncertainty': uncertainty, 'with_unc': with_unc,
         'co': co, 'ds': diff.ds, 'phi': diff.phi, 'w': diff.w, 'eps_zz': diff.eps_zz, 'w0': diff.w0, 'bed': diff.bed,
         'wraps': wraps, 'strain_sens': strain_sens, 'flags_phase_diff': np.asarray(diff.flags.phase_diff),
         'has_w_err': hasattr(diff, 'w_err'), 'min_dphi_from_pi': float(np.min(np.abs(dphi - np.pi))),
         'min_co_from_thresh': float(np.min(np.abs(np.abs(co) - args[2])))}
    g.update({'header_' + k: v for k, v in HEADER.items()})
    if with_unc:
        g.update(unc1=unc1, unc2=unc2, w_err=diff.w_err)
    assert g['min_dphi_from_pi'] > 1. and g['min_co_from_thresh'] > 0.01, (g['min_dphi_from_pi'], g['min_co_from_thresh'])
    size = save(name, g)
    print('%-22s %d windows, %d wraps, eps_zz %.5e w0 %.3e, bed sample %d coherence %.4f, |dphi| - pi >= %.2f, ||co| - thresh| >= '
          '%.3f, strain_sens %.1e %.1e  %7d bytes' % (name, len(co), wraps, diff.eps_zz, diff.w0, int(diff.bed[0]), diff.bed[2],
                                                     g['min_dphi_from_pi'], g['min_co_from_thresh'], strain_sens[0],
                                                     strain_sens[1], size))


# ------------------------------------------------------------------------------------------------ uncertainty
def stacked(s1, ax):
    dat = ApresData(None)
    dat.data = s1.reshape(1, 1, -1).copy()
    dat.bnum, dat.cnum, dat.snum = dat.data.shape
    dat.Rcoarse = ax.copy()
    dat.flags.range = 4000.
    return dat


def make_au(name, s1, ax, bed_range=900., seed=5):
    while True:
        dat = stacked(s1, ax)
        np.random.seed(seed)
        state = np.random.get_state()
        with np.errstate(invalid='ignore'):
            dat.phase_uncertainty(bed_range)
        np.random.set_state(state)
        meas = np.squeeze(dat.data)
        noise_phase = np.random.uniform(-np.pi, np.pi, np.shape(meas))
        median_mag = np.nanmedian(abs(meas[np.argwhere(dat.Rcoarse > bed_range)]))
        noise = median_mag * (np.cos(noise_phase) + 1j * np.sin(noise_phase))
        x = median_mag * np.sin(np.angle(meas) - np.angle(noise)) / np.abs(meas)
        with np.errstate(invalid='ignore'):
            np.testing.assert_array_equal(np.abs(np.arcsin(x)), dat.uncertainty)
        if np.min(np.abs(np.abs(x) - 1.)) > 1e-9:
            break
        seed += 1
    g = {'data': dat.data, 'Rcoarse': dat.Rcoarse, 'bed_range': bed_range, 'seed': seed, 'noise_phase': noise_phase,
         'uncertainty': dat.uncertainty, 'x': x, 'flags_uncertainty': dat.flags.uncertainty}
    size = save(name, g)
    print('%-22s seed %d: %d NaN of %d, min ||x| - 1| %.2e  %7d bytes'
          % (name, seed, int(np.isnan(dat.uncertainty).sum()), x.size, np.min(np.abs(np.abs(x) - 1.)), size))


# ------------------------------------------------------------------------------------------------ errors
def errors(acq):
    labels, types_, messages = [], [], []

    def record(label, fn, only=None):
        try:
            with quiet(), np.errstate(all='ignore'):
                fn()
        except (ImpdarError, ValueError, TypeError, AttributeError, IndexError) as e:
            assert only is None or type(e) is only, (label, e)
            labels.append(label), types_.append(type(e).__name__), messages.append(str(e))
        else:
            raise AssertionError(label)
    v = mq.vectors(40, 9)
    ax = np.arange(40.) * 2.
    record('cpe_before_rotation', lambda: mq.quadpol(v, ax).find_cpe())
    qp = mq.quadpol(v, ax)
    with quiet():
        qp.rotational_transform(n_thetas=12)
    nyq = 0.5 / DT
    record('cpe_empty_window', lambda: qp.find_cpe(Wn=0.1 * nyq, rad_start=2., rad_end=1.))
    record('cpe_wn_above_nyquist', lambda: qp.find_cpe(Wn=1.5 * nyq))
    record('cpe_wn_zero', lambda: qp.find_cpe(Wn=0.))
    record('fabric_before_gradient', lambda: refqp.phase_gradient_to_fabric(qp))
    short = mq.quadpol(mq.vectors(12, 9), np.arange(12.) * 2.)
    with quiet():
        short.rotational_transform(n_thetas=12)
    record('cpe_twelve_rows', lambda: short.find_cpe(Wn=0.1 * nyq))

    s1, s2, axis, unc1, unc2 = acq
    args = (20, 20, 0.95, (200, 800), 'noise_phasor')
    diff = time_diff(s1, s2, axis, unc1, unc2)
    diff.flags.phase_diff = None
    record('unwrap_before_phase_diff', lambda: diff.phase_unwrap())
    diff = time_diff(s1, s2, axis, unc1, unc2)
    diff.phase_diff(20, 20)
    record('range_diff_before_unwrap', lambda: diff.range_diff())
    del diff.w
    record('strain_before_range_diff', lambda: diff.strain_rate())
    flat = time_diff(np.ones(N_TD) + 0j, np.ones(N_TD) + 0j, axis, unc1, unc2)
    flat.phase_diff(20, 20)
    record('bed_no_peaks', lambda: flat.bed_pick(), only=ValueError)
    apart = time_diff(s1, np.concatenate((s2[400:], s2[-400:])), axis, unc1, unc2)
    apart.phase_diff(20, 20)
    record('bed_picks_apart', lambda: apart.bed_pick())
    diff = time_diff(s1, s2, axis, unc1, unc2)
    diff.phase_diff(20, 20)
    record('bed_low_coherence', lambda: diff.bed_pick(coherence_threshold=1.5))

    dat = stacked(s1, axis)
    dat.flags.range = 0
    record('uncertainty_before_range', lambda: dat.phase_uncertainty(900.))
    bursts = stacked(s1, axis)
    bursts.data = np.vstack((s1[:60], s1[60:120], s1[120:180])).reshape(3, 1, 60)
    bursts.Rcoarse = axis[:60].copy()
    record('uncertainty_per_burst_stack', lambda: bursts.phase_uncertainty(5.), only=IndexError)
    save('CZ_errors', {'label': np.array(labels), 'exc_type': np.array(types_), 'message': np.array(messages)})
    for row in zip(labels, types_, messages):
        print('AF_CZ_errors: %s %s %r' % row)


def main():
    ax1 = np.arange(257) * 4.2
    jitter = 1.05 * (np.arange(400) + 0.2 * np.sin(np.arange(400) * 1.7))
    jitter[:2] = [0., 1.05]
    with np.errstate(all='ignore'):
        make_qc('QC1_products_257x24', 257, 1, ax1, 24, 0.1, products_first=True, extra=rolls)
        make_qc('QC2_uneven_400x40', 400, 4, jitter, 40, 0.1)
        make_qc('QC3_rows_1200x100', 1200, 6, np.arange(1200) * 1.05, 100, 0.1, rows_kept=slice(None, None, 40))
        make_qc('QC4_low_corner_257x24', 257, 1, ax1, 24, 0.004)
    acq = acquisitions(21)
    make_td('TD1_noise_phasor', acq)
    make_td('TD2_cramer_rao', acq, uncertainty='CR')
    make_td('TD3_no_uncertainty', acq, with_unc=False)
    make_au('AU1_stack_6000', acq[0], acq[2])
    errors(acq)


if __name__ == '__main__':
    main()
