#!/usr/bin/env python3
"""Generate the ``FS*`` golden vectors (spectra of a radargram) by running the REFERENCE's ``plot_ft``, ``plot_hft`` and
``plot_spectrogram`` (``src/impdar/lib/plot.py:286-365, 621-725``) -- loaded by file path, never copied -- on small
synthetic radargrams, and evaluating the same quantities one precision step higher.

What the reference computed is taken from what it did: the line it drew (``plot_ft``, ``plot_hft``: the bins at
frequencies >= 0, held equal here to the same expression over all bins) and the ``scipy.signal.periodogram`` calls it
made (recorded through its own ``signal`` name while ``plot_spectrogram`` runs).  Its loaders need packages this
generator has no use for, so the ``load`` module it imports is replaced by an empty stand-in.

Every case exists as float32 and as float64; the float64 data is the float32 data widened, so both have the same exact
spectrum.  Stored per case: ``data`` (float32), and per quantity ``q`` in ft, hft, pg0, pg1, pg2 (the periodogram with
``spectra_ref.PARAMS[i]``, fs = 1 / ``spectra_ref.DT``):

  ``q_hi``       the quantity evaluated in longdouble on the widened data (``tests/spectra_ref.py``; ``np.fft`` of NumPy 2
                 takes longdouble), rounded to float64: the expected value of BOTH dtypes.  The HIP library widens float32
                 to float64 on load, so its float32 result is "the reference on the data widened to float64"; that float64
                 evaluation lies ``rho64_q`` from ``q_hi``, which is stored in its place (half the bytes, and the closer
                 value).
  ``rho64_q``    max |reference's float64 result - q_hi|: the reference's own error, what the bar is built from
  ``rho32_q``    max |reference's float32 result - q_hi|: how far NumPy >= 2 / SciPy on a float32 file lie from it (reported)
  ``Y_q``        the yardstick (``spectra_ref.yardstick_*``): a number for ft and hft, per trace for the periodograms

The reference's own arrays are not stored (the periodogram images of the larger shapes would take tens of MB); a case
that is larger than one file may be is split into ``name.npz``, ``name_p1.npz`` ... (``spectra_ref.load_fixture``).

The script prints rho64 / Y and rho32 / Y of every quantity, derives ``C`` = 8 x the largest rho64 / Y, checks that
``spectra_ref.C`` is that value rounded up, that the restated periodogram agrees with SciPy's float64 result within Y / 4,
and the bin-resolving condition: on every flat case at least 99 % of the bins of ``q_hi`` lie above 4 C Y (for the
periodograms: of the bins k >= 1 -- the detrend makes bin 0 zero by construction).

Only runs where the reference is installed; the committed files are what travels.

Usage:  python tests/golden/make_golden_spectra.py REFERENCE_SRC            (the directory that holds impdar/)
"""
import contextlib
import importlib
import io
import os
import sys
import types

import numpy as np
import scipy
import scipy.signal

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import spectra_ref as sr          # noqa: E402

VERS = dict(numpy_version=np.__version__, scipy_version=scipy.__version__)
PART_BYTES = 900 * 1024
SHAPES = [(32, 5), (36, 7), (30, 4), (63, 9), (22, 3), (7, 16384), (100, 33), (1022, 4), (1024, 65), (4096, 17), (16384, 2),
          (1, 3), (5, 1)]
NAN_CASE = ((36, 7), (11, 3))       # shape, the sample that is NaN
QUANTITIES = ('ft', 'hft', 'pg0', 'pg1', 'pg2')


def load_reference(src):
    """The reference's plot module under a private package name, its loaders replaced by a stand-in."""
    import matplotlib
    matplotlib.use('Agg')
    pkg = types.ModuleType('ref_impdar_lib')
    pkg.__path__ = [os.path.join(src, 'impdar', 'lib')]
    sys.modules['ref_impdar_lib'] = pkg
    stand_in = types.ModuleType('ref_impdar_lib.load')
    stand_in.load = None
    sys.modules['ref_impdar_lib.load'] = stand_in
    return importlib.import_module('ref_impdar_lib.plot')


def ref_dat(data):
    snum, tnum = data.shape
    return types.SimpleNamespace(data=data, snum=snum, tnum=tnum, dt=sr.DT, trace_num=np.arange(tnum) + 1.0, fn=None,
                                 flags=types.SimpleNamespace(interp=np.array([1.0, 2.0])))


def reference_results(plot, data):
    """{quantity: array} of what the reference computes for ``data`` (in its dtype)."""
    import matplotlib.pyplot as plt
    dat, out = ref_dat(data), {}
    with np.errstate(all='ignore'):
        for q, fn, axis in (('ft', plot.plot_ft, 0), ('hft', plot.plot_hft, 1)):
            _, ax = fn(dat)
            line = np.asarray(ax.lines[0].get_ydata())
            full = np.mean(np.abs(np.fft.fft(data, axis=axis)) ** 2.0, axis=1 - axis)        # plot.py:310-311, 346-347
            keep = np.fft.fftfreq(data.shape[axis]) >= 0
            assert np.array_equal(line, full[keep], equal_nan=True), q
            out[q] = full
        real = plot.signal
        for i, (win, scaling) in enumerate(sr.PARAMS):
            rows = []

            def recorder(x, **kw):
                f, p = scipy.signal.periodogram(x, **kw)
                rows.append(p)
                return f, p
            plot.signal = types.SimpleNamespace(periodogram=recorder)
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    plot.plot_spectrogram(dat, window=win, scaling=scaling)
            except Exception:       # (the contour plot refuses an image with fewer than 2 x 2 points; the loop has run)
                pass
            finally:
                plot.signal = real
            assert len(rows) == data.shape[1], (len(rows), data.shape)
            out['pg%d' % i] = np.transpose(rows)
    plt.close('all')
    return out


def hi_results(data64):
    x = data64.astype(np.longdouble)
    with np.errstate(all='ignore'):
        out = {'ft': sr.mean_spectrum(x, 0), 'hft': sr.mean_spectrum(x, 1)}
        for i, (win, scaling) in enumerate(sr.PARAMS):
            out['pg%d' % i] = sr.periodogram(x, 1.0 / sr.DT, win, scaling)
    return {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}


def yardsticks(data64):
    with np.errstate(all='ignore'):
        out = {'ft': sr.yardstick_mean(data64, 0), 'hft': sr.yardstick_mean(data64, 1)}
        for i, (win, scaling) in enumerate(sr.PARAMS):
            out['pg%d' % i] = sr.yardstick_periodogram(data64, 1.0 / sr.DT, win, scaling)
    return out


def save(name, arrs):
    """Greedy packing into files of at most PART_BYTES."""
    parts, cur, size = [], {}, 0
    for k, v in arrs.items():
        nb = np.asarray(v).nbytes + 256
        assert nb < PART_BYTES, (k, nb)
        if cur and size + nb > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += nb
    parts.append(cur)
    parts[0].update(VERS)
    for i, p in enumerate(parts):
        path = os.path.join(HERE, name + ('' if i == 0 else '_p%d' % i) + '.npz')
        np.savez_compressed(path, **p)
        nbytes = os.path.getsize(path)
        print('wrote', path, nbytes, 'bytes')
        assert nbytes < 1000 * 1024, nbytes


def max_ratio(diff, Y):
    """max |diff| / Y over the finite positions (Y a number, or per trace along the last axis)."""
    with np.errstate(all='ignore'):
        r = np.abs(diff) / Y
    r = r[np.isfinite(r)]
    return float(r.max()) if r.size else 0.0


def main(src):
    plot = load_reference(src)
    rng = np.random.default_rng(20261020)
    cases = []
    for shape in SHAPES:
        flat = rng.standard_normal(shape)
        peaked = flat + 50.0 + 3.0 * np.sin(0.3 * np.arange(shape[0]))[:, None]
        cases += [(shape, 'flat', flat.astype(np.float32)), (shape, 'peaked', peaked.astype(np.float32))]
    shape, where = NAN_CASE
    bad = rng.standard_normal(shape).astype(np.float32)
    bad[where] = np.nan
    cases.append((shape, 'nan', bad))

    table, resolved = [], []
    for idx, (shape, kind, data32) in enumerate(cases):
        name = 'FS%02d_%dx%d_%s' % (idx + 1, shape[0], shape[1], kind)
        data64 = data32.astype(np.float64)
        ref32, ref64, hi, Y = reference_results(plot, data32), reference_results(plot, data64), hi_results(data64), yardsticks(data64)
        arrs = dict(data=data32, kind=kind)
        for q in QUANTITIES:
            assert ref32[q].shape == ref64[q].shape == hi[q].shape, (name, q)
            assert np.array_equal(np.isnan(ref64[q]), np.isnan(hi[q])) and np.array_equal(np.isnan(ref32[q]), np.isnan(hi[q])), (name, q)
            with np.errstate(all='ignore'):
                rho64, rho32 = np.abs(ref64[q] - hi[q]), np.abs(ref32[q].astype(np.float64) - hi[q])
            fin = np.isfinite(hi[q])
            arrs[q + '_hi'], arrs['Y_' + q] = hi[q], Y[q]
            arrs['rho64_' + q] = float(rho64[fin].max()) if fin.any() else 0.0
            arrs['rho32_' + q] = float(rho32[fin].max()) if fin.any() else 0.0
            table.append((name, q, max_ratio(rho64, Y[q]), max_ratio(rho32, Y[q])))
            if q.startswith('pg'):
                win, scaling = sr.PARAMS[int(q[2])]
                with np.errstate(all='ignore'):
                    mine = sr.periodogram(data64, 1.0 / sr.DT, win, scaling)
                assert max_ratio(mine - ref64[q], Y[q]) <= 0.25, (name, q, max_ratio(mine - ref64[q], Y[q]))
            if kind == 'flat':
                resolved.append((name, q, hi[q][1:] if q.startswith('pg') else hi[q], Y[q]))
        save(name, arrs)

    print('%-26s %-4s %12s %12s' % ('case', 'q', 'rho64 / Y', 'rho32 / Y'))
    for name, q, r64, r32 in table:
        print('%-26s %-4s %12.4f %12.4g' % (name, q, r64, r32))
    worst = max(r[2] for r in table)
    C = 8 * worst
    print('largest rho64 / Y: %.4f  ->  C = 8 x that = %.4f; spectra_ref.C = %g' % (worst, C, sr.C))
    assert C <= sr.C <= 1.25 * C + 0.5, 'set spectra_ref.C to %g rounded up' % C
    for name, q, bins, Y in resolved:
        if bins.size:
            frac = float(np.mean(bins > 4 * sr.C * Y))
            assert frac >= 0.99, (name, q, frac)
    print('bin-resolving condition holds on every flat case')


if __name__ == '__main__':
    main(sys.argv[1])
