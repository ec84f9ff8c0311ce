"""The ApRES kernels at their smallest breaking shapes on the GPU: the sweeps of ``test_kernel_sweeps_cpu.py`` (its
docstring has the bars) with ``impdar_amd.apres``'s host-buffer entries in the restatements' place, against the
long-double references of ``sweep_ref.py``.

  phase difference   700 cases: vectors shorter than a window, no terms at all (win 0 and 1), lengths and windows around
                     the 64 terms where a wavefront takes over from a thread, window counts around a workgroup of
                     threads (256) and of wavefronts (4), a run of zeros (0 / 0)
  range conversion   2 and 3 samples (the shortest real transforms), 255 / 256 / 257 around the workgroup of
                     ``ar_prep_kernel``, pad factors 1 ... 3, a tail chunk of one chirp
  stacking           1 and 2 samples, 255 / 256 / 257, means of 1 ... 100 rows, rows behind the last group that must
                     not be read; real and complex

Each test prints its worst |error| / bar (``-s``)."""
import pytest

import sweep_ref as sw
from impdar_amd import apres as apm
from test_kernel_sweeps_cpu import RANGE_P, RANGE_SNUM, STACK_SNUM, check_range, sweep_phase_diff, sweep_stack

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('length', sw.PD_LEN)
def test_phase_diff_sweep(hip, length):
    worst, nans, empty = sweep_phase_diff(apm.phase_diff_host, length)
    print('phase difference len %3d: worst |diff| = %.3f of the bar, %d NaN windows, %d cases without a window'
          % (length, worst, nans, empty))


@pytest.mark.parametrize('snum', RANGE_SNUM)
def test_range_sweep(hip, snum):
    for p in RANGE_P:
        for chunk in ((0, 2) if snum == 257 else (0,)):
            worst, rworst, checked, left = check_range(apm.range_host, snum, p, chunk)
            print('range snum %3d p %d chunk %d: spec/data %.3f of E, Rfine %.3f of its bar on %d bins, %d left out'
                  % (snum, p, chunk, worst, rworst, checked, left))


@pytest.mark.parametrize('snum', STACK_SNUM)
def test_stack_sweep(hip, snum):
    sweep_stack(apm.stack_host, snum)
