"""The quad-pol kernels at their smallest breaking shapes on the GPU: the sweeps of ``test_kernel_sweeps_cpu.py`` (its
docstring has the bars) with ``impdar_amd.quadpol``'s host-buffer entries in the restatements' place, against the
long-double references of ``sweep_ref.py``.

  coherence   1008 cases: n on both sides of every ``bk`` = 4 ... 64 that ``qp_block_rows`` picks, n = 1 (no window at
              all), windows of whole blocks and windows that end on the ragged last block, one output column of a
              padded pair, every column summed twice, rows of zeros (0 / 0)
  rotation    one row, one azimuth, more than one workgroup either way
  gradient    n = 2 (both edge rules, no interior), one column, both rules of numpy.gradient, the filtered form from
              the shortest length filtfilt accepts; a NaN and an exactly zero element
  order       a small call gives the same bits first on a fresh context and right after the largest call of the
              sweep: scratch of a larger call does not leak; the resident entry gives the host-buffer entry's bits

Each test prints its worst |error| / bar (``-s``)."""
import contextlib
import ctypes as C
from unittest.mock import patch

import numpy as np
import pytest

import sweep_ref as sw
from impdar_amd import quadpol as qpm
from test_kernel_sweeps_cpu import (GRAD_FILT_N, GRAD_N, ROT_SHAPES, check_gradient_refuses_twelve_rows,
                                    check_gradient_special_images, check_rotation, lowpass, same_bits, sweep_coherence,
                                    sweep_gradient, sweep_gradient_filtered)

pytestmark = pytest.mark.gpu

# (n, nrange, column case of sweep_ref.COH_COLS): every bk, both column forms, the all-NaN image, the rows of zeros
ORDER_COHERENCE = ((1, 1, 0), (2, 1, 1), (3, 2, 5), (5, 3, 2), (8, 1, 3), (9, 16, 6), (31, 17, 4), (33, 65, 3), (64, 257, 2),
                   (65, 1025, 6))
LARGEST_COHERENCE = (130, 1, 4)           # 130 x 24 box sums, and with bk = 4 the most block sums
# (n, m, jittered axis, filtered)
ORDER_GRADIENT = ((2, 1, True, False), (3, 2, True, False), (13, 5, False, True), (14, 1, True, True))
LARGEST_GRADIENT = ((257, 24, True, False), (257, 5, True, True))


@contextlib.contextmanager
def fresh_context(hip):
    """A context of its own, in ``_hip.context()``'s place while the block runs: the kernels' scratch starts empty."""
    lib, ctx = hip.load(), C.c_void_p()
    hip.check(lib.impdar_ctx_create(0, C.byref(ctx)), 'impdar_ctx_create')
    try:
        with patch.object(hip, 'context', lambda device=None: ctx):
            yield ctx
    finally:
        lib.impdar_ctx_destroy(ctx)


def coherence_case(case):
    n, nrange, col = case
    ncols, ntheta, wrap, _ = sw.COH_COLS[col]
    return sw.coherence_inputs(n, col) + (nrange, ntheta, wrap)


def gradient_case(case):
    n, m, jittered, filtered = case
    return (sw.coherence_image(n, m, 30 * n + m), qpm.gradient_coefficients(sw.range_axis(n, jittered)),
            lowpass() if filtered else None)


@pytest.mark.parametrize('n', sw.COH_N)
def test_coherence_sweep(hip, n):
    worst, nans = sweep_coherence(qpm.coherence_host, n)
    print('coherence n %3d: worst |diff| = %.3f of the bar, %d NaN outputs' % (n, worst, nans))


@pytest.mark.parametrize('shape', ROT_SHAPES)
def test_rotation_shapes(hip, shape):
    print('rotation %s: %.3f of the bar' % (shape, check_rotation(qpm.rotate_host, *shape)))


@pytest.mark.parametrize('n', GRAD_N)
def test_gradient_sweep(hip, n):
    print('gradient n %3d: worst ratio %.3f' % (n, sweep_gradient(qpm.phase_gradient_host, n)))


@pytest.mark.parametrize('n', GRAD_FILT_N)
def test_filtered_gradient_sweep(hip, n):
    print('filtered gradient n %3d: worst ratio %.3f' % (n, sweep_gradient_filtered(qpm.phase_gradient_host, n)))


def test_gradient_edges(hip):
    check_gradient_refuses_twelve_rows(qpm.phase_gradient_host)
    print('special images: worst ratio %.3f' % check_gradient_special_images(qpm.phase_gradient_host))


def test_coherence_does_not_depend_on_the_call_before(hip):
    first = []
    for case in ORDER_COHERENCE:
        with fresh_context(hip):
            first.append(qpm.coherence_host(*coherence_case(case)))
    for case, want in zip(ORDER_COHERENCE, first):
        qpm.coherence_host(*coherence_case(LARGEST_COHERENCE))
        assert same_bits(qpm.coherence_host(*coherence_case(case)), want), case


def test_gradient_does_not_depend_on_the_call_before(hip):
    first = []
    for case in ORDER_GRADIENT:
        with fresh_context(hip):
            first.append(qpm.phase_gradient_host(*gradient_case(case)))
    for case, want in zip(ORDER_GRADIENT, first):
        for largest in LARGEST_GRADIENT:
            qpm.phase_gradient_host(*gradient_case(largest))
        assert same_bits(qpm.phase_gradient_host(*gradient_case(case)), want), case


def test_resident_coherence_equals_the_host_buffer_form(hip):
    ctx = hip.context()
    for case in ORDER_COHERENCE:
        HH, VV, nrange, ntheta, wrap = coherence_case(case)
        held = [hip.DeviceArray.from_host(ctx, HH), hip.DeviceArray.from_host(ctx, VV)]
        try:
            held.append(qpm.coherence_dev(held[0], held[1], nrange, ntheta, wrap))
            assert same_bits(held[2].to_host(), qpm.coherence_host(HH, VV, nrange, ntheta, wrap)), case
        finally:
            for d in held:
                d.free()
