"""The host-only plan of the mixed-radix row transforms (csrc/own_fft_mixed_plan.h), compiled by itself: which lengths it
takes, the passes of a length, the position of every output index, and the passes executed on a host array -- with the index
helpers the kernel calls -- against numpy.fft in float64: max|diff| <= 1e-13 * log2(M) * max|ref| (the bar of
tests/test_own_fft_gpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LENGTHS = [18, 20, 21, 48, 60, 100, 250, 625, 1250, 2401, 5000, 6561, 7500, 8000]
MAX_PASSES = 8


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('mixed_plan'))
    src, lib = os.path.join(tmp, 'mixed_plan_probe.cpp'), os.path.join(tmp, 'libmixedplan.so')
    with open(src, 'w') as f:
        f.write('#define OWN_FFT_MIXED_PROBE 1\n#include "own_fft_mixed_plan.h"\n')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'impdar_amd', 'csrc'), src, '-o', lib])
    so = C.CDLL(lib)
    so.impdar_own_mixed_len_ok.argtypes = [C.c_longlong]
    return so


def smooth(m):
    for p in (2, 3, 5, 7):
        while m % p == 0:
            m //= p
    return m == 1


def radices(plan, M):
    r = np.zeros(MAX_PASSES, dtype=np.int32)
    n = plan.impdar_own_mixed_radices(M, r.ctypes.data_as(C.POINTER(C.c_int)))
    return [int(v) for v in r[:n]]


def test_which_lengths_are_taken(plan):
    for M in range(1, 20001):
        assert bool(plan.impdar_own_mixed_len_ok(M)) == (16 <= M <= 8192 and smooth(M)), M
    for M in (0, -16, 1 << 40):
        assert not plan.impdar_own_mixed_len_ok(M)


def test_passes_multiply_to_the_length(plan):
    for M in range(1, 8300):
        rs = radices(plan, M)
        if not (16 <= M <= 8192 and smooth(M)):
            assert rs == [], M
            continue
        assert 0 < len(rs) <= MAX_PASSES and set(rs) <= {2, 3, 4, 5, 7} and int(np.prod(rs)) == M, (M, rs)
        assert rs.count(2) <= 1, (M, rs)               # (two factors 2 are one radix-4 pass)


@pytest.mark.parametrize('M', LENGTHS + [16, 64, 4096, 8192])
def test_position_map_is_the_digit_reversal(plan, M):
    pos = np.full(M, -1, dtype=np.int32)
    rc = plan.impdar_own_mixed_positions(M, pos.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == 0
    assert np.array_equal(np.sort(pos), np.arange(M))
    # restated: the digits of k, least significant first, in pass order, are the digits of the position, most significant first
    rs = radices(plan, M)
    k = np.arange(M)
    want, span = np.zeros(M, dtype=np.int64), M
    for r in rs:
        span //= r
        want += (k % r) * span
        k = k // r
    assert np.array_equal(pos, want)


@pytest.mark.parametrize('M', LENGTHS)
def test_host_passes_against_numpy(plan, M):
    rng = np.random.default_rng(M)
    z = rng.standard_normal(M) + 1j * rng.standard_normal(M)
    dp = C.POINTER(C.c_double)
    for inv, ref in ((0, np.fft.fft(z)), (1, np.fft.ifft(z) * M)):
        out = np.zeros(M, dtype=np.complex128)
        rc = plan.impdar_own_mixed_transform(M, inv, z.ctypes.data_as(dp), out.ctypes.data_as(dp))
        assert rc == 0
        err = np.max(np.abs(out - ref)) / np.max(np.abs(ref))
        assert err < 1e-13 * np.log2(M), (M, inv, err)
