"""The staged device -> host download (csrc/download.hip) by itself: DeviceArray.from_host, then to_host and to_host_f64,
held to the source bit for bit.  No kernel runs.  The sizes sit at the engine's edges: nothing to move, the direct copy
below 1 MiB (heap staging when it widens), one pinned ring with a ragged tail, several pieces with a short last one, and
an array just past the 64 MiB ring in either element size, so that the ring wraps.  The cases run from the largest to
the smallest in one context: the staging buffer a long download has grown is the one a shorter download then uses."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (shape, dtype), largest first
CASES = [((4099, 4101), np.float32),           # 67 239 996 bytes
         ((2897, 2903), np.float64),           # 67 279 928 bytes
         ((4194309,), np.float32), ((4194309,), np.float64),
         ((262151,), np.float32), ((262151,), np.float64),
         ((262143,), np.float32), ((262143,), np.float64),
         ((1, 1), np.float32), ((1, 1), np.float64),
         ((0, 5), np.float32), ((0, 5), np.float64)]


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.fixture(scope='module')
def sources():
    rng = np.random.default_rng(20261020)
    return [rng.standard_normal(shape).astype(dtype) for shape, dtype in CASES]


def test_sizes_are_the_edges_they_claim():
    ring, pin_from = 64 << 20, 1 << 20
    assert 4099 * 4101 * 4 == 67239996 > ring and 2897 * 2903 * 8 == 67279928 > ring
    assert 262143 * 4 < pin_from < 262151 * 4 and 262151 % 16 and 4194309 % 16


@pytest.mark.parametrize('k', range(len(CASES)), ids=['%s-%s' % ('x'.join(map(str, s)), np.dtype(d).name) for s, d in CASES])
def test_download_is_the_source(hip, sources, k):
    src = sources[k]
    dev = hip.DeviceArray.from_host(hip.context(), src)
    try:
        same, wide = dev.to_host(), dev.to_host_f64()
    finally:
        dev.free()
    assert same.dtype == src.dtype and same.shape == src.shape and np.array_equal(bits(same), bits(src))
    assert wide.dtype == np.float64 and wide.shape == src.shape and np.array_equal(bits(wide), bits(src.astype(np.float64)))
