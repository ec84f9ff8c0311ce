"""The host-side plan of a staged download (csrc/download_plan.h, compiled here by itself with g++: no GPU, no HIP): how
the blocks of a call are cut into pieces, and where the ring puts each piece.  The ring's capacity is a parameter of the
plan, so the sweep runs at capacities of 256 ... 8192 bytes, where every edge is a few pieces away: a ragged last piece,
a granule wider than a quarter of the ring, a wrap onto a piece that has not been copied out yet.  The same sweep runs
once more as a stand-alone program under AddressSanitizer and UBSan (tests/san/download_plan_sweep.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, 'impdar_amd', 'csrc')
CAPS = [256, 260, 1000, 1024, 4099, 8192]
ELEMS = [1, 4, 8]
GRANS = list(range(1, 71))
NBLKS = [1, 2, 3, 4]
VARIANTS = [0, 1, 2]
MAX_PIECES = 8192
needs_gxx = pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not installed')


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('downloadplan'))
    src, so = os.path.join(tmp, 'download_plan_probe.cpp'), os.path.join(tmp, 'libdownloadplan.so')
    with open(src, 'w') as f:
        f.write('#define DOWNLOAD_PLAN_PROBE 1\n#include "download_plan.h"\n')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-shared', '-fPIC', '-I', CSRC, src, '-o', so])
    lib = C.CDLL(so)
    lib.impdar_download_plan_probe.restype = C.c_longlong
    lib.impdar_download_plan_probe.argtypes = [C.c_size_t, C.c_size_t, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                               C.POINTER(C.c_longlong), C.c_longlong]
    return lib


OUT = (C.c_longlong * (6 * MAX_PIECES))()


def plan(lib, cap, elem, blocks):
    """blocks: [(count, gran)] -> the return code and the pieces (block, first, count, bytes, offset, retired)"""
    n = len(blocks)
    counts, grans = (C.c_size_t * n)(*[b[0] for b in blocks]), (C.c_size_t * n)(*[b[1] for b in blocks])
    rc = lib.impdar_download_plan_probe(cap, elem, n, counts, grans, OUT, MAX_PIECES)
    return rc, [tuple(OUT[6 * k:6 * k + 6]) for k in range(max(rc, 0))]


def swept_blocks(ci, elem, gran, nblk, v):
    """0 ... 40 granules per block; in every third case the last granule of a block is short"""
    blocks = []
    for b in range(nblk):
        g = (7 * gran + 13 * b + 11 * v + 5 * nblk + 3 * ci + elem) % 41
        short = (3 * v + b + 1) % gran if v == 2 and g > 0 else 0
        blocks.append((g * gran - short, gran))
    return blocks


def hold(cap, elem, blocks, rc, pieces):
    """what download.hip relies on; raises on the first rule that breaks"""
    too_wide = any(n > 0 and min(n, g) * elem > cap for n, g in blocks)
    assert (rc == -1) == too_wide, (rc, too_wide)          # a granule above the ring is the error, and nothing else is
    if too_wide:
        return
    assert rc >= 0
    # the pieces of a block: in order, each from a granule on, covering the block exactly once
    k = 0
    for i, (n, g) in enumerate(blocks):
        mine = []
        while k < len(pieces) and pieces[k][0] == i:
            mine.append(pieces[k])
            k += 1
        if n == 0:
            assert not mine
            continue
        granules = -(-n // g)
        assert len(mine) == min(granules, max(1, -(-n * elem // max(cap // 4, 1))))
        at = 0
        for (_, first, count, nbytes, _, _) in mine:
            assert first == at and first % g == 0 and count > 0 and nbytes == count * elem and nbytes <= cap
            at += count
        assert at == n
        sizes = [-(-p[2] // g) for p in mine]
        assert max(sizes) - min(sizes) <= 1                 # near-equal
    assert k == len(pieces)
    # the replay: pieces retired[k] ... k are live once k is placed; they lie inside the ring and apart
    last = 0
    for k, (_, _, _, nbytes, off, retired) in enumerate(pieces):
        assert last <= retired <= k and off % elem == 0 and 0 <= off and off + nbytes <= cap
        last = retired
        for j in range(retired, k):
            oj, bj = pieces[j][4], pieces[j][3]
            assert off + nbytes <= oj or oj + bj <= off, (j, k)


@needs_gxx
def test_sweep(lib):
    calls = 0
    for ci, cap in enumerate(CAPS):
        for elem in ELEMS:
            for gran in GRANS:
                for nblk in NBLKS:
                    for v in VARIANTS:
                        blocks = swept_blocks(ci, elem, gran, nblk, v)
                        rc, pieces = plan(lib, cap, elem, blocks)
                        try:
                            hold(cap, elem, blocks, rc, pieces)
                        except AssertionError:
                            print('cap %d elem %d blocks %s -> rc %d pieces %s' % (cap, elem, blocks, rc, pieces))
                            raise
                        calls += 1
    assert calls == len(CAPS) * len(ELEMS) * len(GRANS) * len(NBLKS) * len(VARIANTS)


# cap, element size, blocks
NAMED = {
    'a total below the ring': (4096, 4, [(100, 16)]),
    'a piece of exactly the ring': (1024, 4, [(64, 16), (256, 256), (64, 16)]),
    'a granule between a quarter of the ring and the ring': (1024, 4, [(700, 100)]),
    'a zero-width block between two others': (1024, 8, [(30 * 7, 7), (0, 0), (30 * 9, 9)]),
    'a flat block that is no multiple of 16': (8192, 4, [(1003, 16)]),
    'a flat block shorter than one granule, in a ring of its own size': (20, 4, [(5, 16)]),
    'many rings long': (256, 1, [(5000, 16), (3000, 1)]),
}


@needs_gxx
@pytest.mark.parametrize('name', sorted(NAMED))
def test_named_case(lib, name):
    cap, elem, blocks = NAMED[name]
    rc, pieces = plan(lib, cap, elem, blocks)
    assert rc > 0
    hold(cap, elem, blocks, rc, pieces)


@needs_gxx
def test_named_cases_are_what_they_say(lib):
    """the edge each named case is there for does occur in its plan"""
    pieces = plan(lib, *NAMED['a total below the ring'])[1]
    assert sum(p[3] for p in pieces) == 400 and [p[5] for p in pieces] == [0] * len(pieces)      # nothing waits for room
    pieces = plan(lib, *NAMED['a piece of exactly the ring'])[1]
    whole = [k for k, p in enumerate(pieces) if p[3] == 1024]
    assert len(whole) == 1 and pieces[whole[0]][5] == whole[0] and pieces[whole[0]][4] == 0        # everything before it retired
    pieces = plan(lib, *NAMED['a granule between a quarter of the ring and the ring'])[1]
    assert [p[3] for p in pieces] == [400] * 7 and max(p[5] for p in pieces) > 0
    pieces = plan(lib, *NAMED['a zero-width block between two others'])[1]
    assert sorted({p[0] for p in pieces}) == [0, 2]
    pieces = plan(lib, *NAMED['a flat block that is no multiple of 16'])[1]
    assert pieces[-1][2] % 16 != 0 and all(p[2] % 16 == 0 for p in pieces[:-1]) and len(pieces) > 1
    assert plan(lib, *NAMED['a flat block shorter than one granule, in a ring of its own size'])[1] == [(0, 0, 5, 20, 0, 0)]
    pieces = plan(lib, *NAMED['many rings long'])[1]
    assert any(b[4] < a[4] for a, b in zip(pieces, pieces[1:]))                                    # the ring wraps


@needs_gxx
def test_a_granule_above_the_ring_is_the_error(lib):
    assert plan(lib, 1024, 8, [(129 * 3, 129)])[0] == -1
    assert plan(lib, 1024, 8, [(64, 16), (129, 129)])[0] == -1
    assert plan(lib, 1024, 8, [(128 * 3, 128)])[0] == 3           # (a granule of exactly the ring is not)
    assert plan(lib, 1024, 8, [(0, 129)])[0] == 0                 # (and neither is one that holds nothing)


@needs_gxx
@pytest.mark.skipif(os.path.exists('/dev/kfd'), reason='sanitizer job is for the CPU container (never on the GPU box)')
def test_sweep_under_sanitizers(tmp_path):
    """Host code only, in a program of its own: the sanitizers' runtime is linked into it."""
    exe = str(tmp_path / 'download_plan_sweep')
    subprocess.check_call(['g++', '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-I', CSRC, os.path.join(ROOT, 'tests', 'san', 'download_plan_sweep.cpp'), '-o', exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:]
    swept = len(CAPS) * len(ELEMS) * len(GRANS) * len(NBLKS) * len(VARIANTS)
    assert '%d plans hold' % (swept + len(NAMED) + 4) in out.stdout


def test_download_unit_decides_nothing_itself():
    """download.hip takes the pieces and their places in the ring from the plan; api.hip holds no transfer plumbing."""
    header = open(os.path.join(CSRC, 'download_plan.h')).read()
    assert 'hip_runtime' not in header and '#include <hip' not in header and '#include "common.h"' not in header
    text = open(os.path.join(CSRC, 'download.hip')).read()
    assert '#include "download_plan.h"' in text
    for word in ('download_plan(', 'ring.place(', 'ring.retire('):
        assert word in text, word
    api = open(os.path.join(CSRC, 'api.hip')).read()
    for word in ('hipMemcpyDeviceToHost', 'std::thread', 'condition_variable', 'hipHostMalloc'):
        assert word not in api, word
