"""The host-side route of a Stolt call (csrc/stolt_route.h, compiled here by itself with g++: no GPU, no HIP): the knob, the choice
between rocFFT and the two forms of the own transforms, the sizes of a call, the key of the cached plan, the batches of a
velocity scan and the kernel strings of the metrics line.

Where the expected values come from.  model_route(), model_shape() and model_scan() below are restatements of stolt_route,
stolt_prepare and stolt_scan_run as they stood in csrc/stolt.hip at the commit before the route was split out of it (source (a)),
written from their text; LABELS are that file's string literals.  In addition tests/stolt_route_recorded.json holds (source (b))
what that commit's library reported on the GPU for the cases marked gpu: the `kernel` string of impdar_ctx_last_metrics after a
single call, and `kernel` and "B" after a scan."""
import json
import os
import subprocess

import pytest

import stolt_route_cases as SC
from stolt_route_cases import ROCFFT, ROWS, WKX

BUDGET, MAX_BATCH = 2 << 30, 1024
LABELS = {
    (ROWS, False, False): "stolt_stretch_rows (+ the library's own row transforms, traces first)",
    (ROWS, True, False): "stolt_stretch_rows (+ the library's own row transforms, traces first, mixed radix)",
    (WKX, False, False): "stolt_stretch (+ the library's own row transforms)",
    (WKX, True, False): "stolt_stretch (+ the library's own row transforms, mixed radix)",
    (ROCFFT, False, False): "stolt_stretch (+ rocFFT 2-D real transforms)",
    (ROWS, False, True): "stolt_stretch_scan_rows (+ the library's own row transforms, traces first)",
    (ROWS, True, True): "stolt_stretch_scan_rows (+ the library's own row transforms, traces first, mixed radix)",
    (WKX, False, True): "stolt_stretch_scan_t (+ the library's own row transforms)",
    (WKX, True, True): "stolt_stretch_scan_t (+ the library's own row transforms, mixed radix)",
    (ROCFFT, False, True): "stolt_stretch (+ rocFFT 2-D real transforms, one velocity at a time)",
}


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return SC.probe(str(tmp_path_factory.mktemp('stoltroute')))


def pow2(n):
    return n > 0 and n & (n - 1) == 0


def pow2_len_ok(m):
    return 16 <= m <= 8192 and pow2(m)


def mixed_len_ok(m):
    if m < 16 or m > 8192:
        return False
    for p in (2, 3, 5, 7):
        while m % p == 0:
            m //= p
    return m == 1


def model_route(c):
    snum, tnum, kx, word = c['snum'], c['tnum'], SC.kx_of(c), c['knob']
    want2d, no_own, want_mixed = word != '1d', word == 'rocfft', word == 'mixed'
    if not (want2d and not no_own):
        return ROCFFT
    if snum % 2:
        return ROCFFT
    if pow2(snum) and pow2(tnum):
        if not (pow2_len_ok(snum // 2) and pow2_len_ok(tnum)):
            return ROCFFT
        return ROWS if pow2_len_ok(snum) and tnum >= 64 else WKX
    if not (want_mixed or snum > 1024 or tnum > 1024):
        return ROCFFT

    def len_ok(m):
        return pow2_len_ok(m) or mixed_len_ok(m)
    if tnum % 2 == 0 and tnum >= 64 and len_ok(tnum // 2) and len_ok(snum):
        if all(kx[k] == -kx[tnum - k] for k in range(1, tnum // 2)):
            return ROWS
    return WKX if len_ok(snum // 2) and len_ok(tnum) else ROCFFT


def model_shape(c):
    snum, tnum, route = c['snum'], c['tnum'], model_route(c)
    m, nout = snum // 2 + 1, 2 * (snum // 2)
    use_own = route != ROCFFT
    return dict(route=route, m=m, nz=snum // 2, nout=nout, hs=tnum // 2 + 1, use_own=int(use_own),
                mixed=int(use_own and not (pow2(snum) and pow2(tnum))), x_elems=tnum * snum,
                spec_elems=max(tnum * m, snum * (tnum // 2 + 1)), y_elems=tnum * nout)


def model_scan(c, nv, max_batch):
    s, esz = model_shape(c), 8 if c['dtype'] == 'float64' else 4
    plane = 0 if not s['use_own'] else (s['hs'] * c['snum'] if s['route'] == ROWS else s['m'] * c['tnum'])
    iplane = s['nout'] * c['tnum']
    per = 2 * plane * 2 * esz + max(iplane, 1) * esz
    B = min(max(BUDGET // per, 1), min(nv, MAX_BATCH))
    if max_batch > 0:
        B = min(B, max_batch)
    return dict(plane=plane, iplane=iplane, per=per, B=B, batches=(nv + B - 1) // B)


@pytest.mark.parametrize('c', SC.CASES, ids=SC.IDS)
def test_route_and_shape_are_what_prepare_decided(lib, c):
    assert SC.shape(lib, c) == model_shape(c)


def test_every_branch_is_reached(lib):
    """The preconditions the cases stand for (so that a change of a threshold cannot quietly empty a case)."""
    r = {c['id']: SC.shape(lib, c) for c in SC.CASES}

    def routes(*ids):
        return [r[i + '-float32' if 'float' not in i else i]['route'] for i in ids]
    # the table of the smallest shapes
    assert routes('64x64-float64', '100x48') == [ROWS, ROCFFT]
    assert routes('64x64-float32-scan2', '64x32-float32-scan0', '65x50-float32-scan0', '96x2400-float32-scan0') == [ROWS, WKX, ROCFFT, ROWS]
    assert routes('96x160-float32-mixed', '96x160', '96x1125', '96x2400-float32-bent', '64x64-float32-rocfft', '64x64-float32-1d') == \
        [ROWS, ROCFFT, WKX, WKX, ROCFFT, ROCFFT]
    assert [r[i]['mixed'] for i in ('64x64-float32-scan2', '96x2400-float32-scan0', '96x1125-float32', '64x32-float32-scan0')] == [0, 1, 1, 0]
    # the knob: 'own' and an unknown word are the default, 'mixed' changes nothing at a power of two
    assert routes('64x64-float32-own', '64x64-float32-mixed', '64x64-float32-fastest') == [ROWS, ROWS, ROWS]
    assert routes('96x160-float32-own', '96x160-float32-fastest', '96x160-float32-rocfft', '96x160-float32-1d') == [ROCFFT] * 4
    # powers of two around own_fft_len_ok
    assert routes('8192x64', '16384x64', '32768x64', '16x64', '32x64', '64x8', '64x16', '64x16384') == \
        [ROWS, WKX, ROCFFT, ROCFFT, ROWS, ROCFFT, WKX, ROCFFT]
    assert routes('64x64-float32-bent', '64x64-float32-mixed-bent') == [ROWS, ROWS]             # (see the cases)
    # no power of two: the gate at 1024, and each refusal of the rows form
    assert routes('1500x64', '1024x96', '96x1024', '1080x96', '96x1080') == [ROWS, ROCFFT, ROCFFT, ROWS, ROWS]
    assert routes('120x60-float32-mixed', '9600x64', '96x160-float32-mixed-bent', '96x20-float32-mixed') == [WKX] * 4
    assert routes('96x1144', '1100x64', '88x160-float32-mixed', '96x176-float32-mixed') == [ROCFFT] * 4
    assert routes('20x96-float32-mixed') == [ROWS]
    assert routes('65x51', '64x51', '2x1', '3x2-float64') == [ROCFFT] * 4
    assert r['65x51-float32']['nout'] == 64 and r['2x1-float32']['nout'] == 2 and r['3x2-float64']['m'] == 2
    # a wide radargram: the rows layout is the larger spectrum; a narrow one: the [tnum][m] layout
    assert r['64x64-float32-scan2']['spec_elems'] == 64 * 33 and r['96x2400-float32-scan0']['spec_elems'] == 2400 * 49 > 96 * 1201
    assert r['64x16-float32']['spec_elems'] == 64 * 9 > 16 * 33


@pytest.mark.parametrize('snum,tnum,dtype,word,nv,max_batch', SC.SCAN_CASES)
def test_scan_batches(lib, snum, tnum, dtype, word, nv, max_batch):
    c = SC.case(snum, tnum, dtype, knob=word)
    assert SC.scan_plan(lib, c, nv, max_batch) == model_scan(c, nv, max_batch)


def test_every_bound_of_the_batch_decides_once(lib):
    assert (lib.stolt_probe_budget(), lib.stolt_probe_max_batch()) == (BUDGET, MAX_BATCH)
    got = {k: SC.scan_plan(lib, SC.case(k[0], k[1], k[2], knob=k[3]), k[4], k[5]) for k in SC.SCAN_CASES}
    B = {k: (v['B'], v['batches']) for k, v in got.items()}
    # the budget: 2 GiB / (two spectra of 2049 x 4096 complex and an image of 4096 x 4096) = 10.66 float32, 5.33 float64
    assert B[(4096, 4096, 'float32', None, 64, 0)] == (10, 7) and B[(4096, 4096, 'float64', None, 64, 0)] == (5, 13)
    assert B[(4096, 4096, 'float32', None, 64, 7)] == (7, 10)
    assert B[(64, 64, 'float32', None, 5, 0)] == (5, 1) and B[(64, 64, 'float32', None, 5, 2)] == (2, 3)
    assert B[(64, 64, 'float64', None, 3000, 0)] == (1024, 3)
    assert got[(65, 50, 'float64', None, 5, 0)]['plane'] == 0 and B[(65, 50, 'float64', None, 5, 0)] == (5, 1)
    assert got[(4096, 4096, 'float32', 'rocfft', 64, 0)]['plane'] == 0 and B[(4096, 4096, 'float32', 'rocfft', 64, 0)] == (32, 2)
    assert got[(2, 1, 'float32', None, 5, 0)]['iplane'] == 2 and B[(2, 1, 'float32', None, 5, 0)] == (5, 1)
    assert B[(96, 2400, 'float32', None, 9, 4)] == (4, 3)


def test_labels_are_the_literals(lib):
    """All ten strings, whole; `mixed` follows from the sizes (64 x 64: powers of two; 96 x 160: not)."""
    for (route, mixed, scan), want in LABELS.items():
        snum, tnum = (96, 160) if mixed else (64, 64)
        assert SC.label(lib, snum, tnum, route, scan) == want
    # on rocFFT no transform is the library's own, whatever the sizes
    assert SC.label(lib, 96, 160, ROCFFT, False) == LABELS[(ROCFFT, False, False)]
    assert SC.label(lib, 96, 160, ROCFFT, True) == LABELS[(ROCFFT, False, True)]


def test_plan_key_compares_every_field(lib):
    import numpy as np
    base = np.array([0x1000, 0, 64, 64, 1, 0, ROWS], dtype=np.int64)
    assert lib.stolt_probe_key_eq(base.ctypes.data_as(SC._lp), base.copy().ctypes.data_as(SC._lp)) == 1
    for i, other in enumerate((0x2000, 1, 128, 128, 0, 1, WKX)):
        b = base.copy()
        b[i] = other
        assert lib.stolt_probe_key_eq(base.ctypes.data_as(SC._lp), b.ctypes.data_as(SC._lp)) == 0, i


def test_route_agrees_with_what_the_library_reported(lib):
    """tests/stolt_route_recorded.json: the metrics lines of the gpu cases from a GPU run of the commit before stolt_route.h."""
    with open(SC.RECORDED) as f:
        rec = json.load(f)['cases']
    assert sorted(rec) == sorted(c['id'] for c in SC.GPU_CASES)
    for c in SC.GPU_CASES:
        m = rec[c['id']]
        assert SC.labels_of(lib, c) == (m['kernel'], m['scan_kernel'], m['B']), c['id']


def test_knobs_from_env(tmp_path):
    """StoltKnobs::from_env: one read of IMPDAR_STOLT_FFT, the three words that mean something, and equality."""
    src, exe = str(tmp_path / 'knobs.cpp'), str(tmp_path / 'knobs')
    with open(src, 'w') as f:
        f.write('#include "stolt_route.h"\n#include <cstdio>\nint main() { const StoltKnobs K = StoltKnobs::from_env();\n'
                'printf("%d %d %d %d\\n", K.use2d, K.no_own, K.want_mixed, K == StoltKnobs()); return 0; }\n')
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-I', SC.CSRC, src, '-o', exe])
    clean = {k: v for k, v in os.environ.items() if k != SC.KNOB}

    def read(env):
        return [int(v) for v in subprocess.run([exe], env=dict(clean, **env), capture_output=True, text=True, check=True).stdout.split()]
    assert read({}) == [1, 0, 0, 1]
    for word in SC.WORDS[1:] + ('', 'MIXED', '1D', 'rocfft '):
        assert read({SC.KNOB: word}) == list(SC.knob_flags(word)) + [int(word not in ('mixed', 'rocfft', '1d'))], word
