"""Every header that the phase-shift units (csrc/phaseshift.hip, csrc/ffd.hip), the Kirchhoff units (csrc/kirchhoff.hip,
kirch_ring32.hip, kirch_ring64.hip, kirch_oneshot.hip, kirch_gen.hip) or the Stolt and transform units (csrc/stolt.hip, csrc/fft.hip)
include from csrc/ (transitively) compiles as the only include of a
translation unit: each names what it uses, none relies on the place or the order in which a source happens to include it.
Syntax only (host and device pass), no GPU."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
CSRC = os.path.join(ROOT, 'impdar_amd', 'csrc')


def _local_headers(path, seen):
    with open(path) as f:
        names = re.findall(r'^\s*#\s*include\s+"([^"/]+)"', f.read(), flags=re.M)
    for n in names:
        h = os.path.join(CSRC, n)
        if os.path.exists(h) and n not in seen:
            seen.add(n)
            _local_headers(h, seen)
    return seen


def headers():
    seen = set()
    for src in ('phaseshift.hip', 'ffd.hip', 'kirchhoff.hip', 'kirch_ring32.hip', 'kirch_ring64.hip', 'kirch_oneshot.hip', 'kirch_gen.hip',
                'stolt.hip', 'fft.hip'):
        _local_headers(os.path.join(CSRC, src), seen)
    return sorted(seen)


def test_the_split_headers_are_among_them():
    assert {'ps_layout.h', 'ps_common.h', 'ps_direct.h', 'ps_plan.h', 'ps_mfma.h', 'ps_smooth.h', 'ps_nufft.h', 'ps_series.h',
            'ps_runs.h', 'ps_route.h', 'ps_path_plan.h', 'ps_series_plan.h', 'fft.h', 'own_fft.h', 'common.h',
            'kirch_prep.h', 'kirch_exact.h', 'kirch_ring.h', 'kirch_plan.h', 'kirch_route.h',
            'stolt_route.h', 'stolt_kernels.h'} <= set(headers())


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_every_header_compiles_alone(tmp_path):
    procs = []
    for h in headers():
        src = str(tmp_path / (h[:-2] + '_alone.hip'))
        with open(src, 'w') as f:
            f.write('#include "%s"\n' % h)
        procs.append((h, subprocess.Popen([HIPCC, '--offload-arch=gfx950', '-std=c++17', '-fsyntax-only', '-I', CSRC, src],
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    failed = {}
    for h, pr in procs:
        log = pr.communicate(timeout=600)[0]
        if pr.returncode != 0:
            failed[h] = log[-2000:]
    assert not failed, '\n'.join('%s:\n%s' % kv for kv in sorted(failed.items()))
