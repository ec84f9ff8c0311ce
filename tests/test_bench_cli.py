"""bench.py's command line, CPU only: what --dump-outputs writes stays a fixed sample under 64 MB, and --steps
is the number of timed steps (at least one)."""
import subprocess
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_sample_is_fixed_in_range_and_under_64_mb():
    for snum, tnum in ((4096, 10000), (16384, 40000), (100000, 3000), (64, 50)):
        for itemsize in (4, 8):
            cols = bench.dump_columns(snum, tnum, itemsize)
            assert np.array_equal(cols, bench.dump_columns(snum, tnum, itemsize))
            assert len(cols) >= 1 and np.all(np.diff(cols) > 0) and cols[0] >= 0 and cols[-1] < tnum
            assert snum * len(cols) * itemsize <= 64e6
    assert len(bench.dump_columns(4096, 10000, 8)) == bench.DUMP_TRACES


def test_options_and_steps_guard():
    run = lambda *a: subprocess.run([sys.executable, 'bench.py'] + list(a), cwd=ROOT, capture_output=True, text=True, timeout=120)
    h = run('--help')
    assert h.returncode == 0 and '--full' in h.stdout and '--dump-outputs' in h.stdout
    bad = run('--steps', '0')
    assert bad.returncode == 2 and '--steps must be at least 1' in bad.stderr
