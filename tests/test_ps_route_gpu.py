"""The recorded choice of the phase shift: for every case of tests/ps_route_cases.py (the smallest shapes that reach every branch
of csrc/ps_route.h, the knobs one at a time) the library reports the kernel, walk, transforms, long runs and spectrum layout that
the commit before the route was split out of ps_run reported on an MI355X (tests/ps_route_recorded.json)."""
import json

import numpy as np
import pytest

import ps_route_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def recorded():
    with open(PC.RECORDED) as f:
        return json.load(f)['cases']


@pytest.mark.parametrize('case', PC.CASES, ids=PC.IDS)
def test_recorded_choice(hip, monkeypatch, recorded, case):
    for k in PC.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case['env'].items():
        monkeypatch.setenv(k, v)
    m, img = PC.run(hip, case)
    assert {f: m.get(f) for f in PC.FIELDS} == recorded[PC.case_id(case)]
    assert img.shape == (PC.SNUM, case['tnum']) and np.isfinite(img).all()
