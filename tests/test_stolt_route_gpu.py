"""The gpu cases of tests/stolt_route_cases.py through the library: the metrics line of one migrate('stolt') -- and of a scan of
five velocities where the case has one -- names the kernels, and the batch, that the host-only route (csrc/stolt_route.h, through
its probe) gives for the case, and that the library reported at the commit before the route was split out of csrc/stolt.hip
(tests/stolt_route_recorded.json).  The images are the business of test_stolt_gpu.py, test_stolt_mixed_gpu.py and
test_velscan_gpu.py."""
import json

import pytest

import stolt_route_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
    return SC.probe(str(tmp_path_factory.mktemp('stoltroute')))


@pytest.fixture(scope='module')
def recorded():
    with open(SC.RECORDED) as f:
        return json.load(f)['cases']


@pytest.mark.parametrize('c', SC.GPU_CASES, ids=[c['id'] for c in SC.GPU_CASES])
def test_call_follows_the_route(hip, probe, recorded, c):
    assert c['snum'] <= 100 and c['tnum'] <= 2400
    got, m = SC.run(c), recorded[c['id']]
    assert got == SC.labels_of(probe, c)
    assert got == (m['kernel'], m['scan_kernel'], m['B'])
