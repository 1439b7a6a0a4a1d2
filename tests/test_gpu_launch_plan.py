"""The launch plans the library reports -- the `[cadnip f2]` lines of CADNIP_F2_DEBUG=1 and the ``info`` of ``Handle.factor_solve`` -- for
the matrix of tests/plan_cases.py, against tests/golden/launch_plans.json: the plans recorded (tools/make_plan_fixtures.py) before the
two planners became csrc/launch_plan.hpp, on an MI355X.  Lines and dicts are compared literally.  The plans depend on the device's
compute-unit count, which the fixture records: on another device the test fails and says so."""
import json

import pytest

from tests import plan_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(P.FIXTURE) as f:
        doc = json.load(f)
    assert set(doc["cases"]) == {"%s/%d" % c for c in P.CASES}
    return doc


@pytest.mark.parametrize("name,B", P.CASES, ids=["%s-%d" % c for c in P.CASES])
def test_plans_are_the_recorded_ones(name, B, golden):
    n_cu = P.device_cus()
    assert n_cu == golden["n_cu"], "the plans were recorded on a device of %d compute units; this one has %d" % (golden["n_cu"], n_cu)
    got, want = P.record(name, B), golden["cases"]["%s/%d" % (name, B)]
    for part in want:
        assert got[part] == want[part], (name, B, part)
    assert got == want
