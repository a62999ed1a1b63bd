"""The route trace: every scenario of tests/route_scenarios.py takes the branch of the batch
check's failure search that it took when tests/golden/route_trace.json was recorded
(tools/route_trace.py --record) -- the same fallback stats, launches per stage, verdict, partial
and invalid entries.  Statuses alone cannot show that: every route gives exact statuses.

The stats and launch counts follow the device's CU count (grids, the eight-lane bound), so on a
device with another count than the recorded one the test skips."""
import importlib.util
import json
import os

import pytest

from route_scenarios import SCENARIOS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("route_trace", os.path.join(ROOT, "tools", "route_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tool():
    return _tool()


@pytest.fixture(scope="module")
def recorded(tool):
    with open(tool.GOLDEN) as f:
        rec = json.load(f)
    here = tool.device_info()
    if here["cus"] != rec["device"]["cus"]:
        pytest.skip("recorded on %s with %d CUs, this device (%s) has %d"
                    % (rec["device"]["name"], rec["device"]["cus"], here["name"], here["cus"]))
    return rec["scenarios"]


def test_every_scenario_is_recorded():
    with open(os.path.join(ROOT, "tests", "golden", "route_trace.json")) as f:
        rec = json.load(f)
    assert sorted(rec["scenarios"]) == sorted(s["name"] for s in SCENARIOS)
    assert len(set(s["name"] for s in SCENARIOS)) == len(SCENARIOS)


@pytest.mark.parametrize("scn", SCENARIOS, ids=[s["name"] for s in SCENARIOS])
def test_route(gpu, tool, recorded, scn):
    got = tool.run(scn, gpu)
    want = recorded[scn["name"]]
    print(scn["name"], got["fallback_stats"], got["launches"])
    assert got["invalid"] == tool.invalid_record(tool.forged_entries(scn)) and got["invalid_statuses"] == [1]
    for key in ("fallback_stats", "launches", "batch_ok", "partial", "invalid", "invalid_statuses"):
        assert got[key] == want[key], key
    assert got == want
