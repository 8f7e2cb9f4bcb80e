"""The host side of the device workflow engine launches what it launched when
tests/golden/wf_launch_trace.json was recorded: the same calls through
`pipe.ext` with the same arguments, the same aten ops in every tick after the
first, the same results. The scenarios and the comparison rules live in
tools/wf_launch_trace.py; admit() may issue fewer aten ops than recorded,
never more."""
import importlib.util
import json
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests" / "golden" / "wf_launch_trace.json"

_spec = importlib.util.spec_from_file_location(
    "wf_launch_trace", ROOT / "tools" / "wf_launch_trace.py")
trace = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(trace)

SCENARIOS = trace.scenarios()


@pytest.fixture(scope="module")
def fixture():
    assert FIXTURE.is_file(), f"{FIXTURE} is missing: the trace has nothing to be compared with"
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_every_scenario(fixture):
    assert set(fixture["scenarios"]) == set(SCENARIOS)
    assert len(SCENARIOS) == 18


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_launch_trace_matches_fixture(fixture, name):
    got = SCENARIOS[name]()
    assert any(e[0] == "k" for e in got["events"]) and any(e[0] == "a" for e in got["events"])
    assert trace.compare(trace.unpack(fixture, name), got) == []
