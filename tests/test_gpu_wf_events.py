"""GPU tests of the step-transition journal through WorkflowPipeline: the
scripted churn of tests/test_wf_events.py gives, tick by tick, the same
sorted events on the HIP extension as on the CPU reference, with the captured
tick graph and without it, and a tight event list overflows without losing a
step's history.

Run as a script, this module executes the churn on the GPU and saves the
result: the graph / no-graph comparison starts each mode in a fresh process.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT_S = 120


def _E():
    from tests import test_wf_events as E

    return E


def assert_same_events(got, want):
    assert len(got["events"]) == len(want["events"])
    for i, (g, w) in enumerate(zip(got["events"], want["events"])):
        assert tuple(map(list, g)) == tuple(map(list, w)), f"events of drain {i} differ"
    assert got["event_overflows"] == want["event_overflows"]
    assert torch.equal(got["shadow"], want["shadow"])


def test_scripted_churn_events_match_reference():
    E = _E()
    got = E.run_event_churn("ext", "cuda:0", E.AMPLE)
    want = E.reference_events(E.AMPLE)
    assert got["event_overflows"] == 0
    assert_same_events(got, want)
    E.D.assert_same_run(got, want)


def test_a_tight_event_list_overflows_and_still_replays():
    """event_cap = 8: which changes a full list lets in is undefined on the
    GPU, so the lists differ from the reference's; the replay (asserted
    after every drain inside the driver) and the end state do not."""
    E = _E()
    got = E.run_event_churn("ext", "cuda:0", E.TIGHT)
    assert got["event_overflows"] > 0
    want = E.reference_events(E.TIGHT)
    assert torch.equal(got["shadow"], want["shadow"])
    E.D.assert_same_run(got, want)


def _child(tmp_path, name, no_graph):
    out = tmp_path / f"{name}.pt"
    env = dict(os.environ)
    env.pop("CORDUM_WF_NO_GRAPH", None)
    if no_graph:
        env["CORDUM_WF_NO_GRAPH"] = "1"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    flags = ["-s"] if sys.flags.no_user_site else []
    p = subprocess.run([sys.executable, *flags, os.path.abspath(__file__), str(out)],
                       env=env, cwd=root, timeout=CHILD_TIMEOUT_S,
                       capture_output=True, text=True)
    assert p.returncode == 0, f"{name} child failed ({p.returncode}):\n{p.stderr[-2000:]}"
    return torch.load(out, weights_only=False)


def test_events_are_the_same_with_the_graph_and_without(tmp_path):
    # each mode in a fresh process with its own timeout; a failure of the
    # first raises here, so the second is never started after it
    E = _E()
    graph = _child(tmp_path, "graph", no_graph=False)
    assert graph["graph"] is True
    eager = _child(tmp_path, "eager", no_graph=True)
    assert eager["graph"] is False
    assert_same_events(graph, eager)
    assert_same_events(graph, E.reference_events(E.AMPLE))
    E.D.assert_same_run(graph, eager)


if __name__ == "__main__":
    E = _E()
    torch.save(E.run_event_churn("ext", "cuda:0", E.AMPLE), sys.argv[1])
