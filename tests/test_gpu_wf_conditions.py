"""GPU test of conditions decided on the device, through the pipeline: 65 runs
of one template `worker -> condition(out0 > K) -> guarded for_each x3` with
alternating inputs, a fifth of the children failing, give after every tick
the same step states, output words, run tables and counters, and the same
completion records, on the HIP extension as on the CPU reference backend,
with the captured tick graph and without it.
"""
import functools

import pytest
import torch

from tests.test_gpu_wf_dynamic import COUNTERS, TABLES

pytestmark = pytest.mark.gpu

NR, TICKS, K = 65, 14, 1000
COND_TABLES = ("step_out", "run_input", "run_tmpl", "cond_counts")
BIG, SMALL = [600, 500, -7], [5, 6]          # out0 = 1093 > K, out0 = 11 <= K


def branch_dag():
    from cordum_amd.ops.wf_pipeline import (
        CondSpec, DagSpec, StepSpec, WFK_CONDITION, WFK_FOR_EACH, WFK_WORKER)

    return DagSpec(steps=[
        StepSpec(WFK_WORKER),
        StepSpec(WFK_CONDITION, deps=[0], when=CondSpec(">", ("out", 0), K)),
        StepSpec(WFK_FOR_EACH, deps=[1], fanout=3, when=CondSpec("truthy", ("out", 1))),
    ])


def run_script(backend, device):
    from cordum_amd.ops.wf_pipeline import WorkflowPipeline

    pipe = WorkflowPipeline(device=device, dags=[branch_dag()], backend=backend,
                            n_local_workers=16, payload_words=10, fail_ppt=200,
                            max_retries=2, dynamic_capacity=NR, device_conditions=True)
    log = {"graph": bool(pipe._wf_graph), "ticks": []}
    admits = pipe.admit([0] * NR, inputs=[BIG if r % 2 == 0 else SMALL for r in range(NR)])
    log["admits"] = admits
    for t in range(TICKS):
        pipe.tick()
        step = {"done": pipe.drain_completed() if t % 3 == 2 else None}
        for k in TABLES + COUNTERS + COND_TABLES:
            step[k] = getattr(pipe, k).cpu().clone()
        log["ticks"].append(step)
    return log


@functools.lru_cache(maxsize=None)
def reference_log():
    return run_script("ref", "cpu")


def test_the_reference_run_branches_as_worked_out_by_hand():
    from cordum_amd.ops.wf_pipeline import WFS_FAILED, WFS_SKIPPED, WFS_SUCCEEDED

    log = reference_log()
    assert log["admits"][0] == list(range(NR))
    last = log["ticks"][-1]
    st, out = last["step_state"].view(NR, 64), last["step_out"].view(NR, 64)
    att = last["step_attempts"].view(NR, 64)
    took = skipped = retried = 0
    for r in range(NR):
        if int(st[r, 0]) == WFS_FAILED:                 # three failures in a row
            continue
        # the worker's one child that succeeded had ordinal = its attempts
        base = sum(BIG if r % 2 == 0 else SMALL)
        assert int(out[r, 0]) == base + int(att[r, 0])
        if r % 2 == 0:
            assert int(st[r, 1]) == WFS_SUCCEEDED and int(out[r, 1]) == 1
            took += 1
            retried += int(att[r, 2]) > 0
        else:
            assert st[r, 1:3].tolist() == [WFS_SKIPPED, WFS_SKIPPED]
            assert out[r, 1:3].tolist() == [0, 0]
            skipped += 1
    assert took > 20 and skipped > 20 and retried > 0
    assert int(last["retry_count"][0]) > 0
    done = [s["done"] for s in log["ticks"] if s["done"] is not None]
    assert sum(len(d[0]) for d in done) > 40


def assert_same(got, want):
    assert got["admits"] == want["admits"]
    for t, (g, w) in enumerate(zip(got["ticks"], want["ticks"])):
        for k in w:
            if torch.is_tensor(w[k]):
                assert torch.equal(g[k], w[k]), (t, k)
            else:
                assert g[k] == w[k], (t, k)


@pytest.mark.parametrize("graph", [True, False])
def test_branching_runs_match_the_reference_every_tick(monkeypatch, graph):
    if graph:
        monkeypatch.delenv("CORDUM_WF_NO_GRAPH", raising=False)
    else:
        monkeypatch.setenv("CORDUM_WF_NO_GRAPH", "1")
    got = run_script("ext", "cuda:0")
    assert got["graph"] is graph
    assert_same(got, reference_log())
