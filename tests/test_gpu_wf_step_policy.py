"""GPU test of the per-step retry / backoff / timeout policy through the
pipeline: one scripted schedule of admissions, a cancel and drains, on three
templates with different policies (one with a timeout longer than the
pipeline's cutoff), gives after every tick the same run tables, `run_tmpl` and
counters on the HIP extension as on the CPU reference backend, with the
captured tick graph and without it.

The script's decisions depend only on its own arithmetic and on what the
pipeline reported, so the two backends are driven identically as long as
they agree, and the first tick at which they do not is the one reported.
"""
import functools

import pytest
import torch

from tests.test_gpu_wf_dynamic import COUNTERS, TABLES

pytestmark = pytest.mark.gpu

NR, TICKS, CUTOFF, LONG = 65, 24, 8, 12
POLICY_TABLES = ("run_tmpl", "tmpl_policy", "tmpl_timeout")


def script_dags():
    from cordum_amd.ops.wf_pipeline import (
        DagSpec, RetrySpec, StepSpec, WFK_FOR_EACH, WFK_WORKER)

    return [
        # one retry after one tick; the second step on the pipeline's own policy
        DagSpec(steps=[StepSpec(WFK_FOR_EACH, fanout=4, retry=RetrySpec(1, 1, 256, 0)),
                       StepSpec(WFK_WORKER, deps=[0])]),
        # never retried; a windowed fan-out on 3, 5, 7, 10
        DagSpec(steps=[StepSpec(WFK_WORKER, retry=RetrySpec(0)),
                       StepSpec(WFK_FOR_EACH, fanout=3, max_parallel=2, timeout_ticks=10,
                                retry=RetrySpec(3, 3, 384, 10))]),
        # lost children are waited for LONG ticks, not CUTOFF
        DagSpec(steps=[StepSpec(WFK_WORKER, timeout_ticks=LONG,
                                retry=RetrySpec(2, 2, 512, 16)),
                       StepSpec(WFK_WORKER, deps=[0])]),
    ]


def run_script(backend, device):
    from cordum_amd.ops.wf_pipeline import WorkflowPipeline

    pipe = WorkflowPipeline(device=device, dags=script_dags(), backend=backend,
                            n_local_workers=16, payload_words=4, fail_ppt=250,
                            drop_ppt=150, max_retries=2, timeout_cutoff=CUTOFF,
                            dynamic_capacity=NR, step_policy=True)
    log = {"graph": bool(pipe._wf_graph), "ticks": []}
    for t in range(TICKS):
        slots, gens, states = pipe.drain_completed()
        n = NR + 3 if t == 0 else len(slots) + 1       # the table stays full
        admits = pipe.admit([(t + i) % 3 for i in range(n)])
        cancels = []
        if t == 4:                                     # the first run still active
            slot = int(torch.nonzero(pipe.run_active.cpu())[0])
            cancels = pipe.cancel([slot], [int(pipe.run_gen[slot].cpu())])
        pipe.tick()
        step = {"done": (slots, gens, states), "admits": admits, "cancels": cancels}
        for k in TABLES + COUNTERS + POLICY_TABLES:
            step[k] = getattr(pipe, k).cpu().clone()
        log["ticks"].append(step)
    return log


@functools.lru_cache(maxsize=None)
def reference_log():
    return run_script("ref", "cpu")


def assert_same(got, want):
    for t, (g, w) in enumerate(zip(got["ticks"], want["ticks"])):
        for k in w:
            if torch.is_tensor(w[k]):
                assert torch.equal(g[k], w[k]), (t, k)
            else:
                assert g[k] == w[k], (t, k)


def test_the_script_covers_what_it_is_about():
    from cordum_amd.ops.wf_pipeline import WFL_FREE, WFS_FAILED

    ticks = reference_log()["ticks"]
    assert ticks[0]["admits"][0] == list(range(NR)) + [-1] * 3
    assert ticks[4]["cancels"] == [1]
    last = ticks[-1]
    assert int(last["retry_count"][0]) > 0                         # a retry
    assert min(last["wf_counts"].tolist()) > 0
    assert int(last["run_gen"].max()) >= 3                         # slots change hands
    assert set(last["run_tmpl"].tolist()) == {0, 1, 2}
    # an exhaustion: a step with retries of its own FAILED with all of them used
    pol = last["tmpl_policy"].view(-1, 64, 4)
    exhausted = never = False
    for s in ticks:
        st, att = s["step_state"].view(NR, 64), s["step_attempts"].view(NR, 64)
        for r, c in torch.nonzero(st == WFS_FAILED).tolist():
            most = int(pol[int(s["run_tmpl"][r]), c, 0])
            assert int(att[r, c]) == most
            exhausted |= most > 0
            never |= most == 0
    assert exhausted and never
    # a policy timeout: children written off exactly LONG ticks after their
    # dispatch, in a row that is not FREE, and the counter grew by them
    found = 0
    for t in range(1, TICKS):
        a, b = ticks[t - 1], ticks[t]
        now = int(b["tick_buf"][0])
        rows = torch.nonzero((b["run_tmpl"] == 2) & (b["run_life"] != WFL_FREE)
                             & (a["run_gen"] == b["run_gen"])).flatten().tolist()
        for r in rows:
            i = r * 64
            if (int(a["children_out"][i]) > 0 and int(b["children_out"][i]) == 0
                    and int(a["dispatch_tick"][i]) == now - LONG):
                found += 1
                assert int(b["timeout_count"][0]) > int(a["timeout_count"][0])
    assert found > 0
    # and the cutoff still holds for the steps that did not ask for more
    assert int(ticks[CUTOFF + 1]["timeout_count"][0]) > 0


@pytest.mark.parametrize("graph", [True, False])
def test_scripted_step_policies_match_reference_every_tick(monkeypatch, graph):
    if graph:
        monkeypatch.delenv("CORDUM_WF_NO_GRAPH", raising=False)
    else:
        monkeypatch.setenv("CORDUM_WF_NO_GRAPH", "1")
    got = run_script("ext", "cuda:0")
    assert got["graph"] is graph
    assert_same(got, reference_log())
