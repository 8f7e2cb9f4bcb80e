"""GPU test of externally decided approvals through the pipeline: one
scripted schedule of admissions, decisions, a cancel and expiries gives, after
every tick, the same run tables, hold tables, counters, decision codes and
open_holds() on the HIP extension as on the CPU reference backend, with the
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

NR, FAN, TICKS = 65, 4, 16
HOLD_TABLES = ("hold_mask", "hold_gen", "hold_ttl", "hold_counts", "hold_open")


def script_dags():
    from cordum_amd.ops.wf_pipeline import (
        DagSpec, StepSpec, WFK_APPROVAL, WFK_FOR_EACH, WFK_WORKER)

    def gate(ttl):
        return DagSpec(steps=[StepSpec(WFK_FOR_EACH, fanout=FAN),
                              StepSpec(WFK_APPROVAL, deps=[0], ttl_ticks=ttl),
                              StepSpec(WFK_WORKER, deps=[1])])

    two = DagSpec(steps=[StepSpec(WFK_APPROVAL), StepSpec(WFK_WORKER),
                         StepSpec(WFK_APPROVAL, deps=[1], ttl_ticks=2),
                         StepSpec(WFK_WORKER, deps=[0, 2])])
    return [gate(0), gate(3), two]


def run_script(backend, device):
    from cordum_amd.ops.wf_pipeline import WorkflowPipeline

    pipe = WorkflowPipeline(device=device, dags=script_dags(), backend=backend,
                            n_local_workers=16, payload_words=4,
                            dynamic_capacity=NR, approvals="external", hold_cap=50)
    log = {"graph": bool(pipe._wf_graph), "ticks": []}
    retired = []
    for t in range(TICKS):
        slots, gens, states = pipe.drain_completed()
        retired += list(zip(slots, gens))
        n = NR + 3 if t == 0 else len(slots) + 1       # the table stays full
        admits = pipe.admit([(t + i) % 3 for i in range(n)])
        cancels = []
        if t == 4:                                     # a run with a hold open
            s, g, _, _ = pipe.open_holds()
            cancels = pipe.cancel(s[:1], g[:1])
        pipe.tick()
        holds = pipe.open_holds()
        # decide: approve or reject by arithmetic; slots with slot % 5 == 4
        # are left to expire (or to wait for ever); plus a stale handle and a
        # repeated pair
        req = [(s, g, st, int((s + t) % 3 != 0)) for s, g, st, _ in zip(*holds)
               if s % 5 != 4 and (s + st + t) % 2 == 0]
        if retired:
            req.append(retired[-1] + (1, 1))
        if req:
            req.append(req[0])
        codes = pipe.decide(*[list(c) for c in zip(*req)]) if req else []
        step = {"done": (slots, gens, states), "admits": admits, "cancels": cancels,
                "holds": holds, "codes": codes, "stats": pipe.hold_stats(),
                "after_decide": pipe.open_holds()}
        for k in TABLES + COUNTERS + HOLD_TABLES:
            step[k] = getattr(pipe, k).cpu().clone()
        # written only when a hold opens, so it is exact everywhere as well
        step["hold_tick"] = pipe.hold_tick.cpu().clone()
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
    ticks = reference_log()["ticks"]
    assert ticks[0]["admits"][0] == list(range(NR)) + [-1] * 3
    last = ticks[-1]["stats"]
    assert min(last["opened"], last["expired"], last["approved"], last["rejected"]) > 0
    assert last["open"] > 0
    assert ticks[4]["cancels"] == [1]
    assert any(len(s["holds"][0]) > 50 for s in ticks)            # more than one page
    assert {0, 1, 4} <= {c for s in ticks for c in s["codes"]}
    assert int(ticks[-1]["run_gen"].max()) >= 3                   # slots change hands
    assert any(s["after_decide"] != s["holds"] for s in ticks)


@pytest.mark.parametrize("graph", [True, False])
def test_scripted_approvals_match_reference_every_tick(monkeypatch, graph):
    if graph:
        monkeypatch.delenv("CORDUM_WF_NO_GRAPH", raising=False)
    else:
        monkeypatch.setenv("CORDUM_WF_NO_GRAPH", "1")
    got = run_script("ext", "cuda:0")
    assert got["graph"] is graph
    assert_same(got, reference_log())
