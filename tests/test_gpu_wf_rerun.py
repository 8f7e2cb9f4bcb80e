"""GPU test of reruns on the device workflow engine: one scripted churn that
admits runs with and without kept steps, invalid kept sets among them, and
reruns runs that completed from their final rows, gives exactly the same
admit results, completion records, counters and final tables on the HIP
extension as on the CPU reference backend. Both run in this process.

The check that the script is such a churn needs no GPU.
"""
import functools
import random

import pytest
import torch

CAPACITY, MAX_FAN, WORKERS, WORDS, TICKS = 130, 9, 16, 10, 40
TABLES = ("step_state", "step_attempts", "deps_mask", "step_kind", "children_todo",
          "max_parallel", "children_out", "children_done", "children_fail",
          "children_emitted", "next_ready", "dispatch_tick", "n_steps", "cond_bits",
          "run_state", "run_active", "run_life", "run_gen", "run_tmpl", "run_input",
          "step_out")
COUNTERS = ("wf_counts", "admit_count", "cancel_count", "retry_count",
            "timeout_count", "rq_dead", "tick_buf")


def churn_dags():
    """Approval-free random DAGs: worker, for_each, condition, delay."""
    from cordum_amd.ops.wf_pipeline import (
        DagSpec, StepSpec, WFK_CONDITION, WFK_DELAY, WFK_FOR_EACH, WFK_WORKER)

    rng = random.Random(5)
    dags = []
    for _ in range(10):
        steps = []
        for s in range(rng.randint(2, 7)):
            deps = [d for d in range(s) if rng.random() < 0.45]
            kind = rng.choice([WFK_WORKER, WFK_WORKER, WFK_FOR_EACH, WFK_CONDITION,
                               WFK_DELAY])
            steps.append(StepSpec(
                kind, deps=deps,
                fanout=rng.randint(1, MAX_FAN) if kind == WFK_FOR_EACH else 1,
                max_parallel=rng.choice([0, 0, 2, 3]) if kind == WFK_FOR_EACH else 0,
                delay_ticks=rng.randint(0, 2)))
        dags.append(DagSpec(steps=steps))
    return dags


def closure(dag, s):
    seen, stack = set(), list(dag.steps[s].deps)
    while stack:
        d = stack.pop()
        if d not in seen:
            seen.add(d)
            stack.extend(dag.steps[d].deps)
    return sum(1 << d for d in seen)


def run_churn(backend, device):
    """The scripted churn; every decision depends only on the script's own
    seed and on what the pipeline reported (drains are sorted by slot)."""
    from cordum_amd.ops.wf_pipeline import WFS_SKIPPED, WFS_SUCCEEDED, WorkflowPipeline

    dags = churn_dags()
    pipe = WorkflowPipeline(device=device, dags=dags, backend=backend,
                            n_local_workers=WORKERS, payload_words=WORDS,
                            fail_ppt=60, max_retries=1, device_conditions=True,
                            dynamic_capacity=CAPACITY)
    rng = random.Random(29)
    live = {}                  # (slot, gen) -> (template, cond, fanout, input)
    ended = []                 # (request, final states, final output words)
    log = {"records": [], "admits": [], "kinds": []}
    for tick in range(TICKS):
        slots, gens, states = pipe.drain_completed()
        if slots:
            # the rows of the runs just reported, before anything is admitted
            idx = torch.tensor(slots, dtype=torch.int64).to(device)
            st = pipe.step_state.view(-1, 64)[idx].cpu().tolist()
            out = pipe.step_out.view(-1, 64)[idx].cpu().tolist()
            for k, rec in enumerate(zip(slots, gens, states)):
                log["records"].append((tick,) + rec)
                ended.append((live.pop(rec[:2]), st[k], out[k]))
        n = CAPACITY + 10 if tick == 0 else rng.randint(10, 70)
        reqs, keep, outs, kinds = [], [], [], []
        for _ in range(n):
            how = rng.random()
            if ended and how < 0.45:
                # rerun a completed run from a step: what finished of that
                # step's dependencies is kept (of a failed run that may be
                # less than all of them; it is a closed set all the same)
                req, st, out = rng.choice(ended[-40:])
                s = rng.randrange(len(dags[req[0]].steps))
                want = closure(dags[req[0]], s)
                done = sum(1 << d for d in range(64)
                           if want >> d & 1 and st[d] in (WFS_SUCCEEDED, WFS_SKIPPED))
                skipped = sum(1 << d for d in range(64)
                              if done >> d & 1 and st[d] == WFS_SKIPPED)
                kinds.append("rerun" if done else "rerun-nothing")
                reqs.append(req)
                keep.append((done, skipped))
                outs.append({d: out[d] for d in range(64) if done >> d & 1})
                continue
            t = rng.randrange(len(dags))
            req = (t, rng.getrandbits(64), rng.choice([0, 0, rng.randint(1, MAX_FAN)]),
                   (rng.randint(-5, 2000), rng.randint(0, 9)))
            reqs.append(req)
            if how < 0.52:                  # any bits: out of range
                keep.append(rng.getrandbits(64) & rng.getrandbits(64))
                kinds.append("random")
            elif how < 0.6:                 # any of its steps: open or closed
                keep.append(rng.getrandbits(len(dags[t].steps)))
                kinds.append("subset")
            else:
                keep.append(0)
                kinds.append("plain")
            outs.append(None)
        args = dict(cond_bits=[r[1] for r in reqs], fanout=[r[2] for r in reqs],
                    inputs=[r[3] for r in reqs])
        if tick % 4 == 3:                   # a call without keep among them
            kinds = ["plain"] * n
            got = pipe.admit([r[0] for r in reqs], **args)
        else:
            got = pipe.admit([r[0] for r in reqs], keep=keep, outs=outs, **args)
        log["admits"].append(got)
        log["kinds"].append(kinds)
        for r, s, g in zip(reqs, *got):
            if s >= 0:
                live[(s, g)] = r
        pipe.tick()
    log["tables"] = {k: getattr(pipe, k).cpu().clone() for k in TABLES}
    log["counters"] = {k: getattr(pipe, k).cpu().clone() for k in COUNTERS}
    return log


def assert_same_run(got, want):
    assert got["kinds"] == want["kinds"]
    assert got["admits"] == want["admits"]
    assert got["records"] == want["records"]
    for k in COUNTERS:
        assert torch.equal(got["counters"][k], want["counters"][k]), k
    for k in TABLES:
        assert torch.equal(got["tables"][k], want["tables"][k]), k


@functools.lru_cache(maxsize=None)
def reference_run():
    return run_churn("ref", "cpu")


def test_the_script_is_a_churn_with_reruns():
    """The reference run of the script exercises what the comparison is
    about: a full table, both refusals in one call, reruns admitted with kept
    steps, kept sets that are refused, every outcome, slot reuse."""
    from cordum_amd.ops.wf_pipeline import WFS_FAILED, WFS_SUCCEEDED

    ref = reference_run()
    first = ref["admits"][0][0]             # more requests than slots
    assert all(s in (i, -2) for i, s in enumerate(first[:CAPACITY]))
    assert set(first[CAPACITY:]) == {-1, -2}
    seen = {}
    for kinds, (slots, _) in zip(ref["kinds"], ref["admits"]):
        for kind, slot in zip(kinds, slots):
            seen.setdefault(kind, set()).add(min(slot, 0))
    assert seen["rerun"] == {0, -1}             # admitted, or the table was full
    assert seen["random"] == {-2}               # refused, full or not
    assert seen["subset"] == {0, -1, -2} and seen["plain"] == {0, -1}
    calls = [set(s) for s, _ in ref["admits"]]
    assert any(-1 in c and -2 in c and max(c) >= 0 for c in calls)
    assert {WFS_SUCCEEDED, WFS_FAILED} == {r[3] for r in ref["records"]}
    assert int(ref["tables"]["run_gen"].max()) >= 3
    assert int(ref["counters"]["retry_count"][0]) > 0
    assert int(ref["counters"]["tick_buf"][0]) == TICKS - 1


@pytest.mark.gpu
def test_scripted_rerun_churn_matches_reference():
    got = run_churn("ext", "cuda:0")
    assert_same_run(got, reference_run())
