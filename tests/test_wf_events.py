"""The step-transition journal through WorkflowPipeline and DeviceRunTable, on
the CPU reference backend.

The churn script is the one of tests/test_gpu_wf_dynamic.py (same seeds, same
decisions) with the journal drained every tick; `run_event_churn` is
module-level so tests/test_gpu_wf_events.py runs it on the GPU.
"""
import functools
import random

import pytest
import torch

from cordum_amd.ops.wf_pipeline import (
    DagSpec, StepSpec, WFK_APPROVAL, WFK_CONDITION, WFK_DELAY, WFK_FOR_EACH,
    WFK_WORKER, WFL_FREE, WFS_CANCELLED, WFS_DISPATCHED, WFS_FAILED, WFS_PENDING,
    WFS_SKIPPED, WFS_SUCCEEDED, WFS_WAITING, WorkflowPipeline)
from tests import test_gpu_wf_dynamic as D

AMPLE = 2 * D.CAPACITY * 64     # one event per step per pass, two passes a drain
TIGHT = 8


class Replay:
    """Step images rebuilt from drained events alone, per (slot, gen), from
    all-PENDING; checks the chain contract while it applies them."""

    def __init__(self):
        self.image = {}

    def apply(self, events):
        slots, gens, steps, frm, to, stamps = events
        assert len({len(c) for c in events}) == 1
        last_stamp = {}
        for ev in zip(slots, gens, steps, frm, to, stamps):
            slot, gen, step, f, t, stamp = ev
            row = self.image.setdefault((slot, gen), [WFS_PENDING] * 64)
            assert row[step] == f, f"chain broken at {ev}: image holds {row[step]}"
            assert f != t, ev
            row[step] = t
            # one event per step and stamp within a list
            assert last_stamp.get((slot, gen, step)) != stamp, ev
            last_stamp[(slot, gen, step)] = stamp

    def assert_is(self, pipe):
        """The images equal step_state on every row that is not FREE."""
        life = pipe.run_life.cpu().tolist()
        gen = pipe.run_gen.cpu().tolist()
        state = pipe.step_state.cpu().view(-1, 64).tolist()
        for r, lf in enumerate(life):
            if lf != WFL_FREE:
                want = self.image.get((r, gen[r]), [WFS_PENDING] * 64)
                assert state[r] == want, f"row {r} gen {gen[r]}"


def run_event_churn(backend, device, event_cap, check=True):
    """D.run_churn with the journal on and drained at the top of every tick,
    before drain_completed(). With `check`, the replayed images are compared
    with step_state after every drain."""
    dags = D.churn_dags()
    pipe = WorkflowPipeline(device=device, dags=dags, backend=backend,
                            n_local_workers=D.WORKERS, payload_words=D.WORDS,
                            fail_ppt=100, max_retries=1,
                            dynamic_capacity=D.CAPACITY, event_cap=event_cap)
    rng = random.Random(17)
    live, retired = [], []
    replay = Replay()
    log = {"records": [], "admits": [], "cancels": [], "events": []}
    for tick in range(D.TICKS):
        events = pipe.drain_events()
        log["events"].append(events)
        if check:
            assert list(events[5]) == sorted(events[5])      # time order
            replay.apply(events)
            replay.assert_is(pipe)
        slots, gens, states = pipe.drain_completed()
        for rec in zip(slots, gens, states):
            log["records"].append((tick,) + rec)
            live.remove(rec[:2])
            retired.append(rec[:2])
        n = D.CAPACITY + 10 if tick == 0 else rng.randint(5, 45)
        tmpl = [rng.randrange(len(dags)) for _ in range(n)]
        fan = [rng.choice([0, 0, rng.randint(1, D.MAX_FAN)]) for _ in range(n)]
        cond = [rng.getrandbits(64) for _ in range(n)]
        got = pipe.admit(tmpl, cond_bits=cond, fanout=fan)
        log["admits"].append(got)
        live += [(s, g) for s, g in zip(*got) if s >= 0]
        req = [h for h in live if rng.random() < 0.06]
        if retired and rng.random() < 0.5:
            req.append(rng.choice(retired))        # a stale handle
        ok = pipe.cancel([h[0] for h in req], [h[1] for h in req])
        log["cancels"].append(ok)
        pipe.tick()
    events = pipe.drain_events()
    log["events"].append(events)
    if check:
        replay.apply(events)
        replay.assert_is(pipe)
    log["tables"] = {k: getattr(pipe, k).cpu().clone() for k in D.TABLES}
    log["counters"] = {k: getattr(pipe, k).cpu().clone() for k in D.COUNTERS}
    log["graph"] = bool(pipe._wf_graph)
    log["event_overflows"] = pipe.event_overflows
    log["shadow"] = pipe.ev_shadow_state.cpu().clone()
    return log


@functools.lru_cache(maxsize=None)
def reference_events(event_cap):
    return run_event_churn("ref", "cpu", event_cap)


def _ref_pipe(dags, capacity, event_cap, **kw):
    return WorkflowPipeline(device="cpu", dags=dags, backend="ref", n_local_workers=16,
                            payload_words=4, dynamic_capacity=capacity,
                            event_cap=event_cap, **kw)


# 1 + 2: replay reproduces step_state at every tick (asserted inside the
# driver), and an ample list never overflows
def test_replayed_events_reproduce_step_state_every_tick():
    log = reference_events(AMPLE)
    assert log["event_overflows"] == 0
    flat = [list(zip(*e)) for e in log["events"]]
    tos = {ev[4] for evs in flat for ev in evs}
    # children are applied in the tick that emits them here, so DISPATCHED
    # and the retry's return to PENDING coalesce away (see the lost-children
    # test below for those)
    assert {WFS_SUCCEEDED, WFS_FAILED, WFS_SKIPPED, WFS_CANCELLED} <= tos
    # cancel passes are stamped between ticks, tick passes on the tick
    assert {ev[5] & 1 for evs in flat for ev in evs} == {0, 1}
    assert all(ev[4] == WFS_CANCELLED for evs in flat for ev in evs if ev[5] & 1)
    # a worker step dispatched and completed inside one tick is one event
    assert any(ev[3] == WFS_PENDING and ev[4] == WFS_SUCCEEDED for evs in flat for ev in evs)
    # the stamp's tick is the tick of detection. Drain i follows tick i-1
    # (device ticks count from 0) and, before it, the cancel pass that ran
    # while the device counter still read i-2 (-1 before the first tick).
    for i, evs in enumerate(flat):
        assert all(ev[5] >> 1 == (i - 2 if ev[5] & 1 else i - 1) for ev in evs), i


# 3: a tight list overflows, and loses nothing
def test_a_tight_event_list_overflows_and_still_replays():
    log = reference_events(TIGHT)
    assert log["event_overflows"] > 0
    ample = reference_events(AMPLE)
    assert torch.equal(log["shadow"], ample["shadow"])
    # per step the same first `from` and last `to`, whatever was coalesced
    def ends(l):
        out = {}
        for evs in l["events"]:
            for slot, gen, step, f, t, _ in zip(*evs):
                out[(slot, gen, step)] = (out.get((slot, gen, step), (f,))[0], t)
        return out
    assert ends(log) == ends(ample)


# 4: the journal observes: the engine computes the same with it and without
@pytest.mark.parametrize("event_cap", (AMPLE, TIGHT))
def test_the_journal_changes_nothing_the_engine_computes(event_cap):
    D.assert_same_run(reference_events(event_cap), D.reference_run())


# 5 + 6
def test_event_cap_needs_dynamic_mode_and_a_positive_size():
    dag = DagSpec.fanout_approval(4)
    with pytest.raises(ValueError, match="dynamic_capacity"):
        WorkflowPipeline(device="cpu", dags=[dag], backend="ref", event_cap=64)
    with pytest.raises(ValueError, match=">= 1"):
        _ref_pipe([dag], 4, 0)


def test_drain_events_needs_the_journal():
    dag = DagSpec.fanout_approval(4)
    pipe = _ref_pipe([dag], 4, None)
    assert not hasattr(pipe, "ev_rec")                 # nothing allocated
    with pytest.raises(RuntimeError, match="event_cap"):
        pipe.drain_events()
    static = WorkflowPipeline(device="cpu", dags=[dag], backend="ref")
    with pytest.raises(RuntimeError, match="dynamic"):
        static.drain_events()


def test_no_journal_pass_is_launched_without_event_cap():
    dag = DagSpec.fanout_approval(4)
    for cap, want in ((None, 0), (64, 2)):             # one tick + one cancel
        pipe = _ref_pipe([dag], 4, cap)
        calls = []
        real = pipe.ext.wf_journal
        pipe.ext.wf_journal = lambda *a: (calls.append(a[4]), real(*a))
        slots, gens = pipe.admit([0])
        pipe.tick()
        assert pipe.cancel(slots, gens) == [1]
        assert len(calls) == want and calls == [0, 1][:want]


# 7: cancel, drain and admit of the same slot between two ticks
def test_cancel_events_belong_to_the_old_generation():
    dag = DagSpec(steps=[StepSpec(WFK_WORKER), StepSpec(WFK_DELAY, deps=[0], delay_ticks=9),
                         StepSpec(WFK_WORKER, deps=[1])])
    pipe = _ref_pipe([dag], 1, 64)
    (slot,), (gen,) = pipe.admit([0])
    pipe.tick()
    pipe.tick()
    assert pipe.cancel([slot], [gen]) == [1]
    assert pipe.drain_completed() == ([slot], [gen], [WFS_CANCELLED])
    (slot2,), (gen2,) = pipe.admit([0])
    assert slot2 == slot and gen2 == gen + 1           # the slot is reused at once
    ev = list(zip(*pipe.drain_events()))
    cancelled = [e for e in ev if e[4] == WFS_CANCELLED]
    assert sorted(e[2] for e in cancelled) == [1, 2]
    assert all(e[1] == gen and e[3] == WFS_PENDING and e[5] & 1 for e in cancelled)
    assert all(e[1] == gen for e in ev)                # nothing lands on the new run
    pipe.tick()
    ev = list(zip(*pipe.drain_events()))
    assert ev and all(e[1] == gen2 for e in ev)
    assert all(e[3] == WFS_PENDING for e in ev)        # the new run starts from PENDING
    assert WFS_CANCELLED not in {e[4] for e in ev}


def test_lost_children_show_dispatched_and_the_retry():
    """Every child result dropped: the step stays DISPATCHED across ticks,
    times out back to PENDING (the retry), and fails after max_retries."""
    pipe = _ref_pipe([DagSpec(steps=[StepSpec(WFK_WORKER)])], 2, 64,
                     drop_ppt=1000, max_retries=1, timeout_cutoff=3)
    pipe.admit([0])
    replay, seen = Replay(), []
    for _ in range(40):
        pipe.tick()
        ev = pipe.drain_events()
        replay.apply(ev)
        replay.assert_is(pipe)
        seen += list(zip(ev[3], ev[4]))
        if pipe.drain_completed()[0]:
            break
    assert seen[0] == (WFS_PENDING, WFS_DISPATCHED)
    assert (WFS_DISPATCHED, WFS_PENDING) in seen
    assert seen[-1][1] == WFS_FAILED


# 8: DeviceRunTable + WorkflowStore
def _workflow():
    from cordum_amd.workflow.models import Workflow

    return Workflow.from_dict({"id": "wf-journal", "steps": {
        "seed": {"type": "worker", "topic": "job.x"},
        "fan": {"type": "worker", "topic": "job.x", "for_each": "input.items",
                "max_parallel": 2, "depends_on": ["seed"]},
        "gate": {"type": "approval", "depends_on": ["fan"]},
        "final": {"type": "worker", "topic": "job.x", "depends_on": ["gate"]},
    }})


def _table(approval_verdict=1):
    from cordum_amd.workflow.device_runs import DeviceRunTable
    from cordum_amd.workflow.models import WorkflowRun
    from cordum_amd.workflow.store import WorkflowStore

    pipe = _ref_pipe([], 4, 512, approval_verdict=approval_verdict)
    store = WorkflowStore()
    table = DeviceRunTable(pipe, store=store)
    tmpl = table.register(_workflow(), items_len=3)
    assert tmpl == 0
    for rid in ("r1", "r2"):
        store.create_run(WorkflowRun(id=rid, workflow_id="wf-journal"))
    return table, store, tmpl


def test_timeline_of_follows_the_mapping_table():
    from cordum_amd.workflow.device_runs import timeline_of

    K = {"worker": WFK_WORKER, "for_each": WFK_FOR_EACH, "approval": WFK_APPROVAL,
         "condition": WFK_CONDITION, "delay": WFK_DELAY}
    want = {
        ("worker", WFS_DISPATCHED): ("step_dispatched", "running", {}),
        ("for_each", WFS_DISPATCHED): ("step_dispatched", "running", {}),
        ("approval", WFS_WAITING): ("step_waiting", "waiting", {}),
        ("worker", WFS_SUCCEEDED): ("step_completed", "succeeded", {}),
        ("for_each", WFS_SUCCEEDED): ("step_completed", "succeeded", {}),
        ("approval", WFS_SUCCEEDED): ("step_approved", "succeeded", {}),
        ("delay", WFS_SUCCEEDED): ("step_delay_completed", "succeeded", {}),
        ("condition", WFS_SUCCEEDED): ("step_condition_evaluated", "succeeded", {"value": True}),
        # the host engine completes a false condition as succeeded, value False
        ("condition", WFS_SKIPPED): ("step_condition_evaluated", "succeeded", {"value": False}),
        ("approval", WFS_FAILED): ("step_rejected", "failed", {}),
        ("worker", WFS_FAILED): ("step_completed", "failed", {}),
        ("for_each", WFS_FAILED): ("step_completed", "failed", {}),
        ("for_each", WFS_PENDING): ("step_retry_scheduled", "pending", {}),
        ("worker", WFS_CANCELLED): ("step_cancelled", "cancelled", {}),
        ("approval", WFS_CANCELLED): ("step_cancelled", "cancelled", {}),
    }
    for (kind, to), expect in want.items():
        assert timeline_of(K[kind], to) == expect, (kind, to)


def test_device_run_table_fills_the_store():
    table, store, tmpl = _table()
    assert table.submit("r1", tmpl, fanout=3)
    assert table.step_states("r1") == {k: "pending" for k in ("seed", "fan", "gate", "final")}
    waited = False
    before, status = [], None
    for _ in range(40):
        table.tick()
        done = dict(table.poll())
        before += table.take_events()
        states = table.step_states("r1") if table.handle("r1") else None
        if states and states["gate"] == "waiting":
            waited = True
            assert store.get_run("r1").steps["gate"].status == "waiting"
            assert states["fan"] == "succeeded" and states["final"] == "pending"
        if "r1" in done:
            status = done["r1"]
            break
    assert status == "succeeded" and waited
    # every event was delivered before the completion: the replay is terminal
    image = {}
    for ev in before:
        assert ev.run_id == "r1" and image.get(ev.step_id, WFS_PENDING) == ev.from_state
        image[ev.step_id] = ev.to_state
    assert image == {k: WFS_SUCCEEDED for k in ("seed", "fan", "gate", "final")}
    for _ in range(3):
        table.tick()
        assert table.poll() == [] and table.take_events() == []
    # the timeline: one entry per event in order, then the run's status
    tl = store.get_timeline("r1")
    assert [e.type for e in tl[:-1]] == [
        {WFS_DISPATCHED: "step_dispatched", WFS_WAITING: "step_waiting",
         WFS_PENDING: "step_retry_scheduled",
         WFS_SUCCEEDED: "step_approved" if ev.step_id == "gate" else "step_completed",
         }[ev.to_state] for ev in before]
    assert all(e.run_id == "r1" and e.workflow_id == "wf-journal" for e in tl)
    assert [e.data["tick"] for e in tl[:-1]] == [ev.tick for ev in before]
    by_step = {}
    for e in tl[:-1]:
        by_step.setdefault(e.step_id, []).append((e.type, e.status))
    assert by_step["seed"][-1] == ("step_completed", "succeeded")
    assert by_step["gate"] == [("step_waiting", "waiting"), ("step_approved", "succeeded")]
    assert by_step["fan"][-1] == ("step_completed", "succeeded")
    assert by_step["final"][-1] == ("step_completed", "succeeded")
    assert (tl[-1].type, tl[-1].status) == ("run_status", "succeeded")
    run = store.get_run("r1")
    assert run.status == "succeeded" and run.completed_at is not None
    assert {k: v.status for k, v in run.steps.items()} == {
        k: "succeeded" for k in ("seed", "fan", "gate", "final")}


def test_device_run_table_reports_a_cancelled_run_after_its_events():
    table, store, tmpl = _table()
    assert table.submit("r2", tmpl, fanout=3)
    assert table.submit("ghost", tmpl, fanout=3)       # a run the store does not know
    table.tick()
    assert table.poll() == []
    assert table.cancel("r2")
    done = dict(table.poll())
    assert done == {"r2": "cancelled"}
    ev = [e for e in table.take_events() if e.run_id == "r2"]
    cancelled = {e.step_id for e in ev if e.to_state == WFS_CANCELLED}
    assert {"gate", "final"} <= cancelled and all(
        e.between_ticks for e in ev if e.to_state == WFS_CANCELLED)
    tl = store.get_timeline("r2")
    assert (tl[-1].type, tl[-1].status) == ("run_status", "cancelled")
    assert {e.step_id for e in tl if e.type == "step_cancelled"} == cancelled
    run = store.get_run("r2")
    assert run.status == "cancelled"
    assert all(run.steps[s].status == "cancelled" for s in cancelled)
    assert store.get_timeline("ghost") == []           # skipped silently
    with pytest.raises(KeyError):
        table.step_states("r2")


def test_a_rejected_approval_fails_the_run_in_the_store():
    table, store, tmpl = _table(approval_verdict=0)
    assert table.submit("r1", tmpl, fanout=3)
    status = None
    for _ in range(40):
        table.tick()
        done = dict(table.poll())
        if "r1" in done:
            status = done["r1"]
            break
    assert status == "failed"
    tl = store.get_timeline("r1")
    assert ("step_rejected", "failed") in [(e.type, e.status) for e in tl if e.step_id == "gate"]
    assert (tl[-1].type, tl[-1].status) == ("run_status", "failed")
    assert store.get_run("r1").steps["gate"].status == "failed"


def test_register_refuses_what_the_device_cannot_run():
    from cordum_amd.workflow.device_runs import DeviceRunTable
    from cordum_amd.workflow.models import Workflow

    table = DeviceRunTable(_ref_pipe([], 2, 64))
    wf = Workflow.from_dict({"id": "w", "steps": {
        "a": {"type": "worker"}, "b": {"type": "worker", "condition": "input.x > 1",
                                      "depends_on": ["a"]}}})
    assert table.register(wf) is None
    assert table.pipe.n_templates == 0
    # a template added without register(): events carry no step id
    t = table.pipe.add_template(DagSpec(steps=[StepSpec(WFK_WORKER)]))
    assert table.submit("x", t)
    table.tick()
    table.poll()
    ev = table.take_events()
    assert ev and all(e.step_id == "" and e.step == 0 for e in ev)
