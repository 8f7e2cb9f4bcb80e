"""Rerun of a device run from a step, on the CPU reference backend:
`WorkflowPipeline.admit(keep=..., outs=...)` and `DeviceRunTable.rerun_from`,
against full runs of the same DAGs and against the host engine's
`Engine.rerun_from`."""
import json
import random

import pytest

from cordum_amd.ops.wf_pipeline import (
    DagSpec,
    StepSpec,
    WFK_DELAY,
    WFK_WORKER,
    WFS_PENDING,
    WFS_SKIPPED,
    WFS_SUCCEEDED,
    WorkflowPipeline,
)
from cordum_amd.workflow.device_runs import DeviceRunTable
from cordum_amd.workflow.models import RUN_SUCCEEDED, STEP_SUCCEEDED
from tests.test_device_runs import mk_pipe, random_dag, workflow_of

pytestmark = pytest.mark.timeout(300)


def closure(dag, s):
    """Mask of the transitive dependencies of step s."""
    seen, stack = set(), list(dag.steps[s].deps)
    while stack:
        d = stack.pop()
        if d not in seen:
            seen.add(d)
            stack.extend(dag.steps[d].deps)
    return sum(1 << d for d in seen)


def run_to_end(pipe, slot, limit=200):
    """Tick until `slot`'s run is reported; returns (ticks, final state)."""
    for t in range(1, limit + 1):
        pipe.tick()
        slots, _, states = pipe.drain_completed()
        if slot in slots:
            return t, states[slots.index(slot)]
    raise AssertionError("the run did not end")


def row(table, slot, n):
    return table[slot * 64:slot * 64 + n].tolist()


def random_cases(seed, count):
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        fan = rng.randint(1, 9)
        out.append((random_dag(rng, fan), fan))
    return out


# ---------------------------------------------------------------------------
# the pipeline: admit(keep=...)
# ---------------------------------------------------------------------------
def test_rerun_from_every_step_of_random_dags_ends_as_the_full_run():
    for dag, fan in random_cases(7, 10):
        pipe = mk_pipe([dag], dynamic_capacity=2)
        n = len(dag.steps)
        slots, _ = pipe.admit([0])
        full_ticks, full_state = run_to_end(pipe, slots[0])
        full = row(pipe.step_state, slots[0], n)
        assert full_state == WFS_SUCCEEDED and full == [WFS_SUCCEEDED] * n
        for s in range(n):
            keep = closure(dag, s)
            (slot,), _ = pipe.admit([0], keep=[keep])
            assert slot >= 0
            before = row(pipe.step_state, slot, n)
            assert before == [WFS_SUCCEEDED if keep >> d & 1 else WFS_PENDING
                              for d in range(n)]
            ticks, state = run_to_end(pipe, slot)
            assert state == full_state and row(pipe.step_state, slot, n) == full
            emitted = row(pipe.children_emitted, slot, n)
            assert all(emitted[d] == 0 for d in range(n) if keep >> d & 1)
            assert ticks <= full_ticks
            if keep == 0:
                assert ticks == full_ticks


def test_admit_refuses_an_open_or_out_of_range_set_with_minus_two():
    dag = DagSpec(steps=[StepSpec(WFK_WORKER), StepSpec(WFK_WORKER, deps=[0]),
                         StepSpec(WFK_WORKER, deps=[1])])
    pipe = mk_pipe([dag], dynamic_capacity=3)
    # closed, open (0 missing), bit at n_steps, closed with a skip, past the table
    slots, gens = pipe.admit([0] * 5, keep=[1, 2, 1 << 3, (3, 2), 0])
    assert slots == [0, -2, -2, -1, -1]          # three slots: request 3 is past them
    assert gens == [1, 0, 0, 0, 0]
    assert pipe.run_life.tolist() == [1, 0, 0]   # the refused requests' slots stay FREE
    assert int(pipe.admit_count[0]) == 1
    slots, _ = pipe.admit([0, 0], keep=[(3, 2), 1 << 63])
    assert slots == [1, -2]
    assert row(pipe.step_state, 1, 3) == [WFS_SUCCEEDED, WFS_SKIPPED, WFS_PENDING]


def test_admit_errors():
    dag = DagSpec(steps=[StepSpec(WFK_WORKER), StepSpec(WFK_WORKER, deps=[0])])
    pipe = mk_pipe([dag], dynamic_capacity=2)
    with pytest.raises(ValueError, match="skipped"):
        pipe.admit([0], keep=[(1, 2)])
    for bad in (1 << 64, -1, True, 1.0):
        with pytest.raises(ValueError, match="64-bit mask"):
            pipe.admit([0], keep=[bad])
    with pytest.raises(ValueError, match="length"):
        pipe.admit([0, 0], keep=[1])
    with pytest.raises(ValueError, match="device_conditions"):
        pipe.admit([0], keep=[1], outs=[{0: 5}])
    cpipe = mk_pipe([dag], dynamic_capacity=2, device_conditions=True, payload_words=10)
    with pytest.raises(ValueError, match="length"):
        cpipe.admit([0], keep=[1], outs=[])
    with pytest.raises(ValueError, match="not kept"):
        cpipe.admit([0], keep=[1], outs=[{1: 5}])
    with pytest.raises(ValueError, match="not kept"):
        cpipe.admit([0], keep=[1], outs=[[0, 5] + [0] * 62])
    with pytest.raises(ValueError, match="not kept"):
        cpipe.admit([0], outs=[{0: 5}])
    with pytest.raises(ValueError, match="int32"):
        cpipe.admit([0], keep=[1], outs=[{0: 1 << 31}])
    with pytest.raises(ValueError, match="64 entries"):
        cpipe.admit([0], keep=[1], outs=[[5]])
    assert int(cpipe.admit_count[0]) == 0 and int(pipe.admit_count[0]) == 0
    # the row form, with zeros where nothing is kept
    assert cpipe.admit([0], keep=[1], outs=[[5] + [0] * 63])[0] == [0]
    assert row(cpipe.step_out, 0, 2) == [5, 0]


def test_a_refused_request_leaves_the_last_slots_side_columns_alone():
    """-2 mod (NR + 1) is the table's last row: the columns written after the
    kernel must send every refusal to the spare row."""
    from cordum_amd.ops.wf_pipeline import CondSpec, WFK_CONDITION

    dag = DagSpec(steps=[StepSpec(WFK_DELAY, delay_ticks=50),
                         StepSpec(WFK_CONDITION, deps=[0])])
    other = DagSpec(steps=[StepSpec(WFK_WORKER), StepSpec(WFK_WORKER, deps=[0])])
    pipe = mk_pipe([dag, other], dynamic_capacity=2, device_conditions=True,
                   step_policy=True, payload_words=10)
    slots, _ = pipe.admit([0, 0], cond_bits=[2, 2], inputs=[[11, 12], [21, 22]])
    assert slots == [0, 1]
    before = (pipe.run_tmpl.tolist(), pipe.run_input.tolist(), pipe.step_out.tolist())
    assert before[0] == [0, 0] and before[2][64:66] == [0, 1]
    # not closed and out of range, with a full table and with room
    for _ in range(2):
        slots, _ = pipe.admit([1, 1, 1], inputs=[[7], [8], [9]],
                              keep=[2, 1 << 2, 0], outs=[{1: 99}, {2: 98}, None])
        assert slots[:2] == [-2, -2]
        assert (pipe.run_tmpl.tolist(), pipe.run_input.tolist(),
                pipe.step_out.tolist()) == before
        pipe.cancel([0], [1])
        pipe.tick()
        pipe.drain_completed()
        before = (pipe.run_tmpl.tolist(), pipe.run_input.tolist(), pipe.step_out.tolist())
    assert slots == [-2, -2, -1]


def test_the_journal_reports_a_kept_step_once_at_the_first_pass():
    dag = DagSpec(steps=[StepSpec(WFK_WORKER), StepSpec(WFK_WORKER, deps=[0]),
                         StepSpec(WFK_WORKER, deps=[1])])
    pipe = mk_pipe([dag], dynamic_capacity=1, event_cap=64)
    pipe.admit([0], keep=[(3, 2)])
    for _ in range(6):
        pipe.tick()
    _, _, steps, frm, to, stamps = pipe.drain_events()
    kept = [(s, f, t) for s, f, t in zip(steps, frm, to) if s < 2]
    assert sorted(kept) == [(0, WFS_PENDING, WFS_SUCCEEDED), (1, WFS_PENDING, WFS_SKIPPED)]
    first = min(stamps)
    assert all(st == first for s, st in zip(steps, stamps) if s < 2)


# ---------------------------------------------------------------------------
# conditions: the output words are carried
# ---------------------------------------------------------------------------
COND_WF = {"id": "wf-cond", "steps": {
    "z": {"type": "worker", "topic": "job.x", "condition": "input.x > 0"},
    "a": {"type": "worker", "topic": "job.x"},
    "c": {"type": "condition", "condition": "steps.a.output > 1000", "depends_on": ["a"]},
    "w": {"type": "worker", "topic": "job.x", "depends_on": ["c"],
          "condition": "steps.c.output"},
}}


def cond_table(retain=4):
    pipe = WorkflowPipeline("cpu", [], n_local_workers=4, backend="ref",
                            dynamic_capacity=2, child_cap=64, device_conditions=True,
                            payload_words=10)
    table = DeviceRunTable(pipe, retain=retain)
    assert table.register(COND_WF) == 0
    return pipe, table


def finish(table, want, limit=60):
    got = {}
    for _ in range(limit):
        table.tick()
        got.update(table.poll())
        if all(r in got for r in want):
            return got
    raise AssertionError(f"{want} did not end: {got}")


def test_rerun_from_a_condition_keeps_the_output_it_reads():
    pipe, table = cond_table()
    assert table.submit("big", 0, input={"x": 1100})
    slot = table.handle("big")[0]
    finish(table, ["big"])
    # a worker's word is x + ordinal 0 + its step index
    assert row(pipe.step_out, slot, 4) == [1100, 1101, 1, 1100 + 3]
    new = table.rerun_from("big", "c", new_run_id="big-2")
    assert new == "big-2"
    slot = table.handle(new)[0]
    assert row(pipe.step_state, slot, 4) == [WFS_PENDING, WFS_SUCCEEDED, WFS_PENDING,
                                             WFS_PENDING]
    assert table.step_outputs(new) == {"z": 0, "a": 1101, "c": 0, "w": 0}
    finish(table, [new])
    assert row(pipe.step_state, slot, 4) == [WFS_SUCCEEDED] * 4
    assert row(pipe.step_out, slot, 4) == [1100, 1101, 1, 1100 + 3]
    assert row(pipe.children_emitted, slot, 4) == [1, 0, 0, 1]
    # the same admission with the word left 0 decides the other way
    (slot,), _ = pipe.admit([0], inputs=[[1100]], keep=[1 << 1])
    for _ in range(8):
        pipe.tick()
    assert row(pipe.step_state, slot, 4) == [WFS_SUCCEEDED, WFS_SUCCEEDED, WFS_SKIPPED,
                                             WFS_SKIPPED]
    assert row(pipe.step_out, slot, 4)[1:3] == [0, 0]


@pytest.mark.parametrize("x,c_state", [(1100, WFS_SUCCEEDED), (5, WFS_SKIPPED)])
def test_a_kept_condition_step_keeps_its_decision(x, c_state):
    pipe, table = cond_table()
    table.submit("r", 0, input={"x": x})
    finish(table, ["r"])
    new = table.rerun_from("r", "w")
    slot = table.handle(new)[0]
    truth = int(c_state == WFS_SUCCEEDED)
    assert row(pipe.step_state, slot, 4) == [WFS_PENDING, WFS_SUCCEEDED, c_state, WFS_PENDING]
    assert table.step_outputs(new)["c"] == truth
    assert int(pipe.cond_bits[slot]) >> 2 & 1 == truth
    finish(table, [new])
    assert row(pipe.step_state, slot, 4)[3] == (WFS_SUCCEEDED if truth else WFS_SKIPPED)
    assert row(pipe.children_emitted, slot, 4) == [1, 0, 0, truth]
    # whatever the caller passes for a kept CONDITION step, the state decides
    (slot,), _ = pipe.admit([0], inputs=[[x]], keep=[(6, 4 * (1 - truth))],
                            outs=[{1: 77, 2: 1 - truth}])
    assert row(pipe.step_out, slot, 4) == [0, 77, truth, 0]
    assert int(pipe.cond_bits[slot]) >> 2 & 1 == truth
    # ... and without any outs
    pipe.cancel([slot], [pipe.run_gen[slot].item()])
    pipe.drain_completed()
    (slot,), _ = pipe.admit([0], inputs=[[x]], keep=[(6, 4 * (1 - truth))])
    assert row(pipe.step_out, slot, 4) == [0, 0, truth, 0]


# ---------------------------------------------------------------------------
# against the host engine
# ---------------------------------------------------------------------------
class Host:
    """The harness of tests.test_wf_pipeline._host_oracle_run, kept open so
    that a finished run can be rerun: an auto-succeeding worker, approvals
    granted, timers pumped."""

    def __init__(self, dag, fan):
        from cordum_amd.bus import LoopbackBus
        from cordum_amd.protocol import subjects as subj
        from cordum_amd.store import MemoryStore
        from cordum_amd.utils.clock import ManualClock
        from cordum_amd.workflow import Engine, WorkflowRun, WorkflowStore

        self.clock = ManualClock()
        bus = LoopbackBus(clock=self.clock)
        self.store = WorkflowStore(clock=self.clock)
        self.memory = MemoryStore(clock=self.clock)
        self.engine = Engine(self.store, bus, memory=self.memory, clock=self.clock)
        self.pending = []
        bus.subscribe(subj.SUBJECT_SUBMIT, lambda s, p: self.pending.append(p.job_request))
        self.store.put_workflow(workflow_of(dag))
        self.store.create_run(WorkflowRun(id="r1", workflow_id="wf", org_id="org",
                                          input={"items": list(range(fan))}))

    def run(self, run_id):
        """Start `run_id` and drive it to its end; returns (status, the set
        of step ids a job was dispatched for)."""
        from cordum_amd.protocol.capv2 import JobResult, JobStatus
        from cordum_amd.workflow.engine import split_for_each_step, split_job_id

        dispatched = set()
        self.engine.start_run("wf", run_id)
        for _ in range(10000):
            if self.pending:
                req = self.pending.pop(0)
                rid, step = split_job_id(req.job_id)
                assert rid == run_id
                dispatched.add(split_for_each_step(step)[0])
                ptr = self.memory.put_result(req.job_id, json.dumps({"ok": 1}).encode())
                self.engine.handle_job_result(JobResult(
                    job_id=req.job_id, status=JobStatus.SUCCEEDED, result_ptr=ptr))
                continue
            r = self.store.get_run(run_id)
            if r.status in ("succeeded", "failed", "cancelled", "timed_out"):
                return r.status, dispatched
            if r.status == "waiting":
                for sid, sr in list(r.steps.items()):
                    if sr.status == "waiting":
                        self.engine.approve_step(run_id, sid, True)
                continue
            self.clock.advance(30)
            self.engine.pump_timers()
        raise AssertionError("the host engine did not converge")


def test_rerun_dispatches_the_steps_the_host_engine_dispatches():
    for dag, fan in random_cases(11, 8):
        host = Host(dag, fan)
        assert host.run("r1")[0] == RUN_SUCCEEDED
        pipe = mk_pipe([], dynamic_capacity=2)
        table = DeviceRunTable(pipe, retain=8)
        tmpl = table.register(workflow_of(dag), items_len=fan)
        assert table.submit("r1", tmpl)
        assert finish(table, ["r1"], 200) == {"r1": RUN_SUCCEEDED}
        n = len(dag.steps)
        for s in range(n):
            new = host.engine.rerun_from("r1", f"s{s}")
            status, want = host.run(new)
            dev = table.rerun_from("r1", f"s{s}")
            slot = table.handle(dev)[0]
            got = finish(table, [dev], 200)
            emitted = row(pipe.children_emitted, slot, n)
            assert {f"s{d}" for d in range(n) if emitted[d] > 0} == want, (dag, s)
            assert got[dev] == status
            kept = closure(dag, s)
            assert not any(f"s{d}" in want for d in range(n) if kept >> d & 1)


def test_rerun_errors_are_the_host_engines():
    dag = DagSpec(steps=[StepSpec(WFK_DELAY, delay_ticks=3), StepSpec(WFK_WORKER, deps=[0])])
    host = Host(dag, 1)
    table = DeviceRunTable(mk_pipe([], dynamic_capacity=2))
    tmpl = table.register(workflow_of(dag), items_len=1)
    table.submit("r1", tmpl)                # neither run has started a step
    for args in (("",), ("r1", "nope"), ("r1", "s1")):
        with pytest.raises(ValueError) as h:
            host.engine.rerun_from(*args)
        with pytest.raises(ValueError) as d:
            table.rerun_from(*args)
        assert str(d.value) == str(h.value)
    assert str(d.value) == "dependency s0 not succeeded"
    with pytest.raises(KeyError):
        table.rerun_from("nobody", "s1")
    with pytest.raises(ValueError, match="already live or queued"):
        table.rerun_from("r1", "", new_run_id="r1")
    # step "" keeps nothing, on a run in any state; the id is a fresh one
    new = table.rerun_from("r1")
    assert new not in ("", "r1") and table.handle(new) == (1, 1)
    assert table.rerun_from("r1", 0) != new   # by index; s0 has no dependency


# ---------------------------------------------------------------------------
# the run table: retention, the FIFO, the store, the events
# ---------------------------------------------------------------------------
CHAIN = DagSpec(steps=[StepSpec(WFK_WORKER), StepSpec(WFK_WORKER, deps=[0]),
                       StepSpec(WFK_WORKER, deps=[1])])


def test_retention_keeps_the_last_completed_runs_and_no_more():
    table = DeviceRunTable(mk_pipe([], dynamic_capacity=1), retain=2)
    tmpl = table.register(workflow_of(CHAIN))
    for rid in ("r1", "r2", "r3"):
        table.submit(rid, tmpl)
        finish(table, [rid])
    with pytest.raises(KeyError):
        table.rerun_from("r1", "s2")
    a = table.rerun_from("r2", "s2")
    assert table.step_states(a) == {"s0": STEP_SUCCEEDED, "s1": STEP_SUCCEEDED,
                                    "s2": "pending"}
    finish(table, [a])                      # r2 leaves, r3 and the rerun stay
    with pytest.raises(KeyError):
        table.rerun_from("r2", "s2")
    finish(table, [table.rerun_from("r3", "s1"), ])
    none = DeviceRunTable(mk_pipe([], dynamic_capacity=1))
    tmpl = none.register(workflow_of(CHAIN))
    none.submit("r1", tmpl)
    assert none.rerun_from("r1", "s0")      # resident: no retention needed
    finish(none, ["r1"])
    with pytest.raises(KeyError):
        none.rerun_from("r1", "s2")
    with pytest.raises(ValueError):
        DeviceRunTable(mk_pipe([], dynamic_capacity=1), retain=-1)


def test_a_rerun_waits_in_the_fifo_when_the_table_is_full():
    pipe = mk_pipe([], dynamic_capacity=1)
    table = DeviceRunTable(pipe, retain=1)
    tmpl = table.register(workflow_of(CHAIN))
    table.submit("r1", tmpl)
    finish(table, ["r1"])
    assert table.submit("busy", tmpl)
    new = table.rerun_from("r1", "s2", new_run_id="again")
    assert table.handle(new) is None and table.queued() == 1
    assert table.submit("late", tmpl) is False and table.queued() == 2
    with pytest.raises(ValueError, match="already live or queued"):
        table.rerun_from("r1", "s2", new_run_id="again")
    # a queued run has finished nothing, but can be rerun from its first step
    with pytest.raises(ValueError, match="dependency s0 not succeeded"):
        table.rerun_from("again", "s1")
    finish(table, ["busy"])                 # that poll admits the queue's head
    assert table.handle("again") == (0, 3) and table.queued() == 1
    assert row(pipe.step_state, 0, 3) == [WFS_SUCCEEDED, WFS_SUCCEEDED, WFS_PENDING]
    for _ in range(6):
        table.tick()
    assert row(pipe.children_emitted, 0, 3) == [0, 0, 1]
    assert table.poll() == [("again", RUN_SUCCEEDED)]   # and admits the next one
    assert table.handle("late") == (0, 4)


def stored_table():
    from cordum_amd.workflow.models import WorkflowRun
    from cordum_amd.workflow.store import WorkflowStore

    pipe = mk_pipe([], dynamic_capacity=2, event_cap=256)
    store = WorkflowStore()
    table = DeviceRunTable(pipe, store=store, retain=2)
    tmpl = table.register(workflow_of(CHAIN))
    store.create_run(WorkflowRun(id="r1", workflow_id="wf", org_id="org", team_id="t",
                                 input={"items": [1, 2]}, labels={"k": "v"},
                                 metadata={"m": "1"}))
    table.submit("r1", tmpl)
    finish(table, ["r1"])
    return pipe, store, table


def test_the_store_record_of_a_rerun_has_the_host_engines_fields():
    pipe, store, table = stored_table()
    src = store.get_run("r1")
    new = table.rerun_from("r1", "s2")
    rec = store.get_run(new)
    assert (rec.rerun_of, rec.rerun_step, rec.workflow_id) == ("r1", "s2", "wf")
    assert (rec.org_id, rec.team_id, rec.labels) == ("org", "t", {"k": "v"})
    assert rec.metadata == {"m": "1", "rerun_of": "r1", "rerun_step": "s2"}
    assert rec.input == src.input and rec.input is not src.input
    assert sorted(rec.steps) == ["s0", "s1"]
    assert all(sr.status == STEP_SUCCEEDED for sr in rec.steps.values())
    assert rec.steps["s0"] is not src.steps["s0"]
    finish(table, [new])
    rec = store.get_run(new)
    assert rec.status == RUN_SUCCEEDED and rec.steps["s2"].status == STEP_SUCCEEDED
    # step "": no rerun_step in the metadata, nothing cloned
    rec = store.get_run(table.rerun_from("r1"))
    assert rec.rerun_step == "" and "rerun_step" not in rec.metadata and not rec.steps
    # a source the store does not hold: the rerun runs, nothing is recorded
    table.submit("loose", 0)
    finish(table, ["loose"])
    with pytest.raises(KeyError):
        store.get_run(table.rerun_from("loose", "s1"))


def test_events_of_kept_steps_are_dropped():
    pipe, store, table = stored_table()
    table.take_events()
    new = table.rerun_from("r1", "s2")
    finish(table, [new])
    events = table.take_events()
    assert events and {e.run_id for e in events} == {new}
    assert {e.step_id for e in events} == {"s2"}
    assert events[-1].to_state == WFS_SUCCEEDED
    assert {e.step_id for e in store.get_timeline(new) if e.step_id} == {"s2"}
    # a full run of the same table reports every step
    table.submit("full", 0)
    finish(table, ["full"])
    assert {e.step_id for e in table.take_events()} == {"s0", "s1", "s2"}
