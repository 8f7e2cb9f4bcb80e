"""Externally decided approvals (approvals="external") through
WorkflowPipeline and DeviceRunTable, on the CPU reference backend.

Device ticks count from 0: the n-th call of tick() is device tick n - 1, and
that is the number `since_ticks` and the journal's stamps carry.
"""
import pytest
import torch

from cordum_amd.ops.pipeline import _RefOps
from cordum_amd.ops.wf_pipeline import (
    DagSpec, StepSpec, WFK_APPROVAL, WFK_FOR_EACH, WFK_WORKER, WFL_LIVE,
    WFS_CANCELLED, WFS_FAILED, WFS_PENDING, WFS_SUCCEEDED, WFS_WAITING,
    WorkflowPipeline)
from cordum_amd.workflow.device_runs import DeviceRunTable, PendingApproval
from tests.test_wf_dynamic import AMPLE, random_dags

pytestmark = pytest.mark.timeout(300)

NEW_KERNELS = {"wf_hold_scan", "wf_hold_list", "wf_decide"}


def gate(ttl=0, fanout=0):
    """seed -> approval -> final; with `fanout` the seed is a for_each."""
    first = StepSpec(WFK_FOR_EACH, fanout=fanout) if fanout else StepSpec(WFK_WORKER)
    return DagSpec(steps=[first, StepSpec(WFK_APPROVAL, deps=[0], ttl_ticks=ttl),
                          StepSpec(WFK_WORKER, deps=[1])])


def mk(dags, capacity, **kw):
    kw.setdefault("approvals", "external")
    return WorkflowPipeline(device="cpu", dags=dags, backend="ref", n_local_workers=16,
                            payload_words=4, dynamic_capacity=capacity, **kw)


def tick_until_hold(pipe, limit=10):
    """Tick until a hold is open; returns open_holds() as a list of tuples."""
    for _ in range(limit):
        pipe.tick()
        holds = list(zip(*pipe.open_holds()))
        if holds:
            return holds
    raise AssertionError("no hold opened")


def dev_tick(pipe):
    return int(pipe.tick_buf[0])


def state(pipe, slot, step):
    return int(pipe.step_state[slot * 64 + step])


def test_a_hold_waits_until_someone_decides():
    pipe = mk([gate()], 4)
    assert pipe.admit([0]) == ([0], [1])
    (hold,) = tick_until_hold(pipe)
    h = dev_tick(pipe)
    assert hold == (0, 1, 1, h)
    for _ in range(10):
        pipe.tick()
        assert state(pipe, 0, 1) == WFS_WAITING and state(pipe, 0, 2) == WFS_PENDING
        assert int(pipe.run_active[0]) == 1 and int(pipe.run_life[0]) == WFL_LIVE
        assert list(zip(*pipe.open_holds())) == [hold]          # the tick is kept
    assert pipe.drain_completed() == ([], [], [])
    assert pipe.hold_stats() == {"opened": 1, "expired": 0, "approved": 0,
                                 "rejected": 0, "open": 1}


def test_approval_dispatches_the_dependent_on_the_next_tick():
    pipe = mk([gate()], 4)
    pipe.admit([0])
    tick_until_hold(pipe)
    assert pipe.decide([0], [1], [1], [1]) == [0]
    assert state(pipe, 0, 1) == WFS_SUCCEEDED
    assert pipe.open_holds() == ([], [], [], [])                # gone at once
    assert int(pipe.children_emitted[2]) == 0
    pipe.tick()
    assert int(pipe.children_emitted[2]) == 1                   # dispatched in that tick
    assert state(pipe, 0, 2) == WFS_SUCCEEDED
    assert pipe.drain_completed() == ([0], [1], [WFS_SUCCEEDED])
    assert pipe.hold_stats() == {"opened": 1, "expired": 0, "approved": 1,
                                 "rejected": 0, "open": 0}
    assert int(pipe.hold_mask[0]) == 0                          # the scan closed it


def test_rejection_fails_the_run():
    pipe = mk([gate()], 4)
    pipe.admit([0])
    tick_until_hold(pipe)
    assert pipe.decide([0], [1], [1], [0]) == [0]
    assert state(pipe, 0, 1) == WFS_FAILED
    pipe.tick()
    assert state(pipe, 0, 2) == WFS_PENDING
    assert pipe.drain_completed() == ([0], [1], [WFS_FAILED])
    assert pipe.hold_stats()["rejected"] == 1 and pipe.hold_stats()["open"] == 0


@pytest.mark.parametrize("T", [1, 3])
def test_a_hold_expires_at_exactly_h_plus_T(T):
    pipe = mk([gate(ttl=T)], 4)
    pipe.admit([0])
    ((_, _, _, h),) = tick_until_hold(pipe)
    assert h == dev_tick(pipe)
    while dev_tick(pipe) < h + T - 1:
        pipe.tick()
        assert state(pipe, 0, 1) == WFS_WAITING
    assert pipe.hold_stats()["expired"] == 0 and pipe.hold_stats()["open"] == 1
    pipe.tick()
    assert dev_tick(pipe) == h + T
    assert state(pipe, 0, 1) == WFS_FAILED
    assert pipe.drain_completed() == ([0], [1], [WFS_FAILED])   # failed in that tick
    assert pipe.hold_stats() == {"opened": 1, "expired": 1, "approved": 0,
                                 "rejected": 0, "open": 0}
    assert pipe.open_holds() == ([], [], [], [])


def test_a_decision_at_the_last_moment_beats_expiry():
    T = 3
    pipe = mk([gate(ttl=T)], 4)
    pipe.admit([0])
    ((_, _, _, h),) = tick_until_hold(pipe)
    while dev_tick(pipe) < h + T - 1:
        pipe.tick()
    assert pipe.decide([0], [1], [1], [1]) == [0]
    pipe.tick()                                                 # tick h + T
    assert dev_tick(pipe) == h + T and state(pipe, 0, 1) == WFS_SUCCEEDED
    assert pipe.drain_completed() == ([0], [1], [WFS_SUCCEEDED])
    assert pipe.hold_stats()["expired"] == 0 and pipe.hold_stats()["approved"] == 1


def test_a_stale_handle_after_slot_reuse_is_refused():
    pipe = mk([gate()], 1)
    assert pipe.admit([0]) == ([0], [1])
    tick_until_hold(pipe)
    assert pipe.cancel([0], [1]) == [1]
    assert pipe.drain_completed() == ([0], [1], [WFS_CANCELLED])
    assert pipe.admit([0]) == ([0], [2])
    holds = tick_until_hold(pipe)
    assert [h[:3] for h in holds] == [(0, 2, 1)]
    before = pipe.step_state.clone()
    assert pipe.decide([0, 0], [1, 3], [1, 1], [1, 0]) == [1, 4]
    assert torch.equal(pipe.step_state, before)                 # the occupant is untouched
    assert pipe.decide([0], [3], [1], [0]) == [1]
    assert state(pipe, 0, 1) == WFS_WAITING
    assert pipe.hold_stats()["approved"] == pipe.hold_stats()["rejected"] == 0
    assert pipe.decide([0], [2], [1], [1]) == [0]


def test_decide_codes_through_the_pipeline():
    pipe = mk([gate()], 3)
    pipe.admit([0, 0])
    tick_until_hold(pipe)
    assert pipe.cancel([1], [1]) == [1]
    #   not waiting (a worker), out of range step, inactive run, free slot,
    #   slot out of range, repeated (slot, step), then the one that applies
    assert pipe.decide([0, 0, 1, 2, 7, 0, 0], [1, 1, 1, 1, 1, 1, 1],
                       [0, 3, 1, 1, 1, 0, 1], [1] * 7) == [3, 3, 2, 1, 1, 4, 0]
    with pytest.raises(ValueError):
        pipe.decide([0], [1], [1], [])
    assert pipe.decide([], [], [], []) == []


def test_a_cancelled_runs_hold_leaves_the_list():
    pipe = mk([gate()], 4)
    pipe.admit([0, 0])
    holds = tick_until_hold(pipe)
    assert [h[0] for h in holds] == [0, 1]
    assert pipe.cancel([0], [1]) == [1]
    assert [h[0] for h in zip(*pipe.open_holds())] == [1]       # before any tick
    pipe.tick()
    assert pipe.hold_stats()["open"] == 1 and int(pipe.hold_mask[0]) == 0
    assert [h[0] for h in zip(*pipe.open_holds())] == [1]


def test_a_slot_readmitted_between_two_ticks_gets_a_fresh_since_tick():
    """cancel + drain + admit between two ticks: no scan sees the slot empty.
    Its hold words still carry the previous occupant's bit and tick; only the
    generation says that they are stale."""
    pipe = mk([DagSpec(steps=[StepSpec(WFK_APPROVAL, ttl_ticks=6)])], 1)
    assert pipe.admit([0]) == ([0], [1])
    assert tick_until_hold(pipe) == [(0, 1, 0, 0)]
    for _ in range(3):
        pipe.tick()
    assert pipe.cancel([0], [1]) == [1]
    assert pipe.drain_completed()[0] == [0]
    assert pipe.admit([0]) == ([0], [2])
    assert int(pipe.hold_mask[0]) == 1 and int(pipe.hold_gen[0]) == 1   # stale words
    assert pipe.open_holds() == ([], [], [], [])
    pipe.tick()                                                 # device tick 4
    assert list(zip(*pipe.open_holds())) == [(0, 2, 0, 4)]
    pipe.tick()
    pipe.tick()                                                 # tick 6 = 0 + ttl
    assert state(pipe, 0, 0) == WFS_WAITING                     # not the old hold's expiry
    assert pipe.hold_stats()["expired"] == 0 and pipe.hold_stats()["opened"] == 2
    for _ in range(4):
        pipe.tick()                                             # tick 10 = 4 + ttl
    assert state(pipe, 0, 0) == WFS_FAILED and pipe.hold_stats()["expired"] == 1


def test_two_approval_steps_of_one_run_are_independent():
    dag = DagSpec(steps=[StepSpec(WFK_APPROVAL), StepSpec(WFK_APPROVAL),
                         StepSpec(WFK_WORKER, deps=[0, 1])])
    pipe = mk([dag], 2)
    pipe.admit([0])
    holds = tick_until_hold(pipe)
    assert [h[:3] for h in holds] == [(0, 1, 0), (0, 1, 1)]
    assert pipe.decide([0], [1], [1], [1]) == [0]
    pipe.tick()
    assert [h[:3] for h in zip(*pipe.open_holds())] == [(0, 1, 0)]
    assert state(pipe, 0, 2) == WFS_PENDING and int(pipe.run_active[0]) == 1
    assert pipe.decide([0, 0], [1, 1], [0, 1], [1, 1]) == [0, 3]   # 1 is decided already
    pipe.tick()
    assert pipe.drain_completed() == ([0], [1], [WFS_SUCCEEDED])
    assert pipe.hold_stats()["approved"] == 2


def test_more_holds_than_hold_cap_page_completely():
    dag = DagSpec(steps=[StepSpec(WFK_APPROVAL), StepSpec(WFK_APPROVAL)])
    pipe = mk([dag], 12, hold_cap=3)
    pipe.admit([0] * 10)
    pipe.tick()
    slots, gens, steps, since = pipe.open_holds()
    assert list(zip(slots, steps)) == [(r, s) for r in range(10) for s in (0, 1)]
    assert gens == [1] * 20 and since == [0] * 20
    assert pipe.hold_stats()["open"] == 20
    assert mk([dag], 12).hold_cap == 64 * 12    # the default page: the whole table


def test_events_chain_with_the_journal_on():
    from tests.test_wf_events import Replay

    pipe = mk([gate(), gate(ttl=2)], 4, event_cap=4096)
    pipe.admit([0, 0, 1])
    replay = Replay()
    holds = tick_until_hold(pipe)
    assert [h[:3] for h in holds] == [(0, 1, 1), (1, 1, 1), (2, 1, 1)]
    k = dev_tick(pipe)
    assert pipe.decide([0, 1], [1, 1], [1, 1], [1, 0]) == [0, 0]
    events = pipe.drain_events()
    replay.apply(events)
    assert not any(t in (WFS_SUCCEEDED, WFS_FAILED) and st == 1
                   for st, t in zip(events[2], events[4]))      # decide journals nothing
    pipe.tick()
    pipe.tick()                                                 # run 2's hold expires
    events = pipe.drain_events()
    replay.apply(events)
    replay.assert_is(pipe)
    rows = [e for e in zip(*events) if e[2] == 1]
    # decided between tick k and k+1: detected by the pass that ends tick k+1
    assert (0, 1, 1, WFS_WAITING, WFS_SUCCEEDED, 2 * (k + 1)) in rows
    assert (1, 1, 1, WFS_WAITING, WFS_FAILED, 2 * (k + 1)) in rows
    assert (2, 1, 1, WFS_WAITING, WFS_FAILED, 2 * (k + 2)) in rows   # h + ttl, phase 0


def test_device_run_table_serves_approvals_by_run_and_step_id():
    wf = {"id": "wf-gate", "steps": {
        "build": {"type": "worker", "topic": "job.x"},
        "sign-off": {"type": "approval", "depends_on": ["build"]},
        "ship": {"type": "worker", "topic": "job.x", "depends_on": ["sign-off"]}}}
    pipe = mk([], 2, event_cap=1024)
    table = DeviceRunTable(pipe)
    t_plain = table.register(wf)
    t_ttl = table.register(wf, tick_seconds=2.0, approval_ttl_sec=5.0)   # 3 ticks
    assert pipe.tmpl_ttl[t_ttl * 64:t_ttl * 64 + 3].tolist() == [0, 3, 0]
    assert not bool(pipe.tmpl_ttl[t_plain * 64:t_plain * 64 + 64].any())
    assert table.submit("a", t_plain) and table.submit("b", t_ttl)
    assert not table.submit("c", t_plain)                       # queued
    assert table.approvals() == []
    with pytest.raises(ValueError, match="step not waiting"):
        table.approve("a", "sign-off")                          # still pending
    for _ in range(5):
        table.tick()
        if table.approvals():
            break
    h = dev_tick(pipe)
    assert table.approvals() == [PendingApproval("a", 1, "sign-off", h, None),
                                 PendingApproval("b", 1, "sign-off", h, h + 3)]
    with pytest.raises(KeyError):
        table.approve("nobody", "sign-off")
    with pytest.raises(ValueError, match="step not found"):
        table.approve("a", "no-such-step")
    with pytest.raises(ValueError, match="step not found"):
        table.reject("a", 3)
    with pytest.raises(ValueError, match="step not waiting"):
        table.approve("a", "build")
    with pytest.raises(ValueError, match="step not waiting"):
        table.approve("c", "sign-off")                          # queued
    with pytest.raises(ValueError, match="step not found"):
        table.approve("c", "nope")
    table.approve("a", "sign-off")
    with pytest.raises(ValueError, match="step not waiting"):
        table.approve("a", 1)                                   # decided already
    table.reject("b", 1)
    assert table.approvals() == []
    table.tick()
    assert sorted(table.poll()) == [("a", "succeeded"), ("b", "failed")]
    from cordum_amd.workflow.device_runs import timeline_of

    names = {(e.run_id, timeline_of(WFK_APPROVAL, e.to_state)[0])
             for e in table.take_events() if e.step == 1}
    assert names == {("a", "step_waiting"), ("a", "step_approved"),
                     ("b", "step_waiting"), ("b", "step_rejected")}
    # c was admitted by the poll; its hold expires nowhere (plain template)
    for _ in range(3):
        table.tick()
    assert [a[:3] for a in table.approvals()] == [("c", 1, "sign-off")]
    with pytest.raises(KeyError):
        table.approve("a", "sign-off")                          # reported and gone


def test_device_run_table_needs_external_approvals_to_decide():
    pipe = mk([gate()], 2, approvals="auto")
    table = DeviceRunTable(pipe)
    table.submit("a", 0)
    with pytest.raises(RuntimeError):
        table.approvals()
    with pytest.raises(RuntimeError):
        table.approve("a", 1)


def run_to_the_end(pipe, n_dags, approve):
    slots, gens = pipe.admit(list(range(n_dags)))
    assert slots == list(range(n_dags))
    for _ in range(80):
        pipe.tick()
        if approve:
            s, g, st, _ = pipe.open_holds()
            assert pipe.decide(s, g, st, [1] * len(s)) == [0] * len(s)
        if pipe.active() == 0:
            break
    assert pipe.active() == 0
    return pipe.run_state[:n_dags].clone()


def test_approving_everything_every_tick_ends_where_auto_mode_ends():
    dags = random_dags()
    assert any(s.kind == WFK_APPROVAL for d in dags for s in d.steps)
    auto = run_to_the_end(mk(dags, 16, approvals="auto", approval_verdict=1, **AMPLE),
                          len(dags), approve=False)
    ext = mk(dags, 16, **AMPLE)
    got = run_to_the_end(ext, len(dags), approve=True)
    assert torch.equal(got, auto)
    stats = ext.hold_stats()
    assert stats["opened"] == stats["approved"] > 0 and stats["open"] == 0


class Counting(_RefOps):
    """_RefOps that counts the kernels launched through it."""

    def __init__(self):
        super().__init__()
        self.calls = {}

    def __getattribute__(self, name):
        attr = super().__getattribute__(name)
        if not name.startswith("_") and name != "calls" and callable(attr):
            self.calls[name] = self.calls.get(name, 0) + 1
        return attr


def drive(pipe):
    pipe.ext = Counting()
    pipe.admit([0, 0])
    for _ in range(6):
        pipe.tick()
        pipe.drain_completed()
    return pipe.ext.calls


def test_auto_mode_launches_no_new_kernel_and_allocates_no_table():
    auto = mk([gate()], 4, approvals="auto")
    calls = drive(auto)
    assert not NEW_KERNELS & set(calls) and calls["wf_grant"] >= 1
    assert calls["wf_sweep"] == 6
    for name in ("hold_mask", "hold_tick", "hold_ttl", "hold_gen", "hold_counts",
                 "hold_open", "tmpl_ttl"):
        assert not hasattr(auto, name), name
    assert auto.active() == 0                                   # auto-granted as before
    ext = mk([gate()], 4)
    calls = drive(ext)
    assert calls["wf_hold_scan"] == calls["wf_sweep"] == 6
    assert "wf_grant" not in calls and ext.active() == 2        # nobody decided


def test_external_approvals_are_refused_where_they_cannot_work():
    with pytest.raises(ValueError):
        WorkflowPipeline(device="cpu", dags=[gate()], backend="ref",
                         n_local_workers=16, payload_words=4, approvals="external")
    with pytest.raises(ValueError):
        mk([gate()], 4, approvals="sometimes")
    with pytest.raises(ValueError):
        mk([gate()], 4, approvals="auto", hold_cap=8)
    with pytest.raises(ValueError):
        mk([gate(ttl=2)], 4, approvals="auto")                  # a ttl nobody enforces
    with pytest.raises(ValueError):
        mk([DagSpec(steps=[StepSpec(WFK_WORKER, ttl_ticks=2)])], 4)
    auto = mk([gate()], 4, approvals="auto")
    static = WorkflowPipeline(device="cpu", dags=[gate()], backend="ref",
                              n_local_workers=16, payload_words=4)
    for pipe in (auto, static):
        for call in (pipe.open_holds, pipe.hold_stats,
                     lambda: pipe.decide([0], [1], [1], [1])):
            with pytest.raises(RuntimeError):
                call()


def test_hold_ttl_follows_the_template_into_a_reused_slot():
    pipe = mk([gate(ttl=5), gate()], 2)
    assert pipe.admit([0, 1]) == ([0, 1], [1, 1])
    assert pipe.hold_ttl.view(2, 64)[:, :3].tolist() == [[0, 5, 0], [0, 0, 0]]
    pipe.cancel([0], [1])
    pipe.drain_completed()
    assert pipe.admit([1, 0]) == ([0, -1], [2, 0])              # the full one is skipped
    assert pipe.hold_ttl.view(2, 64)[:, :3].tolist() == [[0, 0, 0], [0, 0, 0]]
