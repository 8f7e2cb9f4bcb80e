"""Conditions decided on the device (`device_conditions=True`), pipeline
level, on the CPU backend: branching on step outputs, the run's input and
output rows over a slot's life, the validation of predicates, the tick's
launch sequence and the interplay with the other dynamic-mode options. All
tables are small (NR <= 8).

A child's payload is (input words, ordinal, step, zeros) and the echo worker
answers with the wraparound sum of the payload, so a child's result is
sum(input words) + ordinal + step, and a step's output the sum of that over
the children that succeeded. The expected outputs below are worked out from
that by hand.
"""
import pytest
import torch

from cordum_amd.ops.reference import wf_fail_hash
from cordum_amd.ops.wf_pipeline import (
    CondSpec,
    DagSpec,
    RetrySpec,
    StepSpec,
    WFC_GT,
    WFK_APPROVAL,
    WFK_CONDITION,
    WFK_DELAY,
    WFK_FOR_EACH,
    WFK_WORKER,
    WFS_PENDING,
    WFS_SKIPPED,
    WFS_SUCCEEDED,
    WorkflowPipeline,
)
from cordum_amd.workflow.device_runs import DeviceRunTable

IW = 8


def _pipe(dags, NR=4, **kw):
    kw.setdefault("device_conditions", True)
    kw.setdefault("payload_words", 10)
    return WorkflowPipeline("cpu", dags, n_local_workers=4, backend="ref",
                            dynamic_capacity=NR, child_cap=64, **kw)


def _branch_dag():
    """worker -> condition(out0 > 1000) -> for_each x3 if true / worker if false"""
    return DagSpec(steps=[
        StepSpec(WFK_WORKER),
        StepSpec(WFK_CONDITION, deps=[0], when=CondSpec(WFC_GT, ("out", 0), 1000)),
        StepSpec(WFK_FOR_EACH, deps=[1], fanout=3, when=CondSpec("truthy", ("out", 1))),
        StepSpec(WFK_WORKER, deps=[1], when=CondSpec("==", ("out", 1), 0)),
    ])


def _run(pipe, ticks=12):
    for _ in range(ticks):
        pipe.tick()


def _states(pipe, slot, n):
    return pipe.step_state[slot * 64:slot * 64 + n].tolist()


def _outs(pipe, slot, n):
    return pipe.step_out[slot * 64:slot * 64 + n].tolist()


def test_two_neighbouring_runs_of_one_template_branch_on_their_worker_output():
    pipe = _pipe([_branch_dag()])
    slots, _ = pipe.admit([0, 0], inputs=[[600, 500], [5, 6]])
    assert slots == [0, 1]
    _run(pipe)
    # run 0: out0 = 1100 + ordinal 0 + step 0 > 1000: the for_each runs, three
    # children of 1100 + k + 2 each; the worker on the false side is skipped
    assert _states(pipe, 0, 4) == [WFS_SUCCEEDED, WFS_SUCCEEDED, WFS_SUCCEEDED, WFS_SKIPPED]
    assert _outs(pipe, 0, 4) == [1100, 1, (1102 + 1103 + 1104), 0]
    # run 1: out0 = 11: the condition is false (SKIPPED), the for_each is
    # skipped, the worker runs: 11 + ordinal 0 + step 3
    assert _states(pipe, 1, 4) == [WFS_SUCCEEDED, WFS_SKIPPED, WFS_SKIPPED, WFS_SUCCEEDED]
    assert _outs(pipe, 1, 4) == [11, 0, 0, 14]
    assert pipe.children_emitted[:4].tolist() == [1, 0, 3, 0]
    assert pipe.children_emitted[64:68].tolist() == [1, 0, 0, 1]
    assert pipe.counts() == (2, 0)
    # 3 predicates per run; run 0: true, true, false; run 1: false, false, true
    assert pipe.cond_stats() == {"true": 3, "false": 3}


def test_the_run_table_reports_the_outputs_by_step_id():
    wf = {"id": "wf", "steps": {
        "a": {"type": "worker", "topic": "job.x"},
        "c": {"type": "condition", "condition": "steps.a.output > 1000",
              "depends_on": ["a"]},
        "hi": {"type": "worker", "topic": "job.x", "depends_on": ["c"],
               "condition": "steps.c.output"},
        "lo": {"type": "worker", "topic": "job.x", "depends_on": ["c"],
               "condition": "!steps.c.output"},
    }}
    pipe = _pipe([])
    tab = DeviceRunTable(pipe)
    t = tab.register(wf)
    assert t == 0
    assert tab.submit("big", t, input={"unused": "x"})
    _run(pipe)
    # no input field is named, so every word is 0: a = 0 + 0 + 0, not > 1000
    assert tab.step_outputs("big") == {"a": 0, "c": 0, "hi": 0, "lo": 3}


def test_a_retried_child_contributes_its_fresh_ordinal_exactly_once():
    # the failure hash is a function of (tag, ordinal): find a slot whose
    # first child (ordinal 0) fails at a rate its second (ordinal 1) survives
    NR = 8
    pick = [(wf_fail_hash(s * 64, 0) % 1000, s) for s in range(NR)
            if wf_fail_hash(s * 64, 0) % 1000 < wf_fail_hash(s * 64, 1) % 1000]
    assert pick, "no slot of the eight fails ordinal 0 and passes ordinal 1"
    h0, slot = min(pick)
    pipe = _pipe([DagSpec(steps=[StepSpec(WFK_WORKER)])], NR=NR, fail_ppt=h0 + 1)
    slots, _ = pipe.admit([0] * NR, inputs=[[100, 20, 3]] * NR)
    assert slots == list(range(NR))
    _run(pipe, 16)
    i = slot * 64
    assert int(pipe.step_state[i]) == WFS_SUCCEEDED
    assert int(pipe.step_attempts[i]) == 1 and int(pipe.children_emitted[i]) == 2
    # the failed child (ordinal 0) added nothing; the retry is 123 + 1 + 0
    assert int(pipe.step_out[i]) == 124


def test_a_reused_slot_starts_with_zero_outputs_and_the_new_inputs():
    pipe = _pipe([DagSpec(steps=[StepSpec(WFK_WORKER)])], NR=1)
    assert pipe.admit([0], inputs=[[7, 8, 9]])[0] == [0]
    _run(pipe, 4)
    assert _outs(pipe, 0, 1) == [24]
    assert pipe.drain_completed()[0] == [0]
    assert pipe.admit([0], inputs=[[-5]])[0] == [0]
    assert pipe.step_out.tolist() == [0] * 64
    assert pipe.run_input.tolist() == [-5] + [0] * (IW - 1)
    _run(pipe, 4)
    assert _outs(pipe, 0, 1) == [-5]


def test_a_refused_admission_writes_no_row():
    pipe = _pipe([DagSpec(steps=[StepSpec(WFK_WORKER)]),
                  DagSpec(steps=[StepSpec(WFK_WORKER), StepSpec(WFK_WORKER)])], NR=2)
    assert pipe.admit([0, 0], inputs=[[1, 2], [3]])[0] == [0, 1]
    _run(pipe, 3)
    before = (pipe.run_input.clone(), pipe.step_out.clone(), pipe.run_tmpl.clone())
    assert before[1].view(2, 64)[:, 0].tolist() == [3, 3]
    assert pipe.admit([1, 1], inputs=[[50], [60]])[0] == [-1, -1]
    assert torch.equal(pipe.run_input, before[0])
    assert torch.equal(pipe.step_out, before[1])
    assert torch.equal(pipe.run_tmpl, before[2])


def test_a_condition_without_a_predicate_keeps_its_admitted_bit():
    dag = DagSpec(steps=[
        StepSpec(WFK_CONDITION),
        StepSpec(WFK_CONDITION, when=CondSpec("<", ("input", 0), 0)),
        StepSpec(WFK_WORKER, deps=[0], when=CondSpec("truthy", ("out", 0))),
    ])
    pipe = _pipe([dag])
    pipe.admit([0, 0], cond_bits=[0b01, 0b10], inputs=[[5], [5]])
    _run(pipe, 5)
    # step 1's predicate is false whatever its admitted bit says; step 0
    # follows the admitted bit, and its output word is that bit
    assert _states(pipe, 0, 3) == [WFS_SUCCEEDED, WFS_SKIPPED, WFS_SUCCEEDED]
    assert _states(pipe, 1, 3) == [WFS_SKIPPED, WFS_SKIPPED, WFS_SKIPPED]
    assert _outs(pipe, 0, 3) == [1, 0, 5 + 0 + 2]
    assert _outs(pipe, 1, 3) == [0, 0, 0]


def test_a_guard_behind_a_guarded_off_step_is_decided_before_the_sweep_sees_it():
    """Step 1 is skipped by its guard, which satisfies step 2's deps in the
    same tick; step 2's own guard is false too and must be looked at before
    the sweep could dispatch it."""
    dag = DagSpec(steps=[
        StepSpec(WFK_WORKER),
        StepSpec(WFK_WORKER, deps=[0], when=CondSpec("!=", ("input", 0), 9)),
        StepSpec(WFK_WORKER, deps=[1], when=CondSpec("<", ("out", 0), 0)),
        StepSpec(WFK_WORKER, deps=[2]),
    ])
    pipe = _pipe([dag])
    pipe.admit([0], inputs=[[9]])
    _run(pipe, 6)
    assert _states(pipe, 0, 4) == [WFS_SUCCEEDED, WFS_SKIPPED, WFS_SKIPPED, WFS_SUCCEEDED]
    assert pipe.children_emitted[:4].tolist() == [1, 0, 0, 1]


# ---- validation ---------------------------------------------------------------
def test_the_option_needs_dynamic_mode_and_room_in_the_payload():
    dag = DagSpec(steps=[StepSpec(WFK_WORKER)])
    with pytest.raises(ValueError, match="dynamic_capacity"):
        WorkflowPipeline("cpu", [dag], backend="ref", device_conditions=True)
    for iw in (0, 33):
        with pytest.raises(ValueError, match="input_words"):
            _pipe([dag], input_words=iw, payload_words=64)
    with pytest.raises(ValueError, match="payload_words"):
        _pipe([dag], input_words=8, payload_words=9)
    _pipe([dag], input_words=8, payload_words=10)
    _pipe([dag], input_words=32, payload_words=34)


@pytest.mark.parametrize("steps,match", [
    # an input index past input_words
    ([StepSpec(WFK_WORKER, when=CondSpec("==", ("input", IW), 0))], "input word"),
    # immediates outside int32
    ([StepSpec(WFK_WORKER, when=CondSpec("==", ("input", 0), 1 << 31))], "int32"),
    ([StepSpec(WFK_WORKER, when=CondSpec("==", ("input", 0), -(1 << 31) - 1))], "int32"),
    # an output that is not among the transitive dependencies: a later step,
    # the step itself, an unrelated earlier step
    ([StepSpec(WFK_WORKER, when=CondSpec("==", ("out", 1), 0)), StepSpec(WFK_WORKER)],
     "dependencies"),
    ([StepSpec(WFK_WORKER, when=CondSpec("==", ("out", 0), 0))], "dependencies"),
    ([StepSpec(WFK_WORKER), StepSpec(WFK_WORKER),
      StepSpec(WFK_WORKER, deps=[1], when=CondSpec("==", ("input", 0), ("out", 0)))],
     "dependencies"),
    # an output of a step that has none
    ([StepSpec(WFK_DELAY), StepSpec(WFK_WORKER, deps=[0],
                                    when=CondSpec("truthy", ("out", 0)))], "no output"),
    ([StepSpec(WFK_APPROVAL), StepSpec(WFK_WORKER, deps=[0],
                                       when=CondSpec("==", ("input", 0), ("out", 0)))],
     "no output"),
])
def test_add_template_refuses(steps, match):
    pipe = _pipe([])
    with pytest.raises(ValueError, match=match):
        pipe.add_template(DagSpec(steps=steps))
    assert pipe.n_templates == 0


def test_a_transitive_dependency_is_accepted():
    pipe = _pipe([])
    pipe.add_template(DagSpec(steps=[
        StepSpec(WFK_WORKER), StepSpec(WFK_DELAY, deps=[0]),
        StepSpec(WFK_WORKER, deps=[1], when=CondSpec(">=", ("out", 0), ("input", IW - 1)))]))


def test_when_needs_the_option():
    dag = DagSpec(steps=[StepSpec(WFK_WORKER, when=CondSpec("truthy", ("input", 0)))])
    with pytest.raises(ValueError, match="device_conditions"):
        _pipe([dag], device_conditions=False)
    pipe = _pipe([], device_conditions=False)
    with pytest.raises(ValueError, match="device_conditions"):
        pipe.add_template(dag)
    with pytest.raises(ValueError, match="device_conditions"):
        WorkflowPipeline("cpu", [dag], backend="ref")
    pipe.add_template(DagSpec(steps=[StepSpec(WFK_WORKER)]))
    with pytest.raises(ValueError, match="device_conditions"):
        pipe.admit([0], inputs=[[1]])


def test_admit_refuses_bad_inputs():
    pipe = _pipe([DagSpec(steps=[StepSpec(WFK_WORKER)])])
    for bad in ([[1] * (IW + 1)], [[1 << 31]], [[True]], [[1.5]], [[1], [2]]):
        with pytest.raises(ValueError):
            pipe.admit([0], inputs=bad)
    assert int(pipe.run_life.sum()) == 0


# ---- launch sequence -------------------------------------------------------------
class _Recorder:
    def __init__(self, ext):
        self._ext, self.calls = ext, []

    def __getattr__(self, name):
        fn = getattr(self._ext, name)

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


# what one tick of a dynamic-mode pipeline launches without the option
PARENT_TICK = [
    "wf_sweep", "wf_expand", "worker_precompute_into", "pack_requeue", "pack_by_dest",
    "gather_payload_padded", "materialize_rq_payload", "materialize_rq_payload",
    "materialize_rq_payload", "echo_padded", "load_feedback_padded", "wf_apply",
    "wf_apply_dead", "wf_timeout_scan", "wf_commit", "wf_status"]


def test_with_the_option_off_the_tick_is_the_parents_and_nothing_is_allocated():
    pipe = _pipe([DagSpec(steps=[StepSpec(WFK_WORKER)])], device_conditions=False)
    pipe.ext = rec = _Recorder(pipe.ext)
    pipe.admit([0])
    pipe.tick()
    pipe.tick()
    assert rec.calls == ["wf_admit"] + PARENT_TICK * 2
    for name in ("run_input", "step_out", "run_tmpl", "tmpl_cond", "tmpl_cond_mask",
                 "cond_counts", "input_words", "_run_input_buf", "_step_out_buf",
                 "_run_tmpl_buf"):
        assert not hasattr(pipe, name), name
    with pytest.raises(RuntimeError):
        pipe.cond_stats()


def test_with_the_option_on_the_tick_launches_the_three_kernels_and_never_wf_apply():
    pipe = _pipe([_branch_dag()])
    pipe.ext = rec = _Recorder(pipe.ext)
    pipe.admit([0], inputs=[[1]])
    pipe.tick()
    pipe.tick()
    want = list(PARENT_TICK)
    want[want.index("wf_apply")] = "wf_apply_out"
    want.insert(want.index("wf_expand") + 1, "wf_child_payload")
    want.insert(0, "wf_cond_eval")
    assert rec.calls == ["wf_admit"] + want * 2
    assert "wf_apply" not in rec.calls


# ---- interplay with the other options ----------------------------------------------
def _gated_approval_dag():
    return DagSpec(steps=[
        StepSpec(WFK_WORKER),
        StepSpec(WFK_APPROVAL, deps=[0], when=CondSpec(">", ("out", 0), 1000)),
        StepSpec(WFK_WORKER, deps=[1]),
    ])


def test_a_guarded_off_approval_never_opens_a_hold():
    pipe = _pipe([_gated_approval_dag()], approvals="external")
    pipe.admit([0, 0], inputs=[[5], [5000]])
    _run(pipe, 6)
    # run 0: out0 = 5, the approval is skipped and the run finishes; run 1:
    # out0 = 5000, the approval waits for a decision
    assert _states(pipe, 0, 3) == [WFS_SUCCEEDED, WFS_SKIPPED, WFS_SUCCEEDED]
    slots, gens, steps, _ = pipe.open_holds()
    assert (slots, steps) == ([1], [1])
    assert pipe.hold_stats()["opened"] == 1
    assert pipe.decide(slots, gens, steps, [1]) == [0]
    _run(pipe, 4)
    assert pipe.counts() == (2, 0)
    assert pipe.hold_stats() == {"opened": 1, "expired": 0, "approved": 1,
                                 "rejected": 0, "open": 0}


def test_the_journal_records_the_skip_exactly_once():
    pipe = _pipe([_gated_approval_dag()], event_cap=256)
    pipe.admit([0], inputs=[[5]])
    ev = []
    for _ in range(6):
        pipe.tick()
        ev += list(zip(*pipe.drain_events()))
    skips = [e for e in ev if e[2] == 1]
    assert [(e[3], e[4]) for e in skips] == [(WFS_PENDING, WFS_SKIPPED)]
    assert not any(e[2] == 1 and e[4] not in (WFS_SKIPPED,) for e in ev)


def test_step_policy_and_conditions_share_one_run_tmpl():
    dags = [DagSpec(steps=[StepSpec(WFK_WORKER)]),
            DagSpec(steps=[
                StepSpec(WFK_WORKER, retry=RetrySpec(max_retries=1)),
                StepSpec(WFK_WORKER, deps=[0], when=CondSpec("<", ("out", 0), 0))])]
    pipe = _pipe(dags, step_policy=True)
    pipe.ext = rec = _Recorder(pipe.ext)
    assert pipe.admit([1, 0, 1], inputs=[[3], [], [-9]])[0] == [0, 1, 2]
    assert pipe.run_tmpl.tolist()[:3] == [1, 0, 1]
    assert pipe._run_tmpl_buf.numel() == pipe.NR + 1
    _run(pipe, 5)
    assert "wf_settle" in rec.calls and "wf_cond_eval" in rec.calls
    assert "wf_commit" not in rec.calls and "wf_apply" not in rec.calls
    assert _states(pipe, 0, 2) == [WFS_SUCCEEDED, WFS_SKIPPED]
    assert _states(pipe, 2, 2) == [WFS_SUCCEEDED, WFS_SUCCEEDED]
    assert _outs(pipe, 2, 2) == [-9, -9 + 1]
    assert pipe.counts() == (3, 0)
