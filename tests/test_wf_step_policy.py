"""Per-step retry, backoff and timeout policy of the device workflow engine
(`step_policy=True`), on the CPU reference backend: the public interface, the
tick's launch sequence, the lowering of a `Workflow`'s `retry` blocks and
`timeout_sec`, and the run table on top. All tables are small (NR <= 65).

The echo workers answer within the tick, so with every child failing
(`fail_ppt=1000`) a step is dispatched, fails and is settled in one tick: its
dispatch ticks are the whole schedule. A dispatch is a tick in which the
step's `children_emitted` grew; `dispatch_tick` then holds that tick.
"""
import random

import pytest
import torch

from cordum_amd.ops.wf_pipeline import (
    DagSpec, RetrySpec, StepSpec, WFK_APPROVAL, WFK_CONDITION, WFK_DELAY, WFK_FOR_EACH,
    WFK_WORKER, WFS_DISPATCHED, WFS_FAILED, WFS_PENDING, WorkflowPipeline)
from tests.test_gpu_wf_dynamic import COUNTERS, TABLES, churn_dags

T0 = 3          # runs are admitted after this many empty ticks


def _pipe(dags, capacity=4, **kw):
    kw.setdefault("step_policy", True)
    return WorkflowPipeline(device="cpu", dags=dags, backend="ref", n_local_workers=16,
                            payload_words=4, dynamic_capacity=capacity, **kw)


def _worker(**kw):
    return StepSpec(WFK_WORKER, **kw)


def _admit_at_t0(pipe, templates):
    for _ in range(T0):
        pipe.tick()
    slots, _ = pipe.admit(templates)
    assert -1 not in slots and not bool(pipe.children_emitted.any())
    return slots


def _dispatches(pipe, cells, ticks):
    """Tick `ticks` times; returns per cell (slot, step) the ticks at which it
    was dispatched, and per tick the pipeline's tick number."""
    seen = {c: [] for c in cells}
    for _ in range(ticks):
        before = pipe.children_emitted.clone()
        pipe.tick()
        for (r, s), hist in seen.items():
            if int(pipe.children_emitted[r * 64 + s]) > int(before[r * 64 + s]):
                assert int(pipe.dispatch_tick[r * 64 + s]) == int(pipe.tick_buf[0])
                hist.append(int(pipe.tick_buf[0]))
    return seen


# 1 ---------------------------------------------------------------------------
def test_a_step_with_no_retries_fails_at_once_on_a_retrying_pipeline():
    pipe = _pipe([DagSpec(steps=[_worker(retry=RetrySpec(max_retries=0))])],
                 max_retries=2, fail_ppt=1000)
    (slot,) = _admit_at_t0(pipe, [0])
    pipe.tick()
    assert int(pipe.run_state[slot]) == WFS_FAILED and int(pipe.run_active[slot]) == 0
    assert int(pipe.step_state[slot * 64]) == WFS_FAILED
    assert int(pipe.step_attempts[slot * 64]) == 0
    assert int(pipe.retry_count[0]) == 0
    assert pipe.counts() == (0, 1)


def test_an_unannotated_step_on_the_same_pipeline_still_retries_twice():
    pipe = _pipe([DagSpec(steps=[_worker()])], max_retries=2, fail_ppt=1000)
    (slot,) = _admit_at_t0(pipe, [0])
    seen = _dispatches(pipe, [(slot, 0)], 8)
    assert seen[(slot, 0)] == [T0, T0 + 2, T0 + 6]          # the stock 2, 4
    assert int(pipe.step_attempts[slot * 64]) == 2 and int(pipe.retry_count[0]) == 2
    assert int(pipe.run_state[slot]) == WFS_FAILED


# 2 ---------------------------------------------------------------------------
def test_backoff_schedule_of_a_step():
    """(3 ticks, x1.5, cap 10) waits 3, 5, 7, 10."""
    spec = RetrySpec(4, backoff_ticks=3, multiplier_q8=384, cap_ticks=10)
    pipe = _pipe([DagSpec(steps=[_worker(retry=spec)])], fail_ppt=1000)
    (slot,) = _admit_at_t0(pipe, [0])
    seen, failed_at = [], []
    for _ in range(27):
        seen += _dispatches(pipe, [(slot, 0)], 1)[(slot, 0)]
        if int(pipe.run_state[slot]) == WFS_FAILED:
            failed_at.append(int(pipe.tick_buf[0]))
    assert seen == [T0, T0 + 3, T0 + 8, T0 + 15, T0 + 25]
    assert failed_at[0] == T0 + 25
    assert int(pipe.step_attempts[slot * 64]) == 4 and int(pipe.retry_count[0]) == 4


# 3 ---------------------------------------------------------------------------
def test_each_step_follows_its_own_policy_in_one_table():
    """Two policies in one run, and a second template with two others (one of
    them the pipeline's own), side by side in one table."""
    a = DagSpec(steps=[_worker(retry=RetrySpec(3, 4, 256, 0)),
                       _worker(retry=RetrySpec(5, 1, 512, 4))])
    b = DagSpec(steps=[_worker(retry=RetrySpec(1, 6, 256, 0)), _worker()])
    pipe = _pipe([a, b], max_retries=3, fail_ppt=1000)
    ra, rb = _admit_at_t0(pipe, [0, 1])
    assert pipe.run_tmpl.tolist()[:2] == [0, 1]
    seen = _dispatches(pipe, [(ra, 0), (ra, 1), (rb, 0), (rb, 1)], 14)
    # run a fails with its step 0 at T0 + 12, run b with its step 0 at T0 + 6;
    # until then each step kept its own schedule
    assert seen[(ra, 0)] == [T0, T0 + 4, T0 + 8, T0 + 12]            # 4, 4, 4
    assert seen[(ra, 1)] == [T0, T0 + 1, T0 + 3, T0 + 7, T0 + 11]    # 1, 2, 4, 4
    assert seen[(rb, 0)] == [T0, T0 + 6]
    assert seen[(rb, 1)] == [T0, T0 + 2, T0 + 6]                     # stock 2, 4
    assert int(pipe.step_state[ra * 64]) == WFS_FAILED
    assert int(pipe.step_state[rb * 64]) == WFS_FAILED
    # one retry per failed dispatch but the last of an exhausted step
    assert pipe.step_attempts.view(-1, 64)[[ra, rb], :2].tolist() == [[3, 5], [1, 3]]


def test_run_tmpl_names_the_occupant_and_a_refused_request_writes_no_row():
    one = DagSpec(steps=[_worker()])
    pipe = _pipe([one, one, one], capacity=3)
    assert pipe.admit([2, 1]) == ([0, 1], [1, 1])
    assert pipe.run_tmpl.tolist() == [2, 1, 0]
    slots, _ = pipe.admit([1, 2, 2])                 # one slot left: two are refused
    assert slots == [2, -1, -1]
    assert pipe.run_tmpl.tolist() == [2, 1, 1] and pipe.run_tmpl.numel() == pipe.NR
    for _ in range(2):
        pipe.tick()
    assert pipe.drain_completed()[0] == [0, 1, 2]
    assert pipe.admit([0])[0] == [0]                 # the slot changes hands
    assert pipe.run_tmpl.tolist() == [0, 1, 1]


# 4 ---------------------------------------------------------------------------
def _churn(step_policy):
    dags = churn_dags()
    pipe = _pipe(dags, capacity=24, step_policy=step_policy, fail_ppt=300,
                 drop_ppt=100, max_retries=2)
    rng = random.Random(5)
    snaps = []
    for tick in range(40):
        pipe.drain_completed()
        n = 30 if tick == 0 else rng.randint(1, 6)
        got = pipe.admit([rng.randrange(len(dags)) for _ in range(n)],
                         fanout=[rng.choice([0, 3]) for _ in range(n)])
        if tick == 9:
            assert pipe.cancel([5], [int(pipe.run_gen[5])]) == [1]
        pipe.tick()
        snaps.append((got, {k: getattr(pipe, k).clone() for k in TABLES + COUNTERS}))
    return snaps


def test_default_policies_compute_what_the_pipeline_computes_without_the_option():
    on, off = _churn(True), _churn(False)
    for tick, ((got_on, s_on), (got_off, s_off)) in enumerate(zip(on, off)):
        assert got_on == got_off, tick
        for k in TABLES + COUNTERS:
            assert torch.equal(s_on[k], s_off[k]), (tick, k)
    last = off[-1][1]
    assert int(last["retry_count"][0]) > 0 and int(last["timeout_count"][0]) > 0
    assert int(last["cancel_count"][0]) == 1
    assert min(last["wf_counts"].tolist()) > 0          # runs succeeded and runs failed


# 5 ---------------------------------------------------------------------------
def test_a_longer_step_timeout_is_waited_out():
    dag = DagSpec(steps=[_worker(timeout_ticks=12), _worker()])
    pipe = _pipe([dag], drop_ppt=1000, timeout_cutoff=8)
    (slot,) = _admit_at_t0(pipe, [0])
    lost = {}
    for _ in range(14):
        pipe.tick()
        lost[int(pipe.tick_buf[0])] = int(pipe.timeout_count[0])
    assert pipe.dispatch_tick[slot * 64:slot * 64 + 2].tolist()[0] == T0
    assert all(lost[t] == 0 for t in range(T0, T0 + 8))
    assert all(lost[t] == 1 for t in range(T0 + 8, T0 + 12))     # step 1: the cutoff
    assert lost[T0 + 12] == lost[T0 + 13] == 2                   # step 0: its own 12
    assert pipe.step_attempts[slot * 64:slot * 64 + 2].tolist() == [1, 1]


# 6 ---------------------------------------------------------------------------
class _Recorder:
    def __init__(self, ext):
        self._ext, self.calls = ext, []

    def __getattr__(self, name):
        fn = getattr(self._ext, name)

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


@pytest.mark.parametrize("on", [False, True])
def test_the_tick_launches_settle_or_the_pair_never_both(on):
    pipe = _pipe([DagSpec(steps=[_worker()])], step_policy=on)
    pipe.ext = rec = _Recorder(pipe.ext)
    pipe.admit([0])
    pipe.tick()
    pipe.tick()
    if on:
        assert rec.calls.count("wf_settle") == 2
        assert "wf_timeout_scan" not in rec.calls and "wf_commit" not in rec.calls
    else:
        assert rec.calls.count("wf_timeout_scan") == rec.calls.count("wf_commit") == 2
        assert "wf_settle" not in rec.calls
        assert not hasattr(pipe, "tmpl_policy") and not hasattr(pipe, "run_tmpl")
    i = rec.calls.index("wf_settle" if on else "wf_commit")
    assert rec.calls[i + 1] == "wf_status"


# 7 ---------------------------------------------------------------------------
def test_step_policy_needs_dynamic_mode():
    with pytest.raises(ValueError, match="dynamic_capacity"):
        WorkflowPipeline(device="cpu", dags=[DagSpec(steps=[_worker()])], backend="ref",
                         step_policy=True)


@pytest.mark.parametrize("spec", [_worker(retry=RetrySpec(1)), _worker(timeout_ticks=9)])
def test_a_policy_on_a_pipeline_without_the_option_is_refused(spec):
    dag = DagSpec(steps=[spec])
    with pytest.raises(ValueError, match="step_policy"):
        _pipe([dag], step_policy=False)
    with pytest.raises(ValueError, match="step_policy"):       # static mode
        WorkflowPipeline(device="cpu", dags=[dag], backend="ref")
    pipe = _pipe([], step_policy=False)
    with pytest.raises(ValueError, match="step_policy"):
        pipe.add_template(dag)
    assert pipe.n_templates == 0


BAD_SPECS = [
    (_worker(timeout_ticks=7), "timeout_cutoff"),           # 0 < 7 < cutoff 8
    (_worker(timeout_ticks=1), "timeout_cutoff"),
    (_worker(retry=RetrySpec(-1)), "max_retries"),
    (_worker(retry=RetrySpec(32768)), "max_retries"),
    (_worker(retry=RetrySpec(1, backoff_ticks=0)), "backoff_ticks"),
    (_worker(retry=RetrySpec(1, backoff_ticks=(1 << 20) + 1)), "backoff_ticks"),
    (_worker(retry=RetrySpec(1, multiplier_q8=255)), "multiplier_q8"),
    (_worker(retry=RetrySpec(1, multiplier_q8=65536)), "multiplier_q8"),
    (_worker(retry=RetrySpec(1, cap_ticks=-1)), "cap_ticks"),
    (_worker(retry=RetrySpec(1, cap_ticks=(1 << 20) + 1)), "cap_ticks"),
    (StepSpec(WFK_APPROVAL, retry=RetrySpec(1)), "emits"),
    (StepSpec(WFK_CONDITION, retry=RetrySpec(1)), "emits"),
    (StepSpec(WFK_DELAY, timeout_ticks=9), "emits"),
    (StepSpec(WFK_APPROVAL, timeout_ticks=9), "emits"),
]


@pytest.mark.parametrize("spec,match", BAD_SPECS)
def test_bad_policies_are_refused_at_construction_and_by_add_template(spec, match):
    dag = DagSpec(steps=[_worker(), spec])
    with pytest.raises(ValueError, match=match):
        _pipe([dag], timeout_cutoff=8)
    pipe = _pipe([], timeout_cutoff=8)
    with pytest.raises(ValueError, match=match):
        pipe.add_template(dag)
    assert pipe.n_templates == 0


def test_the_edges_of_every_range_are_accepted():
    pipe = _pipe([], timeout_cutoff=8)
    for spec in (_worker(timeout_ticks=8), _worker(retry=RetrySpec(0)),
                 _worker(retry=RetrySpec(32767, 1, 256, 0)),
                 StepSpec(WFK_FOR_EACH, fanout=2,
                          retry=RetrySpec(1, 1 << 20, 65535, 1 << 20))):
        pipe.add_template(DagSpec(steps=[spec]))
    assert pipe.n_templates == 4
    assert pipe.tmpl_policy[4 * 64 * 3:4 * 64 * 3 + 4].tolist() == \
        [1, 1 << 20, 1 << 20, 65535]
    assert int(pipe.tmpl_timeout.min()) == 8          # resolved: never 0


# 8 ---------------------------------------------------------------------------
def _wf(retry=None, timeout_sec=0, **extra):
    step = {"type": "worker", "topic": "job.x"}
    if retry is not None:
        step["retry"] = retry
    if timeout_sec:
        step["timeout_sec"] = timeout_sec
    step.update(extra)
    return {"id": "wf-policy", "steps": {"only": step}}


def _lower(wf, tick_seconds=1.0, cutoff=8, step_policy=True):
    from cordum_amd.workflow.device_runs import dag_from_workflow

    return dag_from_workflow(wf, 0, tick_seconds, step_policy=step_policy,
                             timeout_cutoff=cutoff)


def _host_ticks(retry, k, tick_seconds):
    import math

    from cordum_amd.workflow.engine import compute_backoff
    from cordum_amd.workflow.models import Step, StepRun

    step = Step.from_dict("only", {"type": "worker", "retry": retry})
    return math.ceil(compute_backoff(step, StepRun(step_id="only", attempts=k)) / tick_seconds)


def test_lowering_a_retry_block():
    from cordum_amd.ops.reference import wf_backoff_ref

    dag = _lower(_wf({"max_retries": 2, "initial_backoff_sec": 1, "multiplier": 2}), 0.5)
    assert dag.steps[0].retry == RetrySpec(2, 2, 512, 0)
    block = {"max_retries": 12, "initial_backoff_sec": 2, "multiplier": 1.5}
    r = _lower(_wf(block)).steps[0].retry
    assert r == RetrySpec(12, 2, 384, 0)
    got = [wf_backoff_ref(k, r.backoff_ticks, r.cap_ticks, r.multiplier_q8)
           for k in range(1, 13)]
    assert got == [2, 3, 5, 7, 11, 16, 23, 35, 52, 77, 116, 173]
    assert got == [_host_ticks(block, k, 1.0) for k in range(1, 13)]
    # a cap, and the host's defaults for initial <= 0 and multiplier <= 1
    r = _lower(_wf({"max_retries": 6, "max_backoff_sec": 5})).steps[0].retry
    assert r == RetrySpec(6, 1, 512, 5)


def test_lowering_proves_itself_and_gives_up_where_the_schedules_part():
    from cordum_amd.ops.reference import wf_backoff_ref

    block = {"max_retries": 23, "initial_backoff_sec": 1, "multiplier": 1.1}
    r = _lower(_wf(block)).steps[0].retry
    assert r == RetrySpec(23, 1, 282, 0)
    for k in range(1, 24):
        assert wf_backoff_ref(k, 1, 0, 282) == _host_ticks(block, k, 1.0), k
    block["max_retries"] = 24
    assert _lower(_wf(block)) is None
    assert (wf_backoff_ref(24, 1, 0, 282), _host_ticks(block, 24, 1.0)) == (10, 9)
    assert _lower(_wf({"max_retries": 1, "multiplier": 256})) is None    # q8 > 65535
    assert _lower(_wf({"max_retries": 40000})) is None
    assert _lower(_wf({"max_retries": 1, "initial_backoff_sec": 2 << 20})) is None


def test_lowering_no_block_timeouts_and_what_stays_on_the_host():
    assert _lower(_wf()).steps[0].retry == RetrySpec(max_retries=0)
    assert _lower(_wf({"max_retries": 0})).steps[0].retry == RetrySpec(max_retries=0)
    assert _lower(_wf()).steps[0].timeout_ticks == 0
    assert _lower(_wf(timeout_sec=3)).steps[0].timeout_ticks == 8
    assert _lower(_wf(timeout_sec=20)).steps[0].timeout_ticks == 20
    assert _lower(_wf(timeout_sec=20), tick_seconds=0.5).steps[0].timeout_ticks == 40
    # step_policy off: today's result, value for value
    assert _lower(_wf({"max_retries": 1}), step_policy=False) is None
    plain = _lower(_wf(timeout_sec=20), step_policy=False)
    assert plain == DagSpec(steps=[StepSpec(WFK_WORKER, deps=[])])
    assert plain.steps[0].retry is None and plain.steps[0].timeout_ticks == 0
    for extra in ({"on_error": "other"}, {"condition": "x > 1"}, {"delay_until": "2030"}):
        assert _lower(_wf({"max_retries": 1}, **extra)) is None
    # a for_each step carries its policy too
    from cordum_amd.workflow.device_runs import dag_from_workflow

    fe = _wf({"max_retries": 3}, timeout_sec=9, for_each="input.items", max_parallel=2)
    spec = dag_from_workflow(fe, 5, step_policy=True, timeout_cutoff=8).steps[0]
    assert (spec.kind, spec.fanout, spec.max_parallel) == (WFK_FOR_EACH, 5, 2)
    assert spec.retry == RetrySpec(3, 1, 512, 0) and spec.timeout_ticks == 9


# 9 ---------------------------------------------------------------------------
def _timeline(retry):
    """One run of a workflow with a single for_each worker step over two
    items, every child failing. The journal reports a step's state as it is
    between ticks, so a retry shows only if the step was seen DISPATCHED:
    with room for one child per tick in the exchange (pad_cap=1) the second
    child's result arrives a tick later."""
    from cordum_amd.workflow.device_runs import DeviceRunTable
    from cordum_amd.workflow.models import Workflow, WorkflowRun
    from cordum_amd.workflow.store import WorkflowStore

    pipe = _pipe([], fail_ppt=1000, max_retries=2, event_cap=512, pad_cap=1)
    store = WorkflowStore()
    table = DeviceRunTable(pipe, store=store)
    wf = Workflow.from_dict(_wf(retry, for_each="input.items"))
    tmpl = table.register(wf, items_len=2)
    assert tmpl == 0
    store.create_run(WorkflowRun(id="r1", workflow_id="wf-policy"))
    assert table.submit("r1", tmpl, fanout=2)
    done = {}
    for _ in range(12):
        table.tick()
        done.update(table.poll())
        if done:
            break
    tl = store.get_timeline("r1")
    return done, [(e.type, e.status) for e in tl], store.get_run("r1")


def test_a_lowered_retry_block_shows_in_the_run_table_timeline():
    from cordum_amd.workflow.models import RUN_FAILED

    done, events, run = _timeline({"max_retries": 1})
    assert done == {"r1": RUN_FAILED} and run.status == RUN_FAILED
    types = [e[0] for e in events]
    assert types.count("step_retry_scheduled") == 1
    i = types.index("step_retry_scheduled")
    assert ("step_completed", "failed") in events[i + 1:]
    assert types.count("step_completed") == 1
    assert events[-1] == ("run_status", RUN_FAILED)
    assert run.steps["only"].status == "failed"

    done, events, run = _timeline(None)
    assert done == {"r1": RUN_FAILED}
    types = [e[0] for e in events]
    assert "step_retry_scheduled" not in types
    assert ("step_completed", "failed") in events and events[-1] == ("run_status", RUN_FAILED)
