"""Host run table over the device run lifecycle (workflow/device_runs.py) on
the CPU reference backend: the Workflow -> DagSpec lowering, the FIFO of
submissions that found the table full, cancellation by run id, and the
RUN_* status strings against the host workflow engine."""
import random

import pytest

from cordum_amd.ops.wf_pipeline import (
    DagSpec,
    StepSpec,
    WFK_APPROVAL,
    WFK_DELAY,
    WFK_FOR_EACH,
    WFK_WORKER,
    WorkflowPipeline,
)
from cordum_amd.workflow import Step, Workflow
from cordum_amd.workflow.device_runs import DeviceRunTable, dag_from_workflow
from cordum_amd.workflow.models import RUN_CANCELLED, RUN_FAILED, RUN_SUCCEEDED
from tests.test_wf_pipeline import _host_oracle_run

pytestmark = pytest.mark.timeout(300)


def mk_pipe(dags, **kw):
    kw.setdefault("device", "cpu")
    kw.setdefault("backend", "ref")
    kw.setdefault("n_local_workers", 16)
    kw.setdefault("payload_words", 4)
    return WorkflowPipeline(dags=dags, **kw)


def workflow_steps(dag):
    """The step dicts _host_oracle_run builds for `dag`."""
    steps = {}
    for i, spec in enumerate(dag.steps):
        deps = [f"s{d}" for d in spec.deps]
        if spec.kind == WFK_WORKER:
            sd = {"type": "worker", "topic": "job.t", "depends_on": deps}
        elif spec.kind == WFK_FOR_EACH:
            sd = {"type": "worker", "topic": "job.t", "depends_on": deps,
                  "for_each": "${input.items}"}
            if spec.max_parallel:
                sd["max_parallel"] = spec.max_parallel
        elif spec.kind == WFK_APPROVAL:
            sd = {"type": "approval", "depends_on": deps}
        else:
            assert spec.kind == WFK_DELAY
            sd = {"type": "delay", "delay_sec": spec.delay_ticks, "depends_on": deps}
        steps[f"s{i}"] = sd
    return steps


def workflow_of(dag):
    return Workflow(id="wf", org_id="org",
                    steps={sid: Step.from_dict(sid, sd)
                           for sid, sd in workflow_steps(dag).items()})


def random_dag(rng, fan):
    """A random supported DAG in canonical form (what the lowering returns)."""
    steps = []
    for s in range(rng.randint(1, 6)):
        deps = [d for d in range(s) if rng.random() < 0.5]
        kind = rng.choice([WFK_WORKER, WFK_FOR_EACH, WFK_APPROVAL, WFK_DELAY])
        steps.append(StepSpec(
            kind, deps=deps, fanout=fan if kind == WFK_FOR_EACH else 1,
            max_parallel=rng.choice([0, 0, 2, 3]) if kind == WFK_FOR_EACH else 0,
            delay_ticks=rng.randint(0, 3) if kind == WFK_DELAY else 0))
    return DagSpec(steps=steps)


def test_round_trip_over_the_host_oracle_mapping():
    rng = random.Random(5)
    for _ in range(30):
        fan = rng.randint(1, 9)
        dag = random_dag(rng, fan)
        assert dag_from_workflow(workflow_of(dag), fan) == dag
        # the dict form lowers alike
        assert dag_from_workflow({"steps": workflow_steps(dag)}, fan) == dag


def test_delay_seconds_round_up_to_ticks():
    dag = DagSpec(steps=[StepSpec(WFK_DELAY, delay_ticks=5)])
    wf = workflow_of(dag)
    assert dag_from_workflow(wf, 1, tick_seconds=2.0).steps[0].delay_ticks == 3
    assert dag_from_workflow(wf, 1, tick_seconds=5.0).steps[0].delay_ticks == 1
    assert dag_from_workflow(wf, 1, tick_seconds=0.5).steps[0].delay_ticks == 10


BASE = {"a": {"type": "worker", "topic": "job.t"},
        "b": {"type": "worker", "topic": "job.t", "depends_on": ["a"]}}


def _with(step_id, **fields):
    steps = {k: dict(v) for k, v in BASE.items()}
    steps.setdefault(step_id, {"type": "worker"}).update(fields)
    return {"steps": steps}


@pytest.mark.parametrize("workflow", [
    _with("b", type="condition"),
    _with("b", type="parallel"),
    _with("b", condition="${input.x} > 1"),
    _with("b", type="delay", delay_until="2030-01-01T00:00:00Z"),
    _with("b", on_error="a"),
    _with("b", retry={"max_retries": 3}),
    _with("a", depends_on=["b"]),          # a later step
    _with("b", depends_on=["nope"]),       # an unknown step
    {"steps": {f"s{i}": {"type": "worker"} for i in range(65)}},
], ids=["type-condition", "type-parallel", "condition-expr", "delay-until",
        "on-error", "retry-block", "later-dep", "unknown-dep", "65-steps"])
def test_unsupported_workflows_stay_on_the_host(workflow):
    assert dag_from_workflow(workflow, 4) is None


def test_supported_base_and_the_64_step_limit():
    assert dag_from_workflow({"steps": BASE}, 4) == DagSpec(steps=[
        StepSpec(WFK_WORKER, deps=[]), StepSpec(WFK_WORKER, deps=[0])])
    wf64 = {"steps": {f"s{i}": {"type": "worker"} for i in range(64)}}
    assert len(dag_from_workflow(wf64, 1).steps) == 64
    # a for_each over no items cannot complete on the device
    assert dag_from_workflow(_with("b", for_each="${input.items}"), 0) is None
    assert dag_from_workflow(_with("b", for_each="${input.items}"), 3).steps[1] == \
        StepSpec(WFK_FOR_EACH, deps=[0], fanout=3)


def test_fifo_of_submissions_that_found_the_table_full():
    pipe = mk_pipe([DagSpec(steps=[StepSpec(WFK_WORKER)])], dynamic_capacity=2)
    table = DeviceRunTable(pipe)
    assert [table.submit(f"r{i}", 0) for i in range(5)] == [True, True, False, False, False]
    assert table.queued() == 3 and len(table) == 5
    assert table.handle("r0") == (0, 1) and table.handle("r2") is None
    with pytest.raises(ValueError):
        table.submit("r3", 0)              # already queued
    with pytest.raises(ValueError):
        table.submit("r9", 7)              # unknown template
    assert table.poll() == []              # nothing ended, nothing admitted
    for _ in range(3):
        table.tick()
    # the drain comes first, then the queue head takes the freed slots
    assert table.poll() == [("r0", RUN_SUCCEEDED), ("r1", RUN_SUCCEEDED)]
    assert table.queued() == 1
    assert table.handle("r2") == (0, 2) and table.handle("r3") == (1, 2)
    # a new submission does not overtake the one still waiting
    for _ in range(3):
        table.tick()
    assert table.submit("r5", 0) is False and table.queued() == 2
    assert table.poll() == [("r2", RUN_SUCCEEDED), ("r3", RUN_SUCCEEDED)]
    assert table.handle("r4") == (0, 3) and table.handle("r5") == (1, 3)
    for _ in range(3):
        table.tick()
    assert table.poll() == [("r4", RUN_SUCCEEDED), ("r5", RUN_SUCCEEDED)]
    assert len(table) == 0 and table.poll() == []


def test_cancel_queued_and_live_runs():
    dag = DagSpec(steps=[StepSpec(WFK_DELAY, delay_ticks=4),
                         StepSpec(WFK_WORKER, deps=[0])])
    pipe = mk_pipe([dag], dynamic_capacity=1)
    table = DeviceRunTable(pipe)
    assert table.submit("live", 0) and not table.submit("queued", 0)
    assert not table.submit("next", 0)
    launches = int(pipe.cancel_count[0]), int(pipe.admit_count[0])
    assert table.cancel("queued") is True          # without touching the device
    assert (int(pipe.cancel_count[0]), int(pipe.admit_count[0])) == launches
    assert table.cancel("queued") is False and table.cancel("nobody") is False
    table.tick()
    assert table.cancel("live") is True and table.cancel("live") is False
    assert int(pipe.cancel_count[0]) == 1
    assert sorted(table.poll()) == [("live", RUN_CANCELLED), ("queued", RUN_CANCELLED)]
    assert table.handle("next") == (0, 2)          # admitted by that poll
    for _ in range(8):
        table.tick()
    assert table.poll() == [("next", RUN_SUCCEEDED)]
    assert table.cancel("next") is False           # already reported


def test_status_strings():
    assert (RUN_SUCCEEDED, RUN_FAILED, RUN_CANCELLED) == ("succeeded", "failed", "cancelled")
    dag = DagSpec(steps=[StepSpec(WFK_WORKER)])
    table = DeviceRunTable(mk_pipe([dag], dynamic_capacity=2, fail_ppt=1000,
                                   max_retries=0))
    table.submit("f", 0)
    table.submit("c", 0)
    table.cancel("c")
    table.tick()
    assert sorted(table.poll()) == [("c", "cancelled"), ("f", "failed")]
    with pytest.raises(RuntimeError):
        DeviceRunTable(mk_pipe([dag]))             # a static pipeline


def test_polled_status_equals_the_host_engine_on_random_workflows():
    rng = random.Random(42)
    cases = []
    for _ in range(10):
        fan = rng.randint(1, 9)
        cases.append((random_dag(rng, fan), fan))
    pipe = mk_pipe([], dynamic_capacity=4)
    table = DeviceRunTable(pipe)
    for i, (dag, fan) in enumerate(cases):
        lowered = dag_from_workflow(workflow_of(dag), fan)
        assert lowered is not None
        table.submit(f"run-{i}", pipe.add_template(lowered))
    got = {}
    for _ in range(200):
        table.tick()
        got.update(table.poll())
        if len(got) == len(cases):
            break
    assert table.queued() == 0 and len(table) == 0
    for i, (dag, fan) in enumerate(cases):
        assert got[f"run-{i}"] == _host_oracle_run(dag, fan), i
