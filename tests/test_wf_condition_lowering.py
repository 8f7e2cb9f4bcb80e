"""Lowering of `condition` expressions to device predicates
(`dag_from_workflow(conditions=True)`, `lower_condition`) and the run table on
top (`submit(input=...)`, `step_outputs`).

The lowering is proved, not assumed: every lowered form is evaluated by the
device's oracle (`wf_cond_eval_ref`) over operand values where signed 32-bit
arithmetic is most likely to differ from the host's floats, and must decide
as `eval.eval_condition` decides on the same scope.
"""
import json
import random

import pytest
import torch

from cordum_amd.bus import LoopbackBus
from cordum_amd.ops.reference import WFL_LIVE, WFS_PENDING, WFS_SKIPPED, WFS_SUCCEEDED
from cordum_amd.ops.reference import wf_cond_eval_ref
from cordum_amd.ops.wf_pipeline import WFK_CONDITION, WFK_WORKER, WorkflowPipeline
from cordum_amd.protocol import subjects as subj
from cordum_amd.protocol.capv2 import JobResult, JobStatus
from cordum_amd.store import MemoryStore
from cordum_amd.utils.clock import ManualClock
from cordum_amd.workflow import Engine, Step, Workflow, WorkflowRun, WorkflowStore
from cordum_amd.workflow import eval as wfeval
from cordum_amd.workflow.device_runs import DeviceRunTable, dag_from_workflow

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
OPS = ("==", "!=", ">=", "<=", ">", "<")
_rng = random.Random(4711)
VALUES = (I32_MIN, -1, 0, 1, I32_MAX, _rng.randrange(I32_MIN, I32_MAX),
          _rng.randrange(-1000, 1000))
LITERALS = ("0", "-1", "1", "2147483647", "-2147483648", "+7")


def workflow_with(expr, on="t", extra=None):
    """a, b: workers; c, d: condition steps; t: a worker behind all four that
    carries `expr` as its guard."""
    steps = {
        "a": {"type": "worker", "topic": "job.x"},
        "b": {"type": "worker", "topic": "job.x", "depends_on": ["a"]},
        "c": {"type": "condition", "condition": "input.p > 0", "depends_on": ["b"]},
        "d": {"type": "condition", "condition": "input.q > 0", "depends_on": ["b"]},
        "t": {"type": "worker", "topic": "job.x", "depends_on": ["c", "d"],
              "condition": expr},
    }
    steps.update(extra or {})
    return {"id": "wf", "steps": steps}


NUM = ("input.x", "input.y", "steps.a.output", "steps.b.output")
NUM_PAIRS = (("input.x", "input.y"), ("input.x", "steps.a.output"),
             ("steps.a.output", "input.x"), ("steps.a.output", "steps.b.output"),
             ("input.x", "input.x"))
BOOL_PAIRS = (("steps.c.output", "steps.d.output"), ("steps.c.output", "true"),
              ("steps.d.output", "false"), ("true", "steps.c.output"),
              ("false", "steps.d.output"))


def lowered_forms():
    forms = []
    for op in OPS:
        for lhs, rhs in NUM_PAIRS:
            forms.append(f"{lhs} {op} {rhs}")
        for k, lit in enumerate(LITERALS):
            forms.append(f"{NUM[k % 4]} {op} {lit}")
            forms.append(f"{lit}{op}{NUM[(k + 2) % 4]}")       # flipped, and no spaces
    for op in ("==", "!="):
        for lhs, rhs in BOOL_PAIRS:
            forms.append(f"{lhs} {op} {rhs}")
    forms += ["input.x", "steps.a.output", "steps.c.output", " steps.b.output "]
    return forms + ["!" + f for f in forms] + ["! input.y < 3"]


def _operands(expr):
    return [n for n in ("input.x", "input.y", "steps.a.output", "steps.b.output",
                        "steps.c.output", "steps.d.output") if n in expr]


def _scopes(expr):
    """Scopes over every combination of values of the operands `expr` names."""
    names = _operands(expr)
    combos = [{}]
    for n in names:
        vals = (True, False) if n in ("steps.c.output", "steps.d.output") else VALUES
        combos = [dict(c, **{n: v}) for c in combos for v in vals]
    for c in combos:
        scope = {"input": {"x": c.get("input.x", 3), "y": c.get("input.y", 4),
                           "p": 1, "q": 1},
                 "steps": {s: {"output": c.get(f"steps.{s}.output", 0)} for s in "abcd"}}
        yield scope


def test_every_lowered_form_decides_as_the_host_evaluator():
    forms = lowered_forms()
    assert len(forms) <= 256
    pipe = WorkflowPipeline("cpu", [], backend="ref", dynamic_capacity=1,
                            device_conditions=True, payload_words=10, template_cap=256)
    IW = pipe.input_words
    rows = []                                   # (template, scope, expr, input names)
    for expr in forms:
        dag = dag_from_workflow(workflow_with(expr), 0, conditions=True)
        assert dag is not None, expr
        assert dag.steps[4].kind == WFK_WORKER and dag.steps[4].when is not None
        t = pipe.add_template(dag)
        for scope in _scopes(expr):
            rows.append((t, scope, expr, dag.input_names))
    NR = len(rows)
    state = torch.full((NR, 64), WFS_SUCCEEDED, dtype=torch.uint8)
    state[:, 4] = WFS_PENDING
    tm = torch.tensor([r[0] for r in rows], dtype=torch.int64)
    deps = pipe.tmpl_deps.view(-1, 64)[tm].reshape(-1).clone()
    kind = pipe.tmpl_kind.view(-1, 64)[tm].reshape(-1).clone()
    inp = torch.zeros((NR, IW), dtype=torch.int32)
    out = torch.zeros((NR, 64), dtype=torch.int32)
    for r, (t, scope, expr, names) in enumerate(rows):
        for k, name in enumerate(names):
            inp[r, k] = scope["input"][name]
        for j, s in enumerate("abcd"):
            out[r, j] = int(scope["steps"][s]["output"])
    counts = torch.zeros(2, dtype=torch.int64)
    wf_cond_eval_ref(state.view(-1), deps, kind, torch.full((NR,), WFL_LIVE, dtype=torch.uint8),
                     torch.ones(NR, dtype=torch.uint8), tm.to(torch.int32), pipe.tmpl_cond,
                     pipe.tmpl_cond_mask, inp.view(-1), out.view(-1),
                     torch.zeros(NR, dtype=torch.int64), counts, IW)
    assert int(counts.sum()) == NR
    n_true = 0
    for r, (t, scope, expr, names) in enumerate(rows):
        host = wfeval.eval_condition(expr, scope)
        device = int(state[r, 4]) != WFS_SKIPPED
        assert device == host, (expr, scope)
        n_true += host
    assert 0 < n_true < NR and int(counts[0]) == n_true


@pytest.mark.parametrize("expr", [
    "steps.c.output == 1",                # the host compares "true" with "1"
    "steps.c.output > 0",
    "input.x == steps.c.output",
    "steps.c.output == input.x",
    "steps.c.output >= steps.d.output",   # booleans only know == and !=
    "true",                               # a bare literal
    "5",
    "3 < 4",                              # two literals
    "steps.g.output > 1",                 # a guarded worker: nil on the host, 0 here
    "steps.fe.output > 1",                # a for_each step
    "steps.t.output > 1",                 # the step itself
    "steps.z.output > 1",                 # after it / not a dependency
    "steps.nope.output > 1",
    "steps.ap.output == true",            # an approval has no output
    "length(input.items) > 2",
    "first(input.items) == 1",
    "input.name == 'x'",
    'input.name == "x"',
    "ctx.v > 1",
    "item > 1",
    "item.v == 2",
    "input.x > 1.5",                      # not an integer
    "input.x > 1e3",
    "input.x > 2147483648",               # outside int32
    "input.x < -2147483649",
    "input.a.b > 1",                      # more than one path segment
    "input.x > 1 == true",                # more than one operator
    "!!input.x",
    "input.x >",
    "   ",                                # the host never runs such a step
])
def test_forms_outside_the_subset_stay_on_the_host(expr):
    extra = {
        "g": {"type": "worker", "topic": "job.x", "condition": "input.p > 0"},
        "fe": {"type": "worker", "topic": "job.x", "for_each": "input.items"},
        "ap": {"type": "approval"},
    }
    wf = workflow_with(expr, extra=extra)
    wf["steps"]["t"]["depends_on"] = ["c", "d", "g", "fe", "ap"]
    # t is moved behind the extra steps, z comes after it
    wf["steps"]["t"] = wf["steps"].pop("t")
    wf["steps"]["z"] = {"type": "worker", "topic": "job.x"}
    assert dag_from_workflow(wf, 2, conditions=True) is None
    wf["steps"]["t"]["condition"] = "steps.c.output"
    assert dag_from_workflow(wf, 2, conditions=True) is not None


def test_more_input_names_than_words_stays_on_the_host():
    expr = "input.x > input.y"
    assert dag_from_workflow(workflow_with(expr), 0, conditions=True, input_words=4) is not None
    # p and q are named by c and d, x and y by t: four words
    assert dag_from_workflow(workflow_with(expr), 0, conditions=True, input_words=3) is None
    dag = dag_from_workflow(workflow_with(expr), 0, conditions=True, input_words=4)
    assert dag.input_names == ["p", "q", "x", "y"]


def test_a_condition_step_needs_an_expression_and_the_option():
    wf = workflow_with("input.x > 1")
    assert dag_from_workflow(wf, 0) is None
    assert dag_from_workflow(wf, 0, conditions=False) is None
    dag = dag_from_workflow(wf, 0, conditions=True)
    assert [s.kind for s in dag.steps] == [WFK_WORKER, WFK_WORKER, WFK_CONDITION,
                                           WFK_CONDITION, WFK_WORKER]
    assert all(dag.steps[i].when is not None for i in (2, 3, 4))
    wf["steps"]["c"]["condition"] = ""
    assert dag_from_workflow(wf, 0, conditions=True) is None
    # a workflow without any condition lowers as before, with or without it
    plain = {"steps": {"a": {"type": "worker"}, "b": {"type": "delay", "delay_sec": 2,
                                                      "depends_on": ["a"]}}}
    a, b = dag_from_workflow(plain, 0), dag_from_workflow(plain, 0, conditions=True)
    assert a == b and a is not None and a.input_names == []


def _table(NR=2, **kw):
    pipe = WorkflowPipeline("cpu", [], backend="ref", dynamic_capacity=NR, child_cap=64,
                            n_local_workers=4, device_conditions=True, payload_words=10,
                            **kw)
    return pipe, DeviceRunTable(pipe)


def test_submit_maps_the_input_and_refuses_what_the_device_cannot_hold():
    pipe, tab = _table(NR=1)
    t = tab.register(workflow_with("input.x > input.y"))
    for bad in ({"p": 1, "q": 1, "x": 1}, {"p": 1, "q": 1, "x": 1, "y": "2"},
                {"p": 1, "q": 1, "x": True, "y": 2}, {"p": 1, "q": 1, "x": 1.0, "y": 2},
                {"p": 1, "q": 1, "x": 1 << 31, "y": 2}, None):
        with pytest.raises(ValueError, match="input field"):
            tab.submit("r", t, input=bad)
    assert len(tab) == 0 and int(pipe.run_life.sum()) == 0
    assert tab.submit("r1", t, input={"p": 1, "q": -1, "x": 9, "y": I32_MIN, "other": "s"})
    assert pipe.run_input.tolist() == [1, -1, 9, I32_MIN, 0, 0, 0, 0]
    # the table is full: the words wait in the queue with the submission
    assert not tab.submit("r2", t, input={"p": 2, "q": 2, "x": 2, "y": 2})
    for _ in range(8):
        tab.tick()
    assert tab.poll() == [("r1", "succeeded")]
    assert tab.handle("r2") == (0, 2)
    assert pipe.run_input.tolist() == [2, 2, 2, 2, 0, 0, 0, 0]
    with pytest.raises(KeyError):
        tab.step_outputs("r1")


# ---- against the host engine ---------------------------------------------------
WF = {
    "a": {"type": "worker", "topic": "job.x"},
    "c": {"type": "condition", "condition": "steps.a.output > input.limit",
          "depends_on": ["a"]},
    "hi": {"type": "worker", "topic": "job.x", "depends_on": ["c"],
           "condition": "steps.c.output"},
    "lo": {"type": "worker", "topic": "job.x", "depends_on": ["c"],
           "condition": "steps.c.output == false"},
    "ap": {"type": "approval", "depends_on": ["c"], "condition": "0 > input.bonus"},
    "fin": {"type": "worker", "topic": "job.x", "depends_on": ["hi", "lo", "ap"],
            "condition": "!steps.a.output == -1"},
}


def _host_run(run_input, words):
    """Drive the host engine on WF; the stub worker answers every job with the
    number the device's echo worker computes for it: the sum of the run's
    input words + the child's ordinal (0: nothing fails) + the step's index."""
    clock = ManualClock()
    bus = LoopbackBus(clock=clock)
    store = WorkflowStore(clock=clock)
    memory = MemoryStore(clock=clock)
    engine = Engine(store, bus, memory=memory, clock=clock)
    submitted = []
    bus.subscribe(subj.SUBJECT_SUBMIT, lambda s, p: submitted.append(p.job_request))
    wf = Workflow(id="wf", org_id="org",
                  steps={sid: Step.from_dict(sid, sd) for sid, sd in WF.items()})
    store.put_workflow(wf)
    store.create_run(WorkflowRun(id="run", workflow_id="wf", org_id="org", input=run_input))
    engine.start_run("wf", "run")
    order = list(WF)
    answered = 0
    while True:
        while answered < len(submitted):
            job_id = submitted[answered].job_id
            answered += 1
            step_id = job_id.split(":")[1].split("@")[0]
            ptr = memory.put_result(
                job_id, json.dumps(sum(words) + order.index(step_id)).encode())
            engine.handle_job_result(JobResult(job_id=job_id, status=JobStatus.SUCCEEDED,
                                               result_ptr=ptr))
        # the device pipeline's approver (approvals="auto") grants every hold
        waiting = [sid for sid, sr in store.get_run("run").steps.items()
                   if sr.status == "waiting"]
        if not waiting:
            break
        for sid in waiting:
            engine.approve_step("run", sid, True)
    run = store.get_run("run")
    return run.status, {sid: run.steps[sid].status for sid in WF}, run


@pytest.mark.parametrize("run_input", [{"limit": 10, "bonus": 5}, {"limit": 10, "bonus": -5},
                                       {"limit": -1, "bonus": 0}])
def test_a_registered_workflow_ends_as_on_the_host_engine(run_input):
    pipe, tab = _table()
    t = tab.register({"id": "wf", "steps": WF})
    assert t is not None
    names = tab._tmpl_inputs[t]
    assert names == ["limit", "bonus"]
    words = [run_input[n] for n in names]
    assert tab.submit("run", t, input=run_input)
    status = None
    for _ in range(12):
        tab.tick()
        device_steps = tab.step_states("run")
        outs = tab.step_outputs("run")
        done = tab.poll()
        if done:
            status = done[0][1]
            break
    host_status, host_steps, run = _host_run(run_input, words)
    assert status == host_status == "succeeded"
    assert device_steps == host_steps
    # and the numbers the two engines decided on are the same numbers
    order = list(WF)
    for sid in ("a", "hi", "lo", "fin"):
        host_out = (run.context.get("steps", {}).get(sid) or {}).get("output")
        if host_out is None:                  # gated off on the host: never ran
            assert outs[sid] == 0
        else:
            assert outs[sid] == host_out == sum(words) + order.index(sid)
    assert outs["c"] == int(run.context["steps"]["c"]["output"])
