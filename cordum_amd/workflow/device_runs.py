"""Host run table over the device workflow engine's run lifecycle.

`WorkflowPipeline` in dynamic mode (ops/wf_pipeline.py) speaks slots and
generations; the serving layer speaks run ids and `RUN_*` status strings
(workflow/models.py). `DeviceRunTable` is the map between the two: it admits
submissions (queueing them FIFO while the device table is full), cancels by
run id, and turns the device's completion records into `(run_id, status)`
pairs. `dag_from_workflow` lowers a `Workflow` to the `DagSpec` the device
runs, or says (None) that the workflow must stay on the host engine.

With the pipeline's step journal on (`event_cap`), the table also turns the
device's step-transition records into `StepEvent`s keyed by run id, per-step
`STEP_*` statuses, and, given a `WorkflowStore`, the timeline events and run
records the API serves.

On a pipeline with `approvals="external"` the table serves approval gates as
the host engine's `approve_step` does: `approvals()` lists the holds that
wait for a decision, `approve()` / `reject()` settle one by run id and step
id, and `approval_ttl_sec` at registration lets holds expire (an expired hold
shows as `step_rejected`).

On a pipeline with `step_policy=True` registration also lowers each worker
step's `retry` block and `timeout_sec` (`lower_retry`, `dag_from_workflow`):
a step retries as often, and waits as many ticks, as the host engine would.

On a pipeline with `device_conditions=True` registration lowers `condition`
steps and `condition` guards over the run's input and over step outputs
(`lower_condition`), `submit(input=...)` maps the run's input fields onto the
device's input words, and `step_outputs()` reads a run's output words. A step
whose guard is false shows as PENDING -> SKIPPED in the events, which
`timeline_of` reports as `step_condition_evaluated {"value": False}` with
status succeeded; the host engine completes such a step as succeeded without
recording an event. That is the one difference.

`rerun_from()` starts a new run of a run's workflow with the same input and
with the transitive dependencies of a chosen step already finished, as the
host engine's `rerun_from` does: the source is a run in the table, a queued
one, or one of the `retain` last completed ones, whose final step states and
output words the table then keeps.

Wiring an API route to this table, and materialising job results (a step's
output word is a checksum, not the job's result document), are not done here.
"""
from __future__ import annotations

import math
import re
from collections import OrderedDict, deque
from typing import Any, Deque, Dict, List, NamedTuple, Optional, Tuple, Union

from ..ops.reference import wf_backoff_ref
from ..ops.wf_pipeline import (
    CondSpec,
    DagSpec,
    RetrySpec,
    StepSpec,
    WFK_APPROVAL,
    WFK_CONDITION,
    WFK_DELAY,
    WFK_FOR_EACH,
    WFK_WORKER,
    WFS_CANCELLED,
    WFS_DISPATCHED,
    WFS_FAILED,
    WFS_PENDING,
    WFS_SKIPPED,
    WFS_SUCCEEDED,
    WFS_WAITING,
    WorkflowPipeline,
)
from ..utils.clock import SYSTEM_CLOCK
from .models import (
    RUN_CANCELLED,
    RUN_FAILED,
    RUN_SUCCEEDED,
    STEP_CANCELLED,
    STEP_FAILED,
    STEP_PENDING,
    STEP_RUNNING,
    STEP_SUCCEEDED,
    STEP_WAITING,
    Step,
    StepRun,
    TimelineEvent,
)

_STATUS = {
    WFS_SUCCEEDED: RUN_SUCCEEDED,
    WFS_FAILED: RUN_FAILED,
    WFS_CANCELLED: RUN_CANCELLED,
}

# device step state -> the status the API shows. A false condition is
# SKIPPED on the device; the host engine completes it as succeeded with the
# value False (workflow/engine.py, the condition step).
_STEP_STATUS = {
    WFS_PENDING: STEP_PENDING,
    WFS_DISPATCHED: STEP_RUNNING,
    WFS_WAITING: STEP_WAITING,
    WFS_SUCCEEDED: STEP_SUCCEEDED,
    WFS_FAILED: STEP_FAILED,
    WFS_SKIPPED: STEP_SUCCEEDED,
    WFS_CANCELLED: STEP_CANCELLED,
}


class StepEvent(NamedTuple):
    """One journaled step transition of a run. `tick` is the device tick that
    detected it; `between_ticks` marks a pass outside the tick (a cancel)."""
    run_id: str
    step: int
    step_id: str
    from_state: int
    to_state: int
    tick: int
    between_ticks: bool


class PendingApproval(NamedTuple):
    """One approval hold that waits for a decision. `since_tick` is the device
    tick the hold opened in, `expires_tick` the tick whose scan fails it if it
    is still undecided (None: it never expires)."""
    run_id: str
    step: int
    step_id: str
    since_tick: int
    expires_tick: Optional[int]


def timeline_of(kind: int, to_state: int) -> Tuple[str, str, Dict[str, Any]]:
    """(timeline event type, step status, extra data) of a transition into
    `to_state` of a step of `kind`: the host engine's event names where it
    has them, `step_retry_scheduled` and `step_cancelled` where it has none."""
    status = _STEP_STATUS[to_state]
    if to_state == WFS_DISPATCHED:
        return "step_dispatched", status, {}
    if to_state == WFS_WAITING:
        return "step_waiting", status, {}
    if to_state == WFS_SUCCEEDED:
        if kind == WFK_APPROVAL:
            return "step_approved", status, {}
        if kind == WFK_DELAY:
            return "step_delay_completed", status, {}
        if kind == WFK_CONDITION:
            return "step_condition_evaluated", status, {"value": True}
        return "step_completed", status, {}
    if to_state == WFS_SKIPPED:
        return "step_condition_evaluated", status, {"value": False}
    if to_state == WFS_FAILED:
        return ("step_rejected" if kind == WFK_APPROVAL else "step_completed"), status, {}
    if to_state == WFS_CANCELLED:
        return "step_cancelled", status, {}
    # back to PENDING: the device's retry, or a for_each window re-entry
    return "step_retry_scheduled", status, {}


def _steps_of(workflow: Any) -> List[Step]:
    steps = getattr(workflow, "steps", None)
    if steps is None:
        steps = workflow.get("steps", workflow)
    out = []
    for sid, st in steps.items():
        out.append(st if isinstance(st, Step) else Step.from_dict(sid, st))
    return out


def _ceil_ticks(seconds: float, tick_seconds: float) -> int:
    return int(math.ceil(seconds / tick_seconds))


def lower_retry(step: Step, tick_seconds: float) -> Optional[RetrySpec]:
    """The device `RetrySpec` of a worker step's `retry` block, or None if
    the device's integer backoff would not wait what the host engine waits.
    No block (or max_retries <= 0) is the host's "never retry". The result is
    proved, not assumed: for every attempt k in 1..max_retries the device
    formula must give ceil(compute_backoff(step, attempts=k) / tick_seconds)."""
    from .engine import compute_backoff

    cfg = step.retry
    if cfg is None or cfg.max_retries <= 0:
        return RetrySpec(max_retries=0)
    initial = cfg.initial_backoff_sec if cfg.initial_backoff_sec > 0 else 1
    mult = cfg.multiplier if cfg.multiplier > 1 else 2.0
    spec = RetrySpec(
        max_retries=int(cfg.max_retries),
        backoff_ticks=_ceil_ticks(initial, tick_seconds),
        multiplier_q8=int(round(mult * 256)),
        cap_ticks=_ceil_ticks(cfg.max_backoff_sec, tick_seconds)
        if cfg.max_backoff_sec > 0 else 0)
    if not (spec.max_retries <= 32767 and 1 <= spec.backoff_ticks <= 1 << 20
            and 256 <= spec.multiplier_q8 <= 65535 and 0 <= spec.cap_ticks <= 1 << 20):
        return None
    for k in range(1, spec.max_retries + 1):
        try:
            host = _ceil_ticks(compute_backoff(step, StepRun(step_id=step.id, attempts=k)),
                               tick_seconds)
        except OverflowError:       # the host's own float power gave up
            return None
        if wf_backoff_ref(k, spec.backoff_ticks, spec.cap_ticks,
                          spec.multiplier_q8) != host:
            return None
    return spec


_OPS = ["==", "!=", ">=", "<=", ">", "<"]         # eval.py's order of search
_FLIP = {"==": "==", "!=": "!=", ">": "<", "<": ">", ">=": "<=", "<=": ">="}
_RE_INPUT = re.compile(r"input\.([A-Za-z_][A-Za-z0-9_]*)\Z")
_RE_STEP = re.compile(r"steps\.([A-Za-z0-9_-]+)\.output\Z")
_RE_INT = re.compile(r"[+-]?[0-9]+\Z")


def lower_condition(expr: str, steps: List[Step], i: int, names: List[str],
                    input_words: int) -> Optional[CondSpec]:
    """The device predicate of step i's `condition` expression, or None if the
    device would not decide it as `eval.eval_condition` does. The subset is
    `[!] lhs [op rhs]` with op one of == != >= <= > <, split exactly as
    eval.py splits it. An operand is `input.<name>` (an int field of the
    run's input; names take word indices in `names`, in order of first
    appearance), `steps.<id>.output` of a step among the transitive
    dependencies that is an unguarded, non-for_each worker (a number) or a
    condition step (a boolean), an integer literal in int32 range, or `true` /
    `false`. Numbers compare with numbers, with any op; booleans with
    booleans, with == and != only (the host compares everything else as
    strings, or says False). A literal on the left is flipped to the right; a
    bare operand is its truthiness."""
    index = {st.id: j for j, st in enumerate(steps)}
    reach, stack = set(), list(steps[i].depends_on)
    while stack:
        j = index.get(stack.pop())
        if j is not None and j not in reach:
            reach.add(j)
            stack.extend(steps[j].depends_on)
    text = expr.strip()
    negate = text.startswith("!")
    if negate:
        text = text[1:].strip()
    if not text or text.startswith("!"):
        return None
    added: List[str] = []

    def operand(tok: str):
        """(class, operand): class "num" or "bool", literal flag."""
        tok = tok.strip()
        m = _RE_INPUT.match(tok)
        if m:
            name = m.group(1)
            known = names + added
            if name not in known:
                if len(known) >= input_words:
                    return None
                added.append(name)
                known = names + added
            return "num", ("input", known.index(name)), False
        m = _RE_STEP.match(tok)
        if m:
            j = index.get(m.group(1))
            if j is None or j not in reach:
                return None
            ref = steps[j]
            if ref.type == "condition":
                return "bool", ("out", j), False
            if ref.type == "worker" and not ref.for_each and not ref.condition:
                return "num", ("out", j), False
            return None
        if tok in ("true", "false"):
            return "bool", int(tok == "true"), True
        if _RE_INT.match(tok):
            v = int(tok)
            return ("num", v, True) if -(1 << 31) <= v < (1 << 31) else None
        return None

    op = next((o for o in _OPS if o in text), None)
    if op is None:
        a = operand(text)
        if a is None or a[2]:
            return None
        spec = CondSpec("truthy", a[1], 0, negate)
    else:
        k = text.find(op)
        a, b = operand(text[:k]), operand(text[k + len(op):])
        if a is None or b is None or a[0] != b[0] or (a[2] and b[2]):
            return None
        if a[0] == "bool" and op not in ("==", "!="):
            return None
        if a[2]:
            a, b, op = b, a, _FLIP[op]
        spec = CondSpec(op, a[1], b[1], negate)
    names.extend(added)
    return spec


def dag_from_workflow(workflow: Any, items_len: int,
                      tick_seconds: float = 1.0,
                      approval_ttl_sec: float = 0.0,
                      step_policy: bool = False,
                      timeout_cutoff: int = 8,
                      conditions: bool = False,
                      input_words: int = 8) -> Optional[DagSpec]:
    """Lower a workflow (a `Workflow`, or its `{"steps": {id: step}}` dict
    form) to a device `DagSpec`; steps are indexed in `workflow.steps` order.
    Returns None when the workflow cannot run on the device, and the caller
    stays on the host engine: more than 64 steps, a step type other than
    worker / approval / delay (or `condition`, with `conditions`), a
    `condition` expression without `conditions`, `delay_until`,
    `on_error`, a dependency on a later or unknown step, or a `for_each` over
    no items (the device cannot complete a step with nothing to emit).
    `approval_ttl_sec` > 0 gives every approval step that expiry, rounded up
    to ticks (it needs a pipeline with approvals="external"); 0 lowers
    approvals without one.

    Without `step_policy` a per-step `retry` block also returns None, steps
    carry no policy (the pipeline's one `max_retries` applies to all of them,
    which retries steps the host engine would fail at once) and `timeout_sec`
    is not lowered. With `step_policy` (a pipeline with step_policy=True)
    every worker step gets the host's meaning: its `retry` block as a
    `RetrySpec` (see `lower_retry`; no block is max_retries=0, and a block
    whose schedule the device cannot reproduce tick for tick returns None),
    and `timeout_sec` > 0 as `timeout_ticks`, rounded up to ticks and raised
    to `timeout_cutoff`, the pipeline's floor. On the device a step's timeout
    is how long results that never came are waited for before the retry; the
    host engine hands it to the job as its deadline. `retry` and `timeout_sec`
    on approval and delay steps mean nothing to either engine.

    With `conditions` (a pipeline with device_conditions=True) a `condition`
    step lowers to a CONDITION step with a predicate and a `condition` on a
    worker, for_each, approval or delay step to a guard (see
    `lower_condition`; an expression outside its subset returns None). The
    result's `input_names` lists the input fields in word order."""
    steps = _steps_of(workflow)
    ttl = max(0, int(math.ceil(approval_ttl_sec / tick_seconds)))
    if len(steps) > 64:
        return None
    index = {st.id: i for i, st in enumerate(steps)}
    if len(index) != len(steps):
        return None
    specs: List[StepSpec] = []
    names: List[str] = []
    for i, st in enumerate(steps):
        if st.delay_until or st.on_error:
            return None
        if (st.condition or st.type == "condition") and not conditions:
            return None
        if st.retry is not None and not step_policy:
            return None
        deps = []
        for dep in st.depends_on:
            j = index.get(dep)
            if j is None or j >= i:
                return None
            deps.append(j)
        when = None
        cond = (st.condition or "").strip()
        if not cond and (st.type == "condition" or st.condition):
            return None              # the host fails, or never runs, such a step
        if cond:
            when = lower_condition(cond, steps, i, names, int(input_words))
            if when is None:
                return None
        if st.type == "condition":
            specs.append(StepSpec(WFK_CONDITION, deps=deps, when=when))
            continue
        if st.type == "worker":
            policy = {}
            if step_policy:
                retry = lower_retry(st, tick_seconds)
                if retry is None:
                    return None
                timeout = 0
                if st.timeout_sec > 0:
                    timeout = max(int(timeout_cutoff),
                                  _ceil_ticks(st.timeout_sec, tick_seconds))
                    if timeout > 1 << 30:
                        return None
                policy = {"retry": retry, "timeout_ticks": timeout}
            if st.for_each:
                if items_len <= 0:
                    return None
                specs.append(StepSpec(WFK_FOR_EACH, deps=deps, fanout=int(items_len),
                                      max_parallel=int(st.max_parallel), when=when,
                                      **policy))
            else:
                specs.append(StepSpec(WFK_WORKER, deps=deps, when=when, **policy))
        elif st.type == "approval":
            specs.append(StepSpec(WFK_APPROVAL, deps=deps, ttl_ticks=ttl, when=when))
        elif st.type == "delay":
            ticks = int(math.ceil(st.delay_sec / tick_seconds))
            specs.append(StepSpec(WFK_DELAY, deps=deps, delay_ticks=max(0, ticks),
                                  when=when))
        else:
            return None
    return DagSpec(steps=specs, input_names=names)


class DeviceRunTable:
    """Run ids over a dynamic-mode `WorkflowPipeline`."""

    def __init__(self, pipe: WorkflowPipeline, store=None, clock=SYSTEM_CLOCK,
                 retain: int = 0):
        """`retain` > 0 keeps the final step states (and, on a pipeline with
        device_conditions, the output words) of that many most recently
        completed runs, so that rerun_from() can start from them."""
        if not getattr(pipe, "dynamic", False):
            raise RuntimeError("DeviceRunTable needs a dynamic-mode pipeline")
        if int(retain) < 0:
            raise ValueError("retain is a count of runs")
        self.pipe = pipe
        self.store = store                # a WorkflowStore, or None
        self._clock = clock
        self._events_on = getattr(pipe, "event_cap", None) is not None
        self._events: List[StepEvent] = []
        self._tmpl_of: Dict[str, int] = {}
        # template id -> (workflow id, step ids or None, step kinds)
        self._tmpl_info: Dict[int, Tuple[str, Optional[List[str]], List[int]]] = {}
        self._tmpl_ttl: Dict[int, List[int]] = {}    # template id -> hold ttl per step
        self._handle: Dict[str, Tuple[int, int]] = {}
        self._run_of: Dict[Tuple[int, int], str] = {}
        self._tmpl_inputs: Dict[int, List[str]] = {}  # template id -> input field names
        # run id -> (template, cond bits, fanout, input words): what a rerun
        # submits again
        self._req_of: Dict[str, Tuple[int, int, int, Tuple[int, ...]]] = {}
        # run id -> the steps it was admitted with as done, whose one
        # journal event each is still to come (and to be dropped)
        self._kept_of: Dict[str, int] = {}
        self._retain = int(retain)
        # run id -> (request, final step states, output words or None) of
        # the last `retain` completed runs, oldest first
        self._retained: "OrderedDict[str, Tuple[tuple, List[int], Optional[List[int]]]]" = \
            OrderedDict()
        self._tmpl_depmask: Dict[int, List[int]] = {}  # template id -> deps per step
        # (run id, template, cond bits, fanout, input words, (done, skipped)
        # step masks, {step: output word} of the done steps or None)
        self._queue: Deque[Tuple[str, int, int, int, Tuple[int, ...],
                                 Tuple[int, int], Optional[Dict[int, int]]]] = deque()
        self._queued_ids: set = set()     # run ids in _queue
        self._reported: List[Tuple[str, str]] = []  # queued runs cancelled

    def __len__(self) -> int:
        return len(self._handle) + len(self._queue)

    def queued(self) -> int:
        return len(self._queue)

    def handle(self, run_id: str) -> Optional[Tuple[int, int]]:
        return self._handle.get(run_id)

    def _known(self, run_id: str) -> bool:
        return run_id in self._handle or run_id in self._queued_ids

    def _admit(self, reqs) -> int:
        """Admit the requests in order; returns how many got a slot (the
        device accepts a prefix)."""
        extra = {}
        conditions = getattr(self.pipe, "device_conditions", False)
        if conditions:
            extra["inputs"] = [r[4] for r in reqs]
        if any(r[5][0] for r in reqs):      # a rerun among them
            extra["keep"] = [r[5] for r in reqs]
            if conditions:
                extra["outs"] = [r[6] for r in reqs]
        slots, gens = self.pipe.admit([r[1] for r in reqs],
                                      cond_bits=[r[2] for r in reqs],
                                      fanout=[r[3] for r in reqs], **extra)
        n = 0
        for r, slot, gen in zip(reqs, slots, gens):
            if slot == -2:
                # rerun_from() keeps a closed set of the template's steps
                raise RuntimeError(f"the device refused the kept steps of run {r[0]!r}")
            if slot < 0:
                break
            self._handle[r[0]] = (slot, gen)
            self._run_of[(slot, gen)] = r[0]
            self._tmpl_of[r[0]] = r[1]
            self._req_of[r[0]] = r[1:5]
            if r[5][0]:
                self._kept_of[r[0]] = r[5][0]
            n += 1
        return n

    def register(self, workflow: Any, items_len: int = 0,
                 tick_seconds: float = 1.0,
                 approval_ttl_sec: float = 0.0) -> Optional[int]:
        """Lower `workflow` and add it as a template; returns the template id
        to submit() runs of it with, or None if the workflow must stay on the
        host engine. Events of such runs carry the workflow's step ids. On a
        pipeline with step_policy the steps' `retry` blocks and `timeout_sec`
        are lowered too, on one with device_conditions the `condition`
        expressions (see `dag_from_workflow`)."""
        dag = dag_from_workflow(
            workflow, items_len, tick_seconds, approval_ttl_sec,
            step_policy=bool(getattr(self.pipe, "step_policy", False)),
            timeout_cutoff=int(getattr(self.pipe, "timeout_cutoff", 8)),
            conditions=bool(getattr(self.pipe, "device_conditions", False)),
            input_words=int(getattr(self.pipe, "input_words", 8)))
        if dag is None:
            return None
        t = self.pipe.add_template(dag)
        self._tmpl_inputs[t] = list(dag.input_names)
        wf_id = getattr(workflow, "id", None)
        if wf_id is None and isinstance(workflow, dict):
            wf_id = workflow.get("id", "")
        self._tmpl_info[t] = (str(wf_id or ""), [st.id for st in _steps_of(workflow)],
                              [sp.kind for sp in dag.steps])
        return t

    def _info(self, template_id: int):
        info = self._tmpl_info.get(template_id)
        if info is None:    # added to the pipe directly: kinds from the device
            row = self.pipe.tmpl_kind[template_id * 64:template_id * 64 + 64]
            n = int(self.pipe.tmpl_nsteps[template_id])
            info = self._tmpl_info[template_id] = ("", None, row.cpu().tolist()[:n])
        return info

    def _input_words(self, template_id: int, input: Optional[Dict[str, Any]]):
        """The run's input dict as the template's input words."""
        words = []
        for name in self._tmpl_inputs.get(template_id, ()):
            v = (input or {}).get(name)
            if isinstance(v, bool) or not isinstance(v, int) \
                    or not -(1 << 31) <= v < (1 << 31):
                raise ValueError(f"input field {name!r} must be an int in int32 "
                                 f"range for the device to decide on it, got {v!r}")
            words.append(v)
        return tuple(words)

    def submit(self, run_id: str, template_id: int, cond_bits: int = 0,
               fanout: int = 0, input: Optional[Dict[str, Any]] = None) -> bool:
        """Start a run. Returns True if it was admitted now, False if the
        table was full and it waits (FIFO) for the next poll(). `input` is the
        run's input: the fields the template's conditions name go to the
        device as input words. A named field that is missing, not an int, a
        bool or outside int32 raises ValueError; such a run stays on the host
        engine."""
        if self._known(run_id):
            raise ValueError(f"run {run_id!r} is already live or queued")
        if not 0 <= int(template_id) < self.pipe.n_templates:
            raise ValueError(f"unregistered template id {template_id}")
        if not 0 <= int(fanout) <= self.pipe.CB:
            raise ValueError(f"fanout {fanout} can never be emitted")
        return self._submit((run_id, int(template_id), int(cond_bits), int(fanout),
                             self._input_words(int(template_id), input), (0, 0), None))

    def _submit(self, req) -> bool:
        # nobody overtakes a waiting submission
        if not self._queue and self._admit([req]) == 1:
            return True
        self._queue.append(req)
        self._queued_ids.add(req[0])
        return False

    def _deps_of(self, template_id: int) -> List[int]:
        """The dependency mask of every step of a template, as the device
        holds it."""
        deps = self._tmpl_depmask.get(template_id)
        if deps is None:
            row = self.pipe.tmpl_deps[template_id * 64:template_id * 64 + 64]
            deps = self._tmpl_depmask[template_id] = \
                [d & ((1 << 64) - 1) for d in row.cpu().tolist()]
        return deps

    def _source(self, run_id: str):
        """(request, step states, output words or None) of the run a rerun
        starts from: a resident run as the device holds it now, then a
        retained record, then a queued run, which has finished nothing."""
        conditions = getattr(self.pipe, "device_conditions", False)
        h = self._handle.get(run_id)
        if h is not None:
            row = slice(h[0] * 64, h[0] * 64 + 64)
            return (self._req_of[run_id], self.pipe.step_state[row].cpu().tolist(),
                    self.pipe.step_out[row].cpu().tolist() if conditions else None)
        if run_id in self._retained:
            return self._retained[run_id]
        for q in self._queue:
            if q[0] == run_id:
                return q[1:5], [WFS_PENDING] * 64, [0] * 64 if conditions else None
        raise KeyError(run_id)

    def rerun_from(self, run_id: str, step: Union[str, int] = "",
                   new_run_id: Optional[str] = None) -> str:
        """Start a new run of `run_id`'s workflow with the same input, as the
        host engine's rerun_from does; returns its id (`new_run_id`, or a
        fresh one). With `step` (a step id or index) every transitive
        dependency of that step, never the step itself, starts as finished,
        in the state and with the output word it has in the source run; with
        step "" nothing is kept. The source is a run in the table, one of the
        `retain` last completed ones, or a queued one (KeyError otherwise).
        ValueError "run id required", "step not found" and "dependency X not
        succeeded" as the host engine raises them; a dependency counts as
        succeeded if it is SUCCEEDED or SKIPPED (a false condition) on the
        device. If the table is full the rerun waits in the submissions'
        FIFO. With a store that holds the source run, the new run's record
        is created with the host engine's rerun fields."""
        from ..utils.ids import new_id

        if not run_id:
            raise ValueError("run id required")
        req, states, outs = self._source(run_id)
        tmpl = req[0]
        done = skipped = 0
        if step != "":
            s = self._step_index(tmpl, step)
            deps = self._deps_of(tmpl)
            todo = deps[s]
            while todo:                 # the transitive dependencies of s
                d = todo.bit_length() - 1
                todo &= ~(1 << d)
                if not done >> d & 1:
                    done |= 1 << d
                    todo |= deps[d] & ~done
        ids = self._info(tmpl)[1]
        for d in range(64):
            if done >> d & 1:
                if states[d] == WFS_SKIPPED:
                    skipped |= 1 << d
                elif states[d] != WFS_SUCCEEDED:
                    raise ValueError(
                        f"dependency {ids[d] if ids else d} not succeeded")
        new = new_id() if new_run_id is None else new_run_id
        if self._known(new):
            raise ValueError(f"run {new!r} is already live or queued")
        words = None if outs is None else {d: outs[d] for d in range(64) if done >> d & 1}
        if self.store is not None:
            self._store_rerun(run_id, step, new, ids, done)
        self._submit((new,) + tuple(req) + ((done, skipped), words))
        return new

    def _store_rerun(self, run_id: str, step: Union[str, int], new: str,
                     ids: Optional[List[str]], done: int) -> None:
        from .engine import rerun_record

        run = self._stored_run(run_id)
        if run is None:
            return
        step_id = step if isinstance(step, str) else (ids[step] if ids else "")
        deps = {ids[d] for d in range(64) if done >> d & 1} if ids else set()
        self.store.create_run(rerun_record(run, step_id, deps, new, self._clock.now(),
                                           require_succeeded=False))

    def cancel(self, run_id: str) -> bool:
        """Cancel a run. A still-queued submission is dropped without
        touching the device; either way the run is reported RUN_CANCELLED by
        a later poll(). False: unknown run, or already terminal."""
        for q in self._queue:
            if q[0] == run_id:
                self._queue.remove(q)
                self._queued_ids.discard(run_id)
                self._reported.append((run_id, RUN_CANCELLED))
                if self.store is not None:
                    self._store_completion(run_id, RUN_CANCELLED, self._info(q[1])[0])
                return True
        h = self._handle.get(run_id)
        if h is None:
            return False
        return bool(self.pipe.cancel([h[0]], [h[1]])[0])

    # ---- approval gates (pipeline with approvals="external") -----------------
    def _ttl_of(self, template_id: int) -> List[int]:
        ttl = self._tmpl_ttl.get(template_id)
        if ttl is None:
            row = self.pipe.tmpl_ttl[template_id * 64:template_id * 64 + 64]
            ttl = self._tmpl_ttl[template_id] = row.cpu().tolist()
        return ttl

    def approvals(self) -> List[PendingApproval]:
        """The approval holds that wait for a decision, of the runs this
        table knows, ascending in (slot, step)."""
        out = []
        for slot, gen, step, since in zip(*self.pipe.open_holds()):
            run_id = self._run_of.get((slot, gen))
            if run_id is None:
                continue
            tmpl = self._tmpl_of[run_id]
            ids = self._info(tmpl)[1]
            ttl = self._ttl_of(tmpl)[step]
            out.append(PendingApproval(
                run_id, step, ids[step] if ids is not None and step < len(ids) else "",
                since, since + ttl if ttl > 0 else None))
        return out

    def _step_index(self, template_id: int, step: Union[str, int]) -> int:
        _, ids, kinds = self._info(template_id)
        if isinstance(step, str):
            if ids is None or step not in ids:
                raise ValueError("step not found")
            return ids.index(step)
        if not 0 <= int(step) < len(kinds):
            raise ValueError("step not found")
        return int(step)

    def _decide(self, run_id: str, step: Union[str, int], verdict: int) -> None:
        h = self._handle.get(run_id)
        if h is None:
            for q in self._queue:
                if q[0] == run_id:        # not admitted yet: nothing waits
                    self._step_index(q[1], step)
                    raise ValueError("step not waiting")
            raise KeyError(run_id)
        s = self._step_index(self._tmpl_of[run_id], step)
        if self.pipe.decide([h[0]], [h[1]], [s], [verdict])[0] != 0:
            raise ValueError("step not waiting")

    def approve(self, run_id: str, step: Union[str, int]) -> None:
        """Approve a waiting approval step, named by step id or index. As the
        host engine's approve_step: KeyError for an unknown run, ValueError
        "step not found" / "step not waiting" otherwise. The run goes on in
        the next tick."""
        self._decide(run_id, step, 1)

    def reject(self, run_id: str, step: Union[str, int]) -> None:
        """Reject a waiting approval step: the step fails, and the run with
        it, in the next tick. Errors as approve()."""
        self._decide(run_id, step, 0)

    def _drain_events(self) -> None:
        """Journal records -> StepEvents (and the store). Records of a (slot,
        gen) this table does not know are dropped."""
        slots, gens, steps, frm, to, stamps = self.pipe.drain_events()
        for slot, gen, step, f, t, stamp in zip(slots, gens, steps, frm, to, stamps):
            run_id = self._run_of.get((slot, gen))
            if run_id is None:
                continue
            kept = self._kept_of.get(run_id, 0)
            if kept >> step & 1 and f == WFS_PENDING and t in (WFS_SUCCEEDED, WFS_SKIPPED):
                # a step the rerun was admitted with as done: the journal sees
                # it once, as finishing in the run's first pass. Nothing ran.
                self._kept_of[run_id] = kept & ~(1 << step)
                continue
            wf_id, ids, kinds = self._info(self._tmpl_of[run_id])
            step_id = ids[step] if ids is not None and step < len(ids) else ""
            ev = StepEvent(run_id, step, step_id, f, t, stamp >> 1, bool(stamp & 1))
            self._events.append(ev)
            if self.store is not None:
                kind = kinds[step] if step < len(kinds) else WFK_WORKER
                self._store_event(ev, wf_id, kind)

    def _stored_run(self, run_id: str):
        try:
            return self.store.get_run(run_id)
        except KeyError:                  # RunNotFound: not the store's run
            return None

    def _store_event(self, ev: StepEvent, wf_id: str, kind: int) -> None:
        run = self._stored_run(ev.run_id)
        if run is None:
            return
        etype, status, extra = timeline_of(kind, ev.to_state)
        data = {"tick": ev.tick}
        data.update(extra)
        self.store.append_timeline(ev.run_id, TimelineEvent(
            time=self._clock.now(), type=etype, run_id=ev.run_id,
            workflow_id=wf_id or run.workflow_id, step_id=ev.step_id,
            status=status, data=data))
        if ev.step_id:
            sr = run.steps.get(ev.step_id)
            if sr is None:
                sr = run.steps[ev.step_id] = StepRun(step_id=ev.step_id)
            sr.status = status
            self.store.update_run(run)

    def _store_completion(self, run_id: str, status: str, wf_id: str) -> None:
        run = self._stored_run(run_id)
        if run is None:
            return
        run.status = status
        run.completed_at = self._clock.now()
        self.store.update_run(run)
        self.store.append_timeline(run_id, TimelineEvent(
            time=self._clock.now(), type="run_status", run_id=run_id,
            workflow_id=wf_id or run.workflow_id, status=status))

    def take_events(self) -> List[StepEvent]:
        """The step events the polls gathered since the last call, in time
        order per run."""
        out, self._events = self._events, []
        return out

    def step_states(self, run_id: str) -> Dict[Union[str, int], str]:
        """Current `STEP_*` status per step of an admitted or queued run, by
        step id (by step index for a template added without register())."""
        h = self._handle.get(run_id)
        if h is None:
            for q in self._queue:
                if q[0] == run_id:
                    _, ids, kinds = self._info(q[1])
                    return {(ids[s] if ids else s): STEP_PENDING
                            for s in range(len(kinds))}
            raise KeyError(run_id)
        _, ids, kinds = self._info(self._tmpl_of[run_id])
        row = self.pipe.step_state[h[0] * 64:h[0] * 64 + len(kinds)].cpu().tolist()
        return {(ids[s] if ids else s): _STEP_STATUS[v] for s, v in enumerate(row)}

    def step_outputs(self, run_id: str) -> Dict[Union[str, int], int]:
        """The output word of every step of an admitted run, by step id (by
        step index for a template added without register()): a worker or
        for_each step's is the wraparound sum of its succeeded children's
        result words, a condition step's 1 or 0, anything else 0."""
        if not getattr(self.pipe, "device_conditions", False):
            raise RuntimeError("step_outputs needs a pipeline with device_conditions")
        h = self._handle.get(run_id)
        if h is None:
            raise KeyError(run_id)
        _, ids, kinds = self._info(self._tmpl_of[run_id])
        row = self.pipe.step_out[h[0] * 64:h[0] * 64 + len(kinds)].cpu().tolist()
        return {(ids[s] if ids else s): v for s, v in enumerate(row)}

    def poll(self) -> List[Tuple[str, str]]:
        """Drain the device's step events (journal on), then its completion
        records, then admit what is queued. Returns (run_id, status) for
        every run that ended since the last poll, each exactly once; a run's
        events are all gathered before its completion is returned."""
        out, self._reported = self._reported, []
        if self._events_on:
            # before drain_completed(): a run's last events still find its
            # handle, and its slot cannot be released with changes unseen
            self._drain_events()
        slots, gens, states = self.pipe.drain_completed()
        ended: List[Tuple[int, str, tuple]] = []
        for slot, gen, state in zip(slots, gens, states):
            run_id = self._run_of.pop((slot, gen), None)
            if run_id is None:
                continue
            del self._handle[run_id]
            tmpl = self._tmpl_of.pop(run_id)
            ended.append((slot, run_id, self._req_of.pop(run_id)))
            self._kept_of.pop(run_id, None)
            out.append((run_id, _STATUS[state]))
            if self.store is not None:
                self._store_completion(run_id, _STATUS[state], self._info(tmpl)[0])
        if self._retain and ended:
            # before the admissions below: a reported row, DRAINING or freed
            # just now, keeps its content until the next admission takes it
            self._retain_rows(ended)
        if self._queue:
            reqs = list(self._queue)
            for _ in range(self._admit(reqs)):
                self._queued_ids.discard(self._queue.popleft()[0])
        return out

    def _retain_rows(self, ended) -> None:
        """Remember the rows of the runs that just ended: one indexed load of
        their step states (and output words) and one D2H."""
        import torch

        idx = torch.tensor([e[0] for e in ended], dtype=torch.int64).to(self.pipe.device)
        rows = self.pipe.step_state.view(-1, 64)[idx]
        conditions = getattr(self.pipe, "device_conditions", False)
        if conditions:
            rows = torch.cat([rows.to(torch.int32), self.pipe.step_out.view(-1, 64)[idx]], 1)
        rows = rows.cpu().tolist()
        for (_, run_id, req), row in zip(ended, rows):
            self._retained[run_id] = (req, row[:64], row[64:] if conditions else None)
            self._retained.move_to_end(run_id)
        while len(self._retained) > self._retain:
            self._retained.popitem(last=False)

    def tick(self) -> None:
        self.pipe.tick()
