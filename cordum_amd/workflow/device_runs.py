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

Wiring an API route to this table, and result / output materialisation, are
not done here.
"""
from __future__ import annotations

import math
from collections import deque
from typing import Any, Deque, Dict, List, NamedTuple, Optional, Tuple, Union

from ..ops.reference import wf_backoff_ref
from ..ops.wf_pipeline import (
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


def dag_from_workflow(workflow: Any, items_len: int,
                      tick_seconds: float = 1.0,
                      approval_ttl_sec: float = 0.0,
                      step_policy: bool = False,
                      timeout_cutoff: int = 8) -> Optional[DagSpec]:
    """Lower a workflow (a `Workflow`, or its `{"steps": {id: step}}` dict
    form) to a device `DagSpec`; steps are indexed in `workflow.steps` order.
    Returns None when the workflow cannot run on the device, and the caller
    stays on the host engine: more than 64 steps, a step type other than
    worker / approval / delay, a `condition` expression, `delay_until`,
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
    on approval and delay steps mean nothing to either engine."""
    steps = _steps_of(workflow)
    ttl = max(0, int(math.ceil(approval_ttl_sec / tick_seconds)))
    if len(steps) > 64:
        return None
    index = {st.id: i for i, st in enumerate(steps)}
    if len(index) != len(steps):
        return None
    specs: List[StepSpec] = []
    for i, st in enumerate(steps):
        if st.condition or st.delay_until or st.on_error:
            return None
        if st.retry is not None and not step_policy:
            return None
        deps = []
        for dep in st.depends_on:
            j = index.get(dep)
            if j is None or j >= i:
                return None
            deps.append(j)
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
                                      max_parallel=int(st.max_parallel), **policy))
            else:
                specs.append(StepSpec(WFK_WORKER, deps=deps, **policy))
        elif st.type == "approval":
            specs.append(StepSpec(WFK_APPROVAL, deps=deps, ttl_ticks=ttl))
        elif st.type == "delay":
            ticks = int(math.ceil(st.delay_sec / tick_seconds))
            specs.append(StepSpec(WFK_DELAY, deps=deps, delay_ticks=max(0, ticks)))
        else:
            return None
    return DagSpec(steps=specs)


class DeviceRunTable:
    """Run ids over a dynamic-mode `WorkflowPipeline`."""

    def __init__(self, pipe: WorkflowPipeline, store=None, clock=SYSTEM_CLOCK):
        if not getattr(pipe, "dynamic", False):
            raise RuntimeError("DeviceRunTable needs a dynamic-mode pipeline")
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
        self._queue: Deque[Tuple[str, int, int, int]] = deque()
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
        slots, gens = self.pipe.admit([r[1] for r in reqs],
                                      cond_bits=[r[2] for r in reqs],
                                      fanout=[r[3] for r in reqs])
        n = 0
        for r, slot, gen in zip(reqs, slots, gens):
            if slot < 0:
                break
            self._handle[r[0]] = (slot, gen)
            self._run_of[(slot, gen)] = r[0]
            self._tmpl_of[r[0]] = r[1]
            n += 1
        return n

    def register(self, workflow: Any, items_len: int = 0,
                 tick_seconds: float = 1.0,
                 approval_ttl_sec: float = 0.0) -> Optional[int]:
        """Lower `workflow` and add it as a template; returns the template id
        to submit() runs of it with, or None if the workflow must stay on the
        host engine. Events of such runs carry the workflow's step ids. On a
        pipeline with step_policy the steps' `retry` blocks and `timeout_sec`
        are lowered too (see `dag_from_workflow`)."""
        dag = dag_from_workflow(
            workflow, items_len, tick_seconds, approval_ttl_sec,
            step_policy=bool(getattr(self.pipe, "step_policy", False)),
            timeout_cutoff=int(getattr(self.pipe, "timeout_cutoff", 8)))
        if dag is None:
            return None
        t = self.pipe.add_template(dag)
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

    def submit(self, run_id: str, template_id: int, cond_bits: int = 0,
               fanout: int = 0) -> bool:
        """Start a run. Returns True if it was admitted now, False if the
        table was full and it waits (FIFO) for the next poll()."""
        if self._known(run_id):
            raise ValueError(f"run {run_id!r} is already live or queued")
        if not 0 <= int(template_id) < self.pipe.n_templates:
            raise ValueError(f"unregistered template id {template_id}")
        if not 0 <= int(fanout) <= self.pipe.CB:
            raise ValueError(f"fanout {fanout} can never be emitted")
        req = (run_id, int(template_id), int(cond_bits), int(fanout))
        # nobody overtakes a waiting submission
        if not self._queue and self._admit([req]) == 1:
            return True
        self._queue.append(req)
        self._queued_ids.add(run_id)
        return False

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
        for slot, gen, state in zip(slots, gens, states):
            run_id = self._run_of.pop((slot, gen), None)
            if run_id is None:
                continue
            del self._handle[run_id]
            tmpl = self._tmpl_of.pop(run_id)
            out.append((run_id, _STATUS[state]))
            if self.store is not None:
                self._store_completion(run_id, _STATUS[state], self._info(tmpl)[0])
        if self._queue:
            reqs = list(self._queue)
            for _ in range(self._admit(reqs)):
                self._queued_ids.discard(self._queue.popleft()[0])
        return out

    def tick(self) -> None:
        self.pipe.tick()
