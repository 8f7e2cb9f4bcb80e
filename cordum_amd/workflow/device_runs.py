"""Host run table over the device workflow engine's run lifecycle.

`WorkflowPipeline` in dynamic mode (ops/wf_pipeline.py) speaks slots and
generations; the serving layer speaks run ids and `RUN_*` status strings
(workflow/models.py). `DeviceRunTable` is the map between the two: it admits
submissions (queueing them FIFO while the device table is full), cancels by
run id, and turns the device's completion records into `(run_id, status)`
pairs. `dag_from_workflow` lowers a `Workflow` to the `DagSpec` the device
runs, or says (None) that the workflow must stay on the host engine.

Wiring an API route to this table, and result / timeline / output
materialisation, are not done here.
"""
from __future__ import annotations

import math
from collections import deque
from typing import Any, Deque, Dict, List, Optional, Tuple

from ..ops.wf_pipeline import (
    DagSpec,
    StepSpec,
    WFK_APPROVAL,
    WFK_DELAY,
    WFK_FOR_EACH,
    WFK_WORKER,
    WFS_CANCELLED,
    WFS_FAILED,
    WFS_SUCCEEDED,
    WorkflowPipeline,
)
from .models import RUN_CANCELLED, RUN_FAILED, RUN_SUCCEEDED, Step

_STATUS = {
    WFS_SUCCEEDED: RUN_SUCCEEDED,
    WFS_FAILED: RUN_FAILED,
    WFS_CANCELLED: RUN_CANCELLED,
}


def _steps_of(workflow: Any) -> List[Step]:
    steps = getattr(workflow, "steps", None)
    if steps is None:
        steps = workflow.get("steps", workflow)
    out = []
    for sid, st in steps.items():
        out.append(st if isinstance(st, Step) else Step.from_dict(sid, st))
    return out


def dag_from_workflow(workflow: Any, items_len: int,
                      tick_seconds: float = 1.0) -> Optional[DagSpec]:
    """Lower a workflow (a `Workflow`, or its `{"steps": {id: step}}` dict
    form) to a device `DagSpec`; steps are indexed in `workflow.steps` order.
    Returns None when the workflow cannot run on the device, and the caller
    stays on the host engine: more than 64 steps, a step type other than
    worker / approval / delay, a `condition` expression, `delay_until`,
    `on_error`, a per-step `retry` block, a dependency on a later or unknown
    step, or a `for_each` over no items (the device cannot complete a step
    with nothing to emit)."""
    steps = _steps_of(workflow)
    if len(steps) > 64:
        return None
    index = {st.id: i for i, st in enumerate(steps)}
    if len(index) != len(steps):
        return None
    specs: List[StepSpec] = []
    for i, st in enumerate(steps):
        if st.condition or st.delay_until or st.on_error or st.retry is not None:
            return None
        deps = []
        for dep in st.depends_on:
            j = index.get(dep)
            if j is None or j >= i:
                return None
            deps.append(j)
        if st.type == "worker":
            if st.for_each:
                if items_len <= 0:
                    return None
                specs.append(StepSpec(WFK_FOR_EACH, deps=deps, fanout=int(items_len),
                                      max_parallel=int(st.max_parallel)))
            else:
                specs.append(StepSpec(WFK_WORKER, deps=deps))
        elif st.type == "approval":
            specs.append(StepSpec(WFK_APPROVAL, deps=deps))
        elif st.type == "delay":
            ticks = int(math.ceil(st.delay_sec / tick_seconds))
            specs.append(StepSpec(WFK_DELAY, deps=deps, delay_ticks=max(0, ticks)))
        else:
            return None
    return DagSpec(steps=specs)


class DeviceRunTable:
    """Run ids over a dynamic-mode `WorkflowPipeline`."""

    def __init__(self, pipe: WorkflowPipeline):
        if not getattr(pipe, "dynamic", False):
            raise RuntimeError("DeviceRunTable needs a dynamic-mode pipeline")
        self.pipe = pipe
        self._handle: Dict[str, Tuple[int, int]] = {}
        self._run_of: Dict[Tuple[int, int], str] = {}
        self._queue: Deque[Tuple[str, int, int, int]] = deque()
        self._reported: List[Tuple[str, str]] = []  # queued runs cancelled

    def __len__(self) -> int:
        return len(self._handle) + len(self._queue)

    def queued(self) -> int:
        return len(self._queue)

    def handle(self, run_id: str) -> Optional[Tuple[int, int]]:
        return self._handle.get(run_id)

    def _known(self, run_id: str) -> bool:
        return run_id in self._handle or any(q[0] == run_id for q in self._queue)

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
            n += 1
        return n

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
        return False

    def cancel(self, run_id: str) -> bool:
        """Cancel a run. A still-queued submission is dropped without
        touching the device; either way the run is reported RUN_CANCELLED by
        a later poll(). False: unknown run, or already terminal."""
        for q in self._queue:
            if q[0] == run_id:
                self._queue.remove(q)
                self._reported.append((run_id, RUN_CANCELLED))
                return True
        h = self._handle.get(run_id)
        if h is None:
            return False
        return bool(self.pipe.cancel([h[0]], [h[1]])[0])

    def poll(self) -> List[Tuple[str, str]]:
        """Drain the device's completion records, then admit what is queued.
        Returns (run_id, status) for every run that ended since the last
        poll, each exactly once."""
        out, self._reported = self._reported, []
        slots, gens, states = self.pipe.drain_completed()
        for slot, gen, state in zip(slots, gens, states):
            run_id = self._run_of.pop((slot, gen), None)
            if run_id is None:
                continue
            del self._handle[run_id]
            out.append((run_id, _STATUS[state]))
        if self._queue:
            reqs = list(self._queue)
            for _ in range(self._admit(reqs)):
                self._queue.popleft()
        return out

    def tick(self) -> None:
        self.pipe.tick()
