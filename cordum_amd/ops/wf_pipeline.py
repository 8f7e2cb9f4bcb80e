"""Device-resident workflow engine tick (config #3: 1->256 fan-out +
approval gate over 8 pools, RCCL all-to-all over xGMI).

This is the batched HBM counterpart of the host workflow engine
(cordum_amd/workflow/engine.py; semantics oracle core/workflow/engine.go
:453-827 scheduleReady, :1524-1560 applyResult, :1623-1645
aggregateChildren, :1647-1699 updateRunStatus). Run/step state lives in
per-rank HBM tables; each tick is a fixed kernel sequence:

  wf_sweep    readiness gates (deps, backoff, delay), approval holds,
              condition commits          -> dispatch list of (run, step)
  wf_expand   for_each/worker expansion  -> child-job arena (all-or-nothing
              reservation; arena-full steps retry next sweep)
  K2 routing  children spread over the least-loaded global worker order,
              packed per destination rank (pack_requeue + pack_by_dest with
              the NAK requeue ring), payload gathered from the child arena
  exchange    all_to_all_single over RCCL/xGMI (world > 1)
  echo        device worker pools execute on the receiving rank
  wf_apply    owner-rank result application with deterministic failure
              injection (retry waves), dead-letter application for
              max-deliver drops
  wf_commit   child aggregation, retry + exponential tick backoff, FAILED
              after max_retries
  wf_status   run roll-up -> SUCCEEDED/FAILED counts
  host hop    fresh approval holds drained D2H; the approver (the admin
              analog, gateway.go:3553) grants them next tick H2D

Step kinds: WORKER (one child job), FOR_EACH (fanout children, per-child
retry), APPROVAL (host-granted), CONDITION (pre-evaluated bit ->
SUCCEEDED/SKIPPED), DELAY (tick gate). Dependencies are 64-bit step masks;
SKIPPED satisfies a dependency, FAILED permanently blocks (the run fails).

Static mode (the default) creates every run at construction and re-enters
them by reset_runs() / wf_readmit. Dynamic mode (`dynamic_capacity=NR`)
starts with NR FREE slots and gives runs a lifecycle between ticks:
admit() (wf_admit, lowest free slots, templates held on the device),
cancel() (wf_cancel, checked against the slot's generation) and
drain_completed() (wf_retire: completion records, and release of slots
whose rows are quiescent). The tick body is the same in both modes.

With `event_cap=N` dynamic mode also keeps a step-transition journal: one
more kernel (wf_journal) ends the tick and appends a record per step whose
state changed since it last looked, and drain_events() returns them (see
"step-transition journal" below). Without it nothing is allocated and the
tick launches exactly the sequence above.

With `approvals="external"` dynamic mode serves approval gates per run: the
host hop above is gone, a hold stays WAITING until decide() names it by
(slot, gen, step), open_holds() lists what is waiting and a step's
`ttl_ticks` lets a hold expire (see "externally decided approvals" below).
One more kernel (wf_hold_scan) follows the sweep. With the default
`approvals="auto"` nothing is allocated and the tick is unchanged.

With `step_policy=True` dynamic mode takes retry, backoff and timeout per
step (`StepSpec.retry`, `StepSpec.timeout_ticks`) instead of per pipeline:
one kernel (wf_settle) stands in for the pair wf_timeout_scan + wf_commit and
reads each step's constants from its template (see "per-step policy" below).
With the default `step_policy=False` nothing is allocated and the tick is
unchanged.

With `device_conditions=True` dynamic mode decides conditions on the device
from data the run produces: a step may carry a predicate (`StepSpec.when`)
over the run's input words and the output words of steps it depends on. Three
kernels join the tick: wf_cond_eval before the sweep, wf_child_payload after
wf_expand, and wf_apply_out in place of wf_apply (see "conditions decided on
the device" below). With the default nothing is allocated and the tick is
unchanged.
"""
from __future__ import annotations

import os
import sys
import time
from dataclasses import dataclass, field
from typing import List, NamedTuple, Optional, Sequence

import torch
import torch.distributed as dist

from . import get_ext
from .pipeline import _RefOps

WFS_PENDING, WFS_DISPATCHED, WFS_WAITING = 0, 1, 2
WFS_SUCCEEDED, WFS_FAILED, WFS_SKIPPED = 3, 4, 5
WFS_CANCELLED = 6            # dynamic mode: cancelled run / step
WFL_FREE, WFL_LIVE, WFL_DRAINING = 0, 1, 2   # life of a run slot
WFK_WORKER, WFK_FOR_EACH, WFK_APPROVAL, WFK_CONDITION, WFK_DELAY = 0, 1, 2, 3, 4


@dataclass
class RetrySpec:
    """Retry policy of one step (pipeline with step_policy): after failure k
    (k = 1 .. max_retries) the step waits backoff_ticks * (multiplier_q8 /
    256)^(k-1) ticks, rounded up and capped at cap_ticks (0 = no cap; the
    delay then saturates at 2^20 ticks). The defaults are the constants of a
    pipeline without step_policy: 2, 4, 8, 16, 16, ..."""
    max_retries: int
    backoff_ticks: int = 2
    multiplier_q8: int = 512
    cap_ticks: int = 16


WFC_EQ, WFC_NE, WFC_LT, WFC_LE, WFC_GT, WFC_GE, WFC_TRUTHY = 1, 2, 3, 4, 5, 6, 7
_WFC_OPS = {"==": WFC_EQ, "!=": WFC_NE, "<": WFC_LT, "<=": WFC_LE, ">": WFC_GT,
            ">=": WFC_GE, "truthy": WFC_TRUTHY}
_I32_MIN, _I32_MAX = -(1 << 31), (1 << 31) - 1


@dataclass
class CondSpec:
    """Predicate of one step (pipeline with device_conditions): `lhs op rhs`,
    signed 32-bit. `op` is one of WFC_EQ .. WFC_TRUTHY (or "==", "!=", "<",
    "<=", ">", ">=", "truthy"); TRUTHY is `lhs != 0` and ignores rhs. An
    operand is ("input", k) for input word k of the run, ("out", j) for the
    output word of step j, or (rhs only) an int immediate."""
    op: object
    lhs: tuple
    rhs: object = 0
    negate: bool = False


@dataclass
class StepSpec:
    kind: int
    deps: Sequence[int] = ()
    fanout: int = 1          # children for FOR_EACH (WORKER always 1)
    delay_ticks: int = 0     # DELAY gate
    cond: bool = True        # CONDITION value (pre-evaluated)
    max_parallel: int = 0    # for_each window (0 = unlimited)
    ttl_ticks: int = 0       # APPROVAL hold expiry (0 = never; external approvals)
    # step_policy pipelines: None = the pipeline's max_retries with the stock
    # backoff; 0 = the pipeline's timeout_cutoff
    retry: Optional[RetrySpec] = None
    timeout_ticks: int = 0   # ticks until lost children are written off
    # device_conditions pipelines: on a CONDITION step the predicate decides
    # the step (`cond` is then ignored); on any other step it is a guard, and
    # the step is SKIPPED without running when it is false
    when: Optional[CondSpec] = None


@dataclass
class DagSpec:
    """One workflow DAG (<= 64 steps)."""
    steps: List[StepSpec] = field(default_factory=list)
    # set by the lowering of a workflow with conditions: the run-input field
    # names, in the order of the input words they were given
    input_names: List[str] = field(default_factory=list)

    @classmethod
    def fanout_approval(cls, fanout: int = 256) -> "DagSpec":
        """Config #3 shape: seed -> 1->N fan-out -> approval gate -> final."""
        return cls(steps=[
            StepSpec(WFK_WORKER),
            StepSpec(WFK_FOR_EACH, deps=[0], fanout=fanout),
            StepSpec(WFK_APPROVAL, deps=[1]),
            StepSpec(WFK_WORKER, deps=[2]),
        ])


@dataclass
class WfStats:
    runs_succeeded: int = 0
    runs_failed: int = 0
    ticks: int = 0
    wall_s: float = 0.0


def _i64(mask: int) -> int:
    """A 64-bit mask as the signed value an int64 tensor holds."""
    return mask - (1 << 64) if mask >= (1 << 63) else mask


class _StepRows(NamedTuple):
    """One DAG lowered to the 64-wide host rows of the run / template tables."""
    kind: torch.Tensor       # uint8
    deps: torch.Tensor       # int64 step masks
    todo: torch.Tensor       # int32 children to emit
    maxp: torch.Tensor       # int32 for_each window
    delay: torch.Tensor      # int32 DELAY gate
    cond: int                # pre-evaluated CONDITION bits, signed
    n_steps: int
    children: int            # children of one run


def _lower_steps(dag: DagSpec) -> _StepRows:
    if len(dag.steps) > 64:
        raise ValueError("device DAGs cap at 64 steps")
    kind, deps, todo, maxp, delay = ([0] * 64 for _ in range(5))
    cbits = 0
    for s, spec in enumerate(dag.steps):
        kind[s] = spec.kind
        m = 0
        for d in spec.deps:
            m |= 1 << d
        deps[s] = _i64(m)
        if spec.kind == WFK_FOR_EACH:
            todo[s] = spec.fanout
        elif spec.kind == WFK_WORKER:
            todo[s] = 1
        if spec.kind == WFK_DELAY:
            delay[s] = spec.delay_ticks
        maxp[s] = spec.max_parallel
        if spec.cond:
            cbits |= 1 << s
    i32 = torch.int32
    return _StepRows(torch.tensor(kind, dtype=torch.uint8),
                     torch.tensor(deps, dtype=torch.int64), torch.tensor(todo, dtype=i32),
                     torch.tensor(maxp, dtype=i32), torch.tensor(delay, dtype=i32),
                     _i64(cbits), len(dag.steps), sum(todo))


class WorkflowPipeline:
    """Per-rank device workflow engine over a set of runs (same or mixed
    DAGs). World > 1 exchanges children over the padded all-to-all."""

    def __init__(
        self,
        device: torch.device,
        dags: Sequence[DagSpec],
        n_local_workers: int = 256,
        payload_words: int = 64,
        world_size: int = 1,
        rank: int = 0,
        backend: str = "ext",
        fail_ppt: int = 0,
        drop_ppt: int = 0,
        max_retries: int = 2,
        # must exceed the max requeue-ring lifetime (RQ_MAX_DELIVER + 1
        # ticks) so a parked-but-live child is never declared lost — a
        # timeout firing on a child that later applies would double-account
        timeout_cutoff: int = 8,
        approval_verdict: int = 1,
        child_cap: Optional[int] = None,
        pad_cap: Optional[int] = None,
        replicate: Optional[int] = None,
        seed: int = 7,
        # dynamic mode: `dags` are templates, the table has this many run
        # slots, all FREE; runs enter through admit() (see "run lifecycle")
        dynamic_capacity: Optional[int] = None,
        template_cap: int = 256,
        # dynamic mode only: journal every step transition into a device list
        # of this many records (see "step-transition journal")
        event_cap: Optional[int] = None,
        # dynamic mode only: "external" leaves every approval hold WAITING
        # until decide() settles it (see "externally decided approvals");
        # hold_cap is the page size of open_holds()
        approvals: str = "auto",
        hold_cap: Optional[int] = None,
        # dynamic mode only: retry / backoff / timeout per step, read from the
        # template by wf_settle (see "per-step policy")
        step_policy: bool = False,
        # dynamic mode only: predicates over run inputs and step outputs,
        # decided by wf_cond_eval (see "conditions decided on the device")
        device_conditions: bool = False,
        input_words: int = 8,
    ):
        if approvals not in ("auto", "external"):
            raise ValueError("approvals must be 'auto' or 'external'")
        self.device_conditions = bool(device_conditions)
        self.step_policy = bool(step_policy)
        self.external = approvals == "external"
        # every option lives in dynamic mode only
        for on, why in (
                (self.device_conditions, "device_conditions needs dynamic_capacity: the "
                                         "predicates are held per template"),
                (self.step_policy, "step_policy needs dynamic_capacity: the policy is "
                                   "held per template"),
                (self.external, "approvals='external' needs dynamic_capacity: a "
                                "decision names a run by (slot, generation)"),
                (event_cap is not None, "event_cap needs dynamic_capacity: the journal "
                                        "reports runs by (slot, generation)")):
            if on and dynamic_capacity is None:
                raise ValueError(why)
        if self.device_conditions:
            if not 1 <= int(input_words) <= 32:
                raise ValueError("device_conditions needs 1 <= input_words <= 32")
            if int(payload_words) < int(input_words) + 2:
                raise ValueError("device_conditions needs payload_words >= "
                                 "input_words + 2 (inputs, ordinal, step)")
            self.input_words = int(input_words)
        if hold_cap is not None:
            if not self.external:
                raise ValueError("hold_cap needs approvals='external'")
            if int(hold_cap) < 1:
                raise ValueError("hold_cap must be >= 1")
        self.hold_cap = hold_cap
        if event_cap is not None:
            if int(event_cap) < 1:
                raise ValueError("event_cap must be >= 1")
            event_cap = int(event_cap)
        self.event_cap = event_cap
        self.event_overflows = 0
        self.max_retries = max_retries
        self.timeout_cutoff = timeout_cutoff
        for dg in dags:
            for s in dg.steps:
                self._check_step(s)
        device = torch.device(device)
        self.ext = _RefOps() if backend == "ref" else get_ext(required=True)
        self.device = device
        self.world = world_size
        self.rank = rank
        self.NWL = n_local_workers
        self.W = payload_words
        self.fail_ppt = fail_ppt
        self.drop_ppt = drop_ppt
        self.approval_verdict = approval_verdict
        if replicate is not None:
            assert len(dags) == 1
        NR = replicate if replicate is not None else len(dags)
        self.dynamic = dynamic_capacity is not None
        if self.dynamic:
            assert replicate is None, "dynamic mode admits runs, it replicates none"
            NR = int(dynamic_capacity)
            assert NR >= 1 and len(dags) <= template_cap
            templates, dags = list(dags), ()   # no run exists at construction
        self.NR = NR
        assert all(len(d.steps) <= 64 for d in dags), "device DAGs cap at 64 steps"

        # ---- host-side template tables (the run-creation image) -------------
        TN = 1 if replicate is not None else NR
        st = torch.zeros(TN * 64, dtype=torch.uint8)
        deps = torch.zeros(TN * 64, dtype=torch.int64)
        kinds = torch.zeros(TN * 64, dtype=torch.uint8)
        todo = torch.zeros(TN * 64, dtype=torch.int32)
        maxp = torch.zeros(TN * 64, dtype=torch.int32)
        nready = torch.zeros(TN * 64, dtype=torch.int32)
        nsteps = torch.zeros(TN, dtype=torch.uint8)
        cond = torch.zeros(TN, dtype=torch.int64)
        total_children = 0
        for r, dag in enumerate(dags):
            rows, row = _lower_steps(dag), slice(r * 64, r * 64 + 64)
            kinds[row], deps[row], todo[row] = rows.kind, rows.deps, rows.todo
            maxp[row], nready[row] = rows.maxp, rows.delay
            nsteps[r], cond[r] = rows.n_steps, rows.cond
            total_children += rows.children
        if replicate is not None:
            st, deps, kinds, todo, maxp, nready, nsteps, cond = (
                t.repeat(NR) for t in (st, deps, kinds, todo, maxp, nready, nsteps, cond))
            total_children *= NR
        if self.dynamic:
            # arena sizing only: every slot holding the widest template
            total_children = NR * max([_lower_steps(t).children for t in templates],
                                      default=1)
        self.total_children = total_children
        self._tmpl = {
            "step_state": st, "deps_mask": deps, "step_kind": kinds,
            "children_todo": todo, "next_ready": nready, "n_steps": nsteps,
            "cond_bits": cond, "max_parallel": maxp,
        }

        d = device
        # copy=True is load-bearing: on CPU, .to(device) ALIASES the source,
        # and the live tables must not share storage with the creation
        # template (reset_runs / wf_readmit restore from it)
        self.step_state = st.to(d, copy=True)
        self.deps_mask = deps.to(d, copy=True)
        self.step_kind = kinds.to(d, copy=True)
        self.children_todo = todo.to(d, copy=True)
        self.max_parallel = maxp.to(d, copy=True)
        self.next_ready = nready.to(d, copy=True)
        self.n_steps = nsteps.to(d, copy=True)
        self.cond_bits = cond.to(d, copy=True)
        self.run_active = torch.ones(NR, dtype=torch.uint8, device=d)
        self.run_state = torch.zeros(NR, dtype=torch.uint8, device=d)
        self.step_attempts = torch.zeros(NR * 64, dtype=torch.int32, device=d)
        self.children_out = torch.zeros(NR * 64, dtype=torch.int32, device=d)
        self.children_emitted = torch.zeros(NR * 64, dtype=torch.int32, device=d)
        self.children_done = torch.zeros(NR * 64, dtype=torch.int32, device=d)
        self.children_fail = torch.zeros(NR * 64, dtype=torch.int32, device=d)
        self.wf_counts = torch.zeros(2, dtype=torch.int64, device=d)
        self.dispatch_tick = torch.zeros(NR * 64, dtype=torch.int32, device=d)
        self.timeout_count = torch.zeros(1, dtype=torch.int64, device=d)
        # device tick counter: kernels read it from memory so the whole tick
        # body is hipGraph-capturable (a scalar arg would freeze in capture)
        self.tick_buf = torch.full((1,), -1, dtype=torch.int32, device=d)
        self.retry_count = torch.zeros(1, dtype=torch.int64, device=d)
        self.admit_count = torch.zeros(1, dtype=torch.int64, device=d)

        # dispatch + approval lists (overflowing entries simply retry on the
        # next sweep, so the cap bounds memory, not correctness)
        self.disp_cap = min(NR * 64, 1 << 22)
        self.disp_runs = torch.zeros(self.disp_cap, dtype=torch.int32, device=d)
        self.disp_steps = torch.zeros(self.disp_cap, dtype=torch.int32, device=d)
        self.disp_count = torch.zeros(1, dtype=torch.int32, device=d)
        self.appr_runs = torch.zeros(NR, dtype=torch.int32, device=d)
        self.appr_steps = torch.zeros(NR, dtype=torch.int32, device=d)
        self.appr_count = torch.zeros(1, dtype=torch.int32, device=d)

        # ---- child-job arena -------------------------------------------------
        CB = child_cap or max(1024, min(total_children, 1 << 18))
        self.CB = CB
        self.child_tag = torch.zeros(CB, dtype=torch.int32, device=d)
        self.child_seq = torch.zeros(CB, dtype=torch.int32, device=d)
        self.child_widx = torch.zeros(CB, dtype=torch.int32, device=d)
        self.child_count = torch.zeros(1, dtype=torch.int32, device=d)
        g = torch.Generator().manual_seed(seed * 17 + rank)
        self.child_payload = torch.randint(
            -(1 << 31), (1 << 31) - 1, (CB * payload_words,),
            dtype=torch.int32, generator=g).to(d)

        # ---- worker table (global view over all ranks' pools) ---------------
        NWG = self.NWL * world_size
        self.w_pool = (torch.arange(NWG, dtype=torch.int32) // self.NWL).to(d)
        maxp = max(64, (4 * CB) // max(1, self.NWL))
        self.w_maxp = torch.full((NWG,), maxp, dtype=torch.int32, device=d)
        self.w_labels = torch.zeros(NWG, dtype=torch.int64, device=d)
        self.w_active_local = torch.zeros(self.NWL, dtype=torch.int32, device=d)
        self.w_cpu_local = (torch.rand(self.NWL, generator=g) * 50).to(d)
        self.w_gpu_local = (torch.rand(self.NWL, generator=g) * 50).to(d)
        if world_size == 1:
            # the local view IS the global view: no per-tick D2D copies
            self.w_active = self.w_active_local
            self.w_cpu = self.w_cpu_local
            self.w_gpu = self.w_gpu_local
        else:
            self.w_active = torch.zeros(NWG, dtype=torch.int32, device=d)
            self.w_cpu = torch.zeros(NWG, dtype=torch.float32, device=d)
            self.w_gpu = torch.zeros(NWG, dtype=torch.float32, device=d)
        self.w_keys = torch.zeros(NWG, dtype=torch.int64, device=d)
        self.order_buf = torch.arange(NWG, dtype=torch.int32, device=d)
        self.valid_buf = torch.tensor([NWG], dtype=torch.int32, device=d)

        # ---- padded exchange arenas (child dispatch across ranks) -----------
        self.pad_cap = pad_cap or min(CB, max(64, (4 * CB) // max(1, world_size)))
        cap, Wd, world = self.pad_cap, payload_words, world_size

        def zi(n):
            return torch.zeros(n, dtype=torch.int32, device=d)

        self.pad_send_slots = zi(world * cap)
        self.pad_send_widx = zi(world * cap)
        self.pad_send_cnt = zi(world)
        self.pad_recv_cnt = zi(world)
        self.pad_recv_widx = zi(world * cap)
        self.pad_send_payload = torch.zeros(world * cap * Wd, dtype=torch.int32, device=d)
        self.pad_recv_payload = torch.zeros_like(self.pad_send_payload)
        self.pad_res = torch.zeros_like(self.pad_send_payload)
        self.pad_sums = zi(world * cap)
        self.pad_sums_back = zi(world * cap)
        # requeue ring (children parked on destination overflow) + tag carry.
        # Sized well below the child arena: overflow is the exception, and
        # the ring's payload arena is ping-pong COPIED every tick inside the
        # captured graph — a CB-sized ring made that copy 28% of the tick
        # (profiles/r29_wf_tick_ktrace). Ring-full drops land in the dead
        # list -> wf_apply_dead -> the children retry, so a small ring is
        # safe backpressure, not loss.
        RQ = min(CB, max(4096, CB // 16))
        self.rq_src = zi(RQ)
        self.rq_widx = zi(RQ)
        self.rq_attempts = zi(RQ)
        self.rq_count = zi(1)
        self.rq_dead = torch.zeros(1, dtype=torch.int64, device=d)
        self.rq_payload = torch.zeros(RQ * Wd, dtype=torch.int32, device=d)
        self.rq_tag = zi(RQ)
        self.rq_seq = zi(RQ)
        self.rq_prev_widx = zi(RQ)
        self.rq_prev_attempts = zi(RQ)
        self.rq_prev_count = zi(1)
        self.rq_prev_payload = torch.zeros_like(self.rq_payload)
        self.rq_prev_tag = zi(RQ)
        self.rq_prev_seq = zi(RQ)
        self.dead_src = zi(RQ)
        self.dead_count = zi(1)

        # host-side pinned staging for the approval hop
        pin = d.type == "cuda"
        self._appr_host_runs = torch.zeros(NR, dtype=torch.int32)
        self._appr_host_steps = torch.zeros(NR, dtype=torch.int32)
        if pin:
            self._appr_host_runs = self._appr_host_runs.pin_memory()
            self._appr_host_steps = self._appr_host_steps.pin_memory()
        self._pending_grants: List[tuple] = []
        # routable slot list for pack_by_dest = child arena indices 0..C-1
        self._iota = torch.arange(CB, dtype=torch.int32, device=d)
        self._wf_graph = None      # None: not captured yet; (): capture failed
        # what a tick changes on an empty table, put back after the capture's
        # warm-up; an option appends its cumulative counters as it allocates
        self._counters = [self.tick_buf, self.wf_counts, self.timeout_count,
                          self.retry_count, self.admit_count, self.rq_dead]
        if device.type == "cuda":
            self._appr_h_count = torch.zeros(1, dtype=torch.int32).pin_memory()
            self._appr_ev = torch.cuda.Event()
        else:
            self._appr_h_count = None

        self._tick = 0
        if self.dynamic:
            self._init_dynamic(templates, template_cap)

    # ---- run lifecycle (dynamic mode) ---------------------------------------
    def _init_dynamic(self, templates: Sequence[DagSpec], template_cap: int) -> None:
        self._init_lifecycle(int(template_cap))
        if self.event_cap is not None:
            self._init_journal()
        if self.external:
            self._init_holds()
        if self.step_policy:
            self._init_policy()
        if self.step_policy or self.device_conditions:
            # one column serves both options. It has one spare word past the
            # table: admit() sends the template ids of refused requests there.
            self._run_tmpl_buf = torch.zeros(self.NR + 1, dtype=torch.int32,
                                             device=self.device)
            self.run_tmpl = self._run_tmpl_buf[:self.NR]
        if self.device_conditions:
            self._init_conditions()
        for dag in templates:
            self.add_template(dag)
        # Dynamic mode warms up and captures the tick on the EMPTY table, at
        # construction: n calls of tick() then advance the tables by exactly n
        # ticks with the graph or without it. On an empty table the body
        # changes only the tick counter and (never, but restored alike) the
        # cumulative counters, which are put back.
        if self._graph_allowed():
            self._capture_tick()

    def _init_lifecycle(self, TC: int) -> None:
        d, NR = self.device, self.NR
        self.run_active.zero_()               # every slot starts FREE
        self.template_cap = TC
        self.n_templates = 0
        self._tmpl_cond: List[int] = []
        # per template, for admit(keep=...): the CONDITION steps, and those
        # among them without a predicate, as step masks
        self._tmpl_cond_steps: List[int] = []
        self._tmpl_plain_steps: List[int] = []
        self.tmpl_deps =torch.zeros(TC * 64, dtype=torch.int64, device=d)
        self.tmpl_kind = torch.zeros(TC * 64, dtype=torch.uint8, device=d)
        self.tmpl_todo = torch.zeros(TC * 64, dtype=torch.int32, device=d)
        self.tmpl_maxp = torch.zeros(TC * 64, dtype=torch.int32, device=d)
        self.tmpl_delay = torch.zeros(TC * 64, dtype=torch.int32, device=d)
        self.tmpl_nsteps = torch.zeros(TC, dtype=torch.uint8, device=d)
        self.run_life = torch.zeros(NR, dtype=torch.uint8, device=d)
        self.run_gen = torch.zeros(NR, dtype=torch.int32, device=d)
        self.cancel_count = torch.zeros(1, dtype=torch.int64, device=d)
        # completion records share one buffer so a drain is one D2H copy:
        # [count | slot[NR] | gen[NR] | state[NR]]. A run is reported once,
        # so NR records cannot overflow.
        self._done_buf = torch.zeros(1 + 3 * NR, dtype=torch.int32, device=d)
        self.done_count = self._done_buf[0:1]
        self.done_slot = self._done_buf[1:1 + NR]
        self.done_gen = self._done_buf[1 + NR:1 + 2 * NR]
        self.done_state = self._done_buf[1 + 2 * NR:1 + 3 * NR]
        self._done_host = torch.zeros(1 + 3 * NR, dtype=torch.int32)
        if d.type == "cuda":
            self._done_host = self._done_host.pin_memory()
        # wf_admit workspaces: free-slot masks and scanned block counts
        nblk = (NR + 255) // 256
        self._free_mask = torch.zeros(nblk * 4, dtype=torch.int64, device=d)
        self._blk_scan = torch.zeros(nblk + 1, dtype=torch.int32, device=d)

    # ---- per-step policy (dynamic mode, step_policy=True) --------------------
    # Retry, backoff and timeout are properties of a step, held per template
    # (templates are append-only) and not per run:
    #   tmpl_policy  [template_cap*64*4]  one 16-byte record per step:
    #                (max_retries, backoff_ticks, cap_ticks, multiplier_q8)
    #   tmpl_timeout [template_cap*64]    ticks until lost children are written
    #                off, resolved (never 0, never below timeout_cutoff)
    #   run_tmpl     [NR]                 the template of the row's occupant,
    #                written by admit(); a row is admitted only there, so it
    #                holds for as long as the row is LIVE or DRAINING
    # wf_settle does per DISPATCHED step what wf_timeout_scan and then
    # wf_commit do, with these constants, and replaces both in the tick. A
    # step without a RetrySpec gets the pipeline's max_retries with the stock
    # 2 / x2 / cap 16, a step without timeout_ticks the pipeline's cutoff, so
    # a pipeline with no annotated step computes what it computes without
    # step_policy.
    #
    # A step's timeout can only lengthen the wait: timeout_cutoff is what
    # guarantees that a child parked in the requeue ring is never declared
    # lost and applied afterwards, and wf_retire keeps releasing rows by it.
    # A FREE row can therefore hold a DISPATCHED step whose longer timeout
    # has not run out; wf_settle skips FREE rows.
    _POLICY_KINDS = (WFK_WORKER, WFK_FOR_EACH)

    def _init_policy(self) -> None:
        # every record starts as the pipeline's own constants, so a row can
        # never read a zero timeout
        d, TC = self.device, self.template_cap
        if not 0 <= int(self.max_retries) <= 32767:
            raise ValueError("step_policy needs max_retries in 0..32767")
        if int(self.timeout_cutoff) < 1:
            raise ValueError("step_policy needs timeout_cutoff >= 1")
        stock = RetrySpec(int(self.max_retries))
        self.tmpl_policy = torch.tensor(
            [stock.max_retries, stock.backoff_ticks, stock.cap_ticks,
             stock.multiplier_q8], dtype=torch.int32).repeat(TC * 64).to(d)
        self.tmpl_timeout = torch.full((TC * 64,), int(self.timeout_cutoff),
                                       dtype=torch.int32, device=d)

    def _add_policy_rows(self, t: int, dag: DagSpec) -> None:
        stock = RetrySpec(int(self.max_retries))
        pol, tmo = [], []
        for s in range(64):
            sp = dag.steps[s] if s < len(dag.steps) else None
            r = sp.retry if sp is not None and sp.retry is not None else stock
            pol += [int(r.max_retries), int(r.backoff_ticks), int(r.cap_ticks),
                    int(r.multiplier_q8)]
            tmo.append(int(sp.timeout_ticks) if sp is not None and sp.timeout_ticks
                       else int(self.timeout_cutoff))
        self.tmpl_policy[t * 256:t * 256 + 256].copy_(torch.tensor(pol, dtype=torch.int32))
        self.tmpl_timeout[t * 64:t * 64 + 64].copy_(torch.tensor(tmo, dtype=torch.int32))

    # ---- conditions decided on the device (dynamic mode, device_conditions) --
    # Tables, allocated only with the option on:
    #   run_input      [(NR+1)*IW]  the run's input words, written by admit()
    #   step_out       [(NR+1)*64]  one output word per step: a WORKER or
    #                  FOR_EACH step's is the wraparound sum of the result
    #                  words of its children that finally succeeded, a
    #                  CONDITION step's 1 or 0, everything else 0
    #   run_tmpl       [NR]         shared with step_policy
    #   tmpl_cond      [TC*64*4]    one record (code, a, b, imm) per step
    #   tmpl_cond_mask [TC]         bit s = step s carries a predicate
    #   cond_counts    [2]          predicates evaluated true / false
    # Record: code bits 0..3 op (WFC_*), bit 4 negate, bits 8..9 lhs kind
    # (1 INPUT, 2 OUT), bits 12..13 rhs kind (0 IMM, 1 INPUT, 2 OUT); a / b the
    # operand index, imm the immediate. Signed 32-bit comparisons.
    #
    # wf_child_payload makes a child's payload (input words, ordinal, step,
    # zeros), so its echo checksum depends on nothing else; wf_apply_out adds
    # the checksum of each child counted done into its step's output word.
    # wf_cond_eval, directly before the sweep, evaluates every PENDING step
    # with a predicate whose deps are satisfied. An OUT operand must name a
    # step among the transitive deps, so it is final when read, and inputs
    # never change: a step that returns to PENDING evaluates the same again.
    # A CONDITION without a predicate keeps its admitted bit, and admit()
    # writes that bit as its output word.
    _OUT_KINDS = (WFK_WORKER, WFK_FOR_EACH, WFK_CONDITION)

    def _init_conditions(self) -> None:
        # run_input and step_out have one spare row past the table, as
        # run_tmpl has a spare word: admit() sends the rows of refused
        # requests there.
        d, NR, TC, IW = self.device, self.NR, self.template_cap, self.input_words
        self._run_input_buf = torch.zeros((NR + 1) * IW, dtype=torch.int32, device=d)
        self.run_input = self._run_input_buf[:NR * IW]
        self._step_out_buf = torch.zeros((NR + 1) * 64, dtype=torch.int32, device=d)
        self.step_out = self._step_out_buf[:NR * 64]
        self.tmpl_cond = torch.zeros(TC * 64 * 4, dtype=torch.int32, device=d)
        self.tmpl_cond_mask = torch.zeros(TC, dtype=torch.int64, device=d)
        # 1 where the template's step is a CONDITION without a predicate:
        # its output word is the admitted bit, written by admit()
        self._tmpl_plain_cond = torch.zeros(TC * 64, dtype=torch.int32, device=d)
        self._bit_idx = torch.arange(64, dtype=torch.int64, device=d)
        self._any_plain_cond = False
        self.cond_counts = torch.zeros(2, dtype=torch.int64, device=d)
        self._counters.append(self.cond_counts)

    def _add_cond_rows(self, t: int, dag: DagSpec, cond_recs: dict) -> None:
        rec, cm = [0] * 256, 0
        for s, r4 in cond_recs.items():
            rec[4 * s:4 * s + 4] = r4
            cm |= 1 << s
        self.tmpl_cond[t * 256:t * 256 + 256].copy_(torch.tensor(rec, dtype=torch.int32))
        self.tmpl_cond_mask[t:t + 1].fill_(_i64(cm))
        plain = [int(s < len(dag.steps) and dag.steps[s].kind == WFK_CONDITION
                     and dag.steps[s].when is None) for s in range(64)]
        self._tmpl_plain_cond[t * 64:t * 64 + 64].copy_(
            torch.tensor(plain, dtype=torch.int32))
        self._any_plain_cond = self._any_plain_cond or any(plain)

    def _admit_cond_rows(self, dst, tmpl, cond, inputs) -> None:
        """Input row and output row of the runs just admitted; `dst` as in
        admit(). The outputs start at zero, but for a CONDITION step without
        a predicate: its output is the bit it was admitted with."""
        dst = dst.long()
        self._run_input_buf.view(-1, self.input_words)[dst] = \
            inputs.view(-1, self.input_words)
        if self._any_plain_cond:
            bits = (cond[:, None] >> self._bit_idx[None, :]) & 1
            self._step_out_buf.view(-1, 64)[dst] = \
                bits.to(torch.int32) * self._tmpl_plain_cond.view(-1, 64)[tmpl.long()]
        else:       # no template has such a step: fewer launches per admit
            self._step_out_buf.view(-1, 64)[dst] = 0

    def _cond_record(self, dag: DagSpec, s: int) -> List[int]:
        """Validated (code, a, b, imm) of step s's predicate."""
        w = dag.steps[s].when
        op = _WFC_OPS.get(w.op, w.op) if isinstance(w.op, str) else w.op
        if isinstance(op, bool) or not isinstance(op, int) or not WFC_EQ <= op <= WFC_TRUTHY:
            raise ValueError(f"unknown predicate op {w.op!r}")
        reach, stack = set(), list(dag.steps[s].deps)
        while stack:
            j = stack.pop()
            if 0 <= j < len(dag.steps) and j not in reach:
                reach.add(j)
                stack.extend(dag.steps[j].deps)

        def operand(x, side):
            if isinstance(x, int) and not isinstance(x, bool):
                if side == "lhs":
                    raise ValueError("the lhs of a predicate is ('input', k) or ('out', j)")
                if not _I32_MIN <= x <= _I32_MAX:
                    raise ValueError(f"immediate {x} is outside int32")
                return 0, 0, x
            if not (isinstance(x, (tuple, list)) and len(x) == 2
                    and x[0] in ("input", "out") and isinstance(x[1], int)
                    and not isinstance(x[1], bool)):
                raise ValueError(f"bad predicate operand {x!r}")
            if x[0] == "input":
                if not 0 <= x[1] < self.input_words:
                    raise ValueError(f"input word {x[1]} outside 0..{self.input_words - 1}")
                return 1, x[1], 0
            if x[1] not in reach:
                raise ValueError(
                    f"step {s} reads the output of step {x[1]}, which is not among its "
                    "(transitive) dependencies: an operand must be final when read")
            if dag.steps[x[1]].kind not in self._OUT_KINDS:
                raise ValueError(f"step {x[1]} has no output (WORKER, FOR_EACH and "
                                 "CONDITION steps have one)")
            return 2, x[1], 0

        lk, a, _ = operand(w.lhs, "lhs")
        rk, b, imm = (0, 0, 0) if op == WFC_TRUTHY else operand(w.rhs, "rhs")
        return [op | (16 if w.negate else 0) | (lk << 8) | (rk << 12), a, b, imm]

    def cond_stats(self) -> dict:
        """Cumulative predicates evaluated true / false."""
        self._require_dynamic(True, "cond_stats")
        if not self.device_conditions:
            raise RuntimeError("cond_stats needs device_conditions=True")
        c = self.cond_counts.cpu().tolist()
        return {"true": c[0], "false": c[1]}

    def _check_step(self, spec: StepSpec, arena: Optional[int] = None) -> None:
        """Every check of one StepSpec against the pipeline's options; `arena`
        is the child arena a template's fan-out has to fit."""
        if arena is not None and spec.kind == WFK_FOR_EACH and spec.fanout > arena:
            raise ValueError(f"fanout {spec.fanout} can never be emitted "
                             f"(child arena {arena})")
        if spec.ttl_ticks:
            if not self.external:
                raise ValueError("ttl_ticks needs approvals='external'")
            if spec.kind != WFK_APPROVAL or spec.ttl_ticks < 0:
                raise ValueError("ttl_ticks is a positive tick count on an "
                                 "APPROVAL step")
        self._check_policy(spec)
        if spec.when is not None and not self.device_conditions:
            raise ValueError("when needs device_conditions=True")

    def _check_policy(self, spec: StepSpec) -> None:
        if spec.retry is None and not spec.timeout_ticks:
            return
        if not self.step_policy:
            raise ValueError("retry / timeout_ticks need step_policy=True")
        if spec.kind not in self._POLICY_KINDS:
            raise ValueError("retry / timeout_ticks belong on a step that emits "
                             "children (WORKER, FOR_EACH)")
        t = int(spec.timeout_ticks)
        if t < 0 or 0 < t < self.timeout_cutoff:
            raise ValueError(
                f"timeout_ticks {t} is below timeout_cutoff {self.timeout_cutoff}: a "
                "child parked in the requeue ring could be declared lost and "
                "then applied")
        if t > (1 << 30):
            raise ValueError("timeout_ticks must stay below 2^30")
        r = spec.retry
        if r is None:
            return
        for name, lo, hi in (("max_retries", 0, 32767), ("backoff_ticks", 1, 1 << 20),
                             ("multiplier_q8", 256, 65535), ("cap_ticks", 0, 1 << 20)):
            if not lo <= int(getattr(r, name)) <= hi:
                raise ValueError(f"{name} {getattr(r, name)} outside {lo}..{hi}")

    def _require_dynamic(self, dynamic: bool, what: str) -> None:
        if self.dynamic != dynamic:
            raise RuntimeError(
                f"{what} needs a {'dynamic' if dynamic else 'static'}-mode "
                f"pipeline (dynamic_capacity {'unset' if dynamic else 'set'})")

    def add_template(self, dag: DagSpec) -> int:
        """Register one more workflow template; returns its id."""
        self._require_dynamic(True, "add_template")
        rows = _lower_steps(dag)
        t = self.n_templates
        if t >= self.template_cap:
            raise ValueError(f"template table full ({self.template_cap})")
        for spec in dag.steps:
            self._check_step(spec, arena=self.CB)
        cond_recs = {s: self._cond_record(dag, s) for s, sp in enumerate(dag.steps)
                     if sp.when is not None}
        row = slice(t * 64, t * 64 + 64)
        self.tmpl_deps[row].copy_(rows.deps)
        self.tmpl_kind[row].copy_(rows.kind)
        self.tmpl_todo[row].copy_(rows.todo)
        self.tmpl_maxp[row].copy_(rows.maxp)
        self.tmpl_delay[row].copy_(rows.delay)
        self.tmpl_nsteps[t:t + 1].fill_(rows.n_steps)
        if self.external:
            self._add_ttl_row(t, dag)
        if self.step_policy:
            self._add_policy_rows(t, dag)
        if self.device_conditions:
            self._add_cond_rows(t, dag, cond_recs)
        self._tmpl_cond.append(rows.cond)
        conds = [s for s, sp in enumerate(dag.steps) if sp.kind == WFK_CONDITION]
        self._tmpl_cond_steps.append(sum(1 << s for s in conds))
        self._tmpl_plain_steps.append(
            sum(1 << s for s in conds if dag.steps[s].when is None))
        self.n_templates = t + 1
        return t

    def admit(self, templates: Sequence[int], cond_bits=None, fanout=None, inputs=None,
              keep=None, outs=None):
        """Admit one run per template id into the lowest FREE slots; returns
        (slots, gens). slots[i] == -1: the table was full for request i.
        `inputs[i]` (device_conditions) holds at most input_words ints in
        int32 range, zero padded: the run's input words.

        `keep[i]` starts run i with steps already done (a rerun from a step):
        (done_mask, skipped_mask), or a bare int for (mask, 0). A step of
        done_mask starts SUCCEEDED, one of skipped_mask (a subset) SKIPPED.
        The done set has to lie inside the template's steps and hold every
        dependency of each of its steps; the device checks that, and
        slots[i] == -2 says it does not hold (such a request takes no slot;
        the requests around it land where they would have anyway). `outs[i]`
        (device_conditions) gives the output words of kept steps, as a
        {step: word} dict or a 64-entry row. A kept CONDITION step's word
        and condition bit are 1 if SUCCEEDED and 0 if SKIPPED whatever is
        passed; a step that is not kept starts as it does without `keep`."""
        self._require_dynamic(True, "admit")
        if keep is not None or outs is not None:
            return self._admit_keep(templates, cond_bits, fanout, inputs, keep, outs)
        n, req = self._pack_request(templates, cond_bits, fanout, inputs)
        if n == 0:
            return [], []
        req = req.to(self.device)         # the one H2D
        cond, tmpl = req[:2 * n].view(torch.int64), req[2 * n:3 * n]
        fanout, inputs = req[3 * n:4 * n], req[4 * n:]
        out = torch.empty(2 * n, dtype=torch.int32, device=self.device)
        slots = out[:n]
        self.ext.wf_admit(
            tmpl, cond, fanout,
            self.tmpl_deps, self.tmpl_kind, self.tmpl_todo, self.tmpl_maxp,
            self.tmpl_delay, self.tmpl_nsteps,
            self.step_state, self.step_attempts, self.deps_mask, self.step_kind,
            self.children_todo, self.max_parallel, self.children_out,
            self.children_done, self.children_fail, self.children_emitted,
            self.next_ready, self.dispatch_tick, self.n_steps, self.cond_bits,
            self.run_state, self.run_active, self.run_life, self.run_gen,
            self.tick_buf, self._free_mask, self._blk_scan,
            slots, out[n:], self.admit_count)
        if self.step_policy or self.device_conditions:
            # run_tmpl is a run column wf_admit does not know: one indexed
            # store of the accepted requests' template ids. A refused request
            # has slot -1, and -1 mod (NR + 1) = NR is the spare word past the
            # table, so no mask and no host round trip is needed.
            dst = torch.remainder(slots, self.NR + 1)
            self._run_tmpl_buf[dst] = tmpl
            if self.device_conditions:
                # the same trick for the run's input row and its output row
                self._admit_cond_rows(dst, tmpl, cond, inputs)
        if self.external and self._any_ttl:
            self._admit_hold_ttl(slots, tmpl)
        h = out.cpu()                     # the one D2H (synchronising)
        return h[:n].tolist(), h[n:].tolist()

    def _admit_keep(self, templates, cond_bits, fanout, inputs, keep, outs):
        """admit() with kept steps: one H2D of [cond | keep | skip as int64 |
        template ids | fanouts | input rows | output rows], wf_admit_keep,
        the side columns, one D2H."""
        tl, cl, fl, il = self._check_request(templates, cond_bits, fanout, inputs)
        n = len(tl)
        if outs is not None and not self.device_conditions:
            raise ValueError("outs need device_conditions=True")
        kl = [0] * n if keep is None else list(keep)
        ol = [None] * n if outs is None else list(outs)
        if len(kl) != n or len(ol) != n:
            raise ValueError("keep / outs must match templates in length")
        dl = [k[0] if type(k) in (tuple, list) else k for k in kl]
        sl = [k[1] if type(k) in (tuple, list) else 0 for k in kl]
        for m in dl + sl:
            if type(m) is not int or not 0 <= m < (1 << 64):
                raise ValueError(f"keep mask {m!r} is not a 64-bit mask")
        if any(sk & ~d for d, sk in zip(dl, sl)):
            raise ValueError("a skipped step must be among the done steps")
        rows = []
        if self.device_conditions or any(self._tmpl_cond_steps):
            for i, (d, sk) in enumerate(zip(dl, sl)):
                # a kept CONDITION step has decided: its bit says how
                cm = self._tmpl_cond_steps[tl[i]] & d
                if cm:
                    cl[i] = _i64(((cl[i] & ((1 << 64) - 1)) & ~cm) | (cm & ~sk))
                if self.device_conditions:
                    # a CONDITION without a predicate gets its word from its
                    # bit, below, like one that is not kept
                    plain = self._tmpl_plain_steps[tl[i]]
                    rows.append(self._out_row(ol[i], d, cm, cm & ~sk & ~plain))
        if n == 0:
            return [], []
        done = [d - (1 << 64) if d >> 63 else d for d in dl]
        skipped = [s - (1 << 64) if s >> 63 else s for s in sl]
        IW = self.input_words if self.device_conditions else 0
        OW = 64 if self.device_conditions else 0
        req = torch.empty(8 * n + n * IW + n * OW, dtype=torch.int32)
        req[:6 * n].view(torch.int64).copy_(
            torch.tensor(cl + done + skipped, dtype=torch.int64))
        req[6 * n:8 * n] = torch.tensor(tl + fl, dtype=torch.int32)
        if IW:
            req[8 * n:8 * n + n * IW] = torch.tensor(il, dtype=torch.int32)
            req[8 * n + n * IW:] = torch.tensor(rows, dtype=torch.int32).flatten()
        req = req.to(self.device)         # the one H2D
        m64 = req[:6 * n].view(torch.int64)
        cond, kept, skip = m64[:n], m64[n:2 * n], m64[2 * n:]
        tmpl, fan = req[6 * n:7 * n], req[7 * n:8 * n]
        out = torch.empty(2 * n, dtype=torch.int32, device=self.device)
        slots = out[:n]
        self.ext.wf_admit_keep(
            tmpl, cond, fan,
            self.tmpl_deps, self.tmpl_kind, self.tmpl_todo, self.tmpl_maxp,
            self.tmpl_delay, self.tmpl_nsteps,
            self.step_state, self.step_attempts, self.deps_mask, self.step_kind,
            self.children_todo, self.max_parallel, self.children_out,
            self.children_done, self.children_fail, self.children_emitted,
            self.next_ready, self.dispatch_tick, self.n_steps, self.cond_bits,
            self.run_state, self.run_active, self.run_life, self.run_gen,
            self.tick_buf, self._free_mask, self._blk_scan,
            slots, out[n:], self.admit_count, kept, skip)
        if self.step_policy or self.device_conditions:
            # every refused request, -1 or -2, goes to the spare row: -2 mod
            # (NR + 1) would be the table's last run
            dst = torch.where(slots < 0, self.NR, slots).long()
            self._run_tmpl_buf[dst] = tmpl
            if self.device_conditions:
                self._run_input_buf.view(-1, IW)[dst] = req[8 * n:8 * n + n * IW].view(-1, IW)
                # the kept steps' words; elsewhere what _admit_cond_rows writes
                plain = self._tmpl_plain_cond.view(-1, 64)[tmpl.long()]
                bits = ((cond[:, None] >> self._bit_idx[None, :]) & 1).to(torch.int32)
                self._step_out_buf.view(-1, 64)[dst] = \
                    req[8 * n + n * IW:].view(-1, 64) + bits * plain
        if self.external and self._any_ttl:
            self._admit_hold_ttl(slots, tmpl)
        h = out.cpu()                     # the one D2H (synchronising)
        return h[:n].tolist(), h[n:].tolist()

    def _out_row(self, words, done: int, decided: int, true: int) -> List[int]:
        """The 64 output words a request passes for its kept steps. The steps
        of `decided` are kept CONDITION steps: theirs is the bit of `true`."""
        row = [0] * 64
        if words is None:
            items = ()
        elif isinstance(words, dict):
            items = words.items()
        elif len(words) == 64:
            items = enumerate(words)
        else:
            raise ValueError("an outs row has 64 entries")
        for s, v in items:
            if isinstance(s, bool) or not isinstance(s, int) or not 0 <= s < 64:
                raise ValueError(f"outs names step {s!r}")
            if isinstance(v, bool) or not isinstance(v, int) \
                    or not _I32_MIN <= v <= _I32_MAX:
                raise ValueError(f"output word {v!r} is not an int32")
            if not done >> s & 1 and (v or isinstance(words, dict)):
                raise ValueError(f"outs gives a word for step {s}, which is not kept")
            row[s] = v
        for s in range(64 if decided else 0):
            if decided >> s & 1:
                row[s] = true >> s & 1
        return row

    def _check_request(self, templates, cond_bits, fanout, inputs):
        """Validated admit() request as lists: template ids, signed condition
        bits, fanouts and the flat, zero-padded input rows."""
        tl = [int(t) for t in templates]
        n = len(tl)
        for t in tl:
            if not 0 <= t < self.n_templates:
                raise ValueError(f"unregistered template id {t}")
        fl = [0] * n if fanout is None else [int(f) for f in fanout]
        for f in fl:
            if f < 0 or f > self.CB:
                raise ValueError(
                    f"fanout {f} can never be emitted (child arena {self.CB})")
        if cond_bits is None:
            cl = [self._tmpl_cond[t] for t in tl]
        else:
            cl = [_i64(int(c)) for c in cond_bits]
        if len(fl) != n or len(cl) != n:
            raise ValueError("cond_bits / fanout must match templates in length")
        IW = self.input_words if self.device_conditions else 0
        if inputs is not None and not self.device_conditions:
            raise ValueError("inputs need device_conditions=True")
        il: List[int] = []
        if IW:
            rows = [()] * n if inputs is None else [tuple(r) for r in inputs]
            if len(rows) != n:
                raise ValueError("inputs must match templates in length")
            for r in rows:
                if len(r) > IW:
                    raise ValueError(f"a run has at most {IW} input words")
                for v in r:
                    if isinstance(v, bool) or not isinstance(v, int) \
                            or not _I32_MIN <= v <= _I32_MAX:
                        raise ValueError(f"input word {v!r} is not an int32")
                il += list(r) + [0] * (IW - len(r))
        return tl, cl, fl, il

    def _pack_request(self, templates, cond_bits, fanout, inputs):
        """Validated admit() request as (n, one host buffer): [cond as int64 |
        template ids | fanouts | input rows]."""
        tl, cl, fl, il = self._check_request(templates, cond_bits, fanout, inputs)
        n = len(tl)
        IW = self.input_words if self.device_conditions else 0
        if n == 0:
            return 0, None
        req = torch.empty(4 * n + n * IW, dtype=torch.int32)
        if IW:
            req[4 * n:] = torch.tensor(il, dtype=torch.int32)
        req[:2 * n].view(torch.int64).copy_(torch.tensor(cl, dtype=torch.int64))
        req[2 * n:3 * n] = torch.tensor(tl, dtype=torch.int32)
        req[3 * n:4 * n] = torch.tensor(fl, dtype=torch.int32)
        return n, req

    def cancel(self, slots: Sequence[int], gens: Sequence[int]) -> List[int]:
        """Cancel the runs named by (slot, gen) handles; returns 1 per request
        that took effect. A stale generation, a finished run or a repeated
        slot in the same call gives 0."""
        self._require_dynamic(True, "cancel")
        sl, gl = [int(s) for s in slots], [int(g) for g in gens]
        if len(sl) != len(gl):
            raise ValueError("slots and gens must match in length")
        first = {}
        for i, s in enumerate(sl):   # the kernel assumes distinct slots
            first.setdefault(s, i)
        keep = sorted(first.values())
        ok = [0] * len(sl)
        if not keep:
            return ok
        n = len(keep)
        req = torch.tensor([sl[i] for i in keep] + [gl[i] for i in keep],
                           dtype=torch.int32).to(self.device)
        out = torch.zeros(n, dtype=torch.uint8, device=self.device)
        self.ext.wf_cancel(req[:n], req[n:], self.run_life, self.run_gen,
                           self.run_active, self.run_state, self.n_steps,
                           self.step_state, self.cancel_count, out)
        if self.event_cap is not None:
            # the slot can be drained and re-admitted before the next tick:
            # its CANCELLED transitions are journaled now or never
            self._journal(1)
        for i, v in zip(keep, out.cpu().tolist()):
            ok[i] = v
        return ok

    def drain_completed(self):
        """Report every run that became terminal since the last drain, once,
        as (slots, gens, states) sorted by slot, and free the slots whose
        rows are quiescent."""
        self._require_dynamic(True, "drain_completed")
        self.done_count.zero_()
        self.ext.wf_retire(self.run_life, self.run_active, self.run_state,
                           self.run_gen, self.n_steps, self.children_out,
                           self.dispatch_tick, self.tick_buf, self.timeout_cutoff,
                           self.done_slot, self.done_gen, self.done_state,
                           self.done_count)
        h = self._done_host
        h.copy_(self._done_buf)      # the one D2H (synchronising)
        NR = self.NR
        n = min(int(h[0]), NR)
        rec = sorted(zip(h[1:1 + n].tolist(), h[1 + NR:1 + NR + n].tolist(),
                         h[1 + 2 * NR:1 + 2 * NR + n].tolist()))
        return [r[0] for r in rec], [r[1] for r in rec], [r[2] for r in rec]

    # ---- step-transition journal (dynamic mode, event_cap set) ---------------
    # wf_journal compares every step state of the LIVE and DRAINING rows with
    # the state it last reported and appends (slot, gen, step, from, to,
    # stamp) per difference; stamp = 2 * tick + phase. Phase 0 is the pass
    # that ends each tick (inside the captured graph), phase 1 a pass between
    # ticks (after cancel(), and the catch-up passes of drain_events()).
    #
    # Order contract of drain_events():
    # - within one returned list a step never has two events with the same
    #   stamp, and list order is time order;
    # - per (slot, gen, step) the events chain: the first `from` is PENDING,
    #   each `from` is the previous `to`, and after a drain the last `to` is
    #   the live step_state;
    # - transitions between two passes coalesce: a worker step dispatched and
    #   completed in the same tick is one event, PENDING -> SUCCEEDED;
    # - the stamp's tick is the tick of detection. A full list delays events
    #   (to a later pass, with that pass's stamp) and loses none, provided
    #   the list is drained before the run's slot is released: a FREE row is
    #   not journaled, so drain events before drain_completed().
    def _init_journal(self) -> None:
        # The list is one buffer, [count, pad x3 | records], so the records
        # start 16-byte aligned for the kernel's vector stores. The shadow
        # starts as what an empty table is: all PENDING at generation 0,
        # which no admitted run ever has.
        d, NR = self.device, self.NR
        if self.event_cap + 64 * NR + 1024 > (1 << 31) - 1:
            raise ValueError("event_cap + 64 * dynamic_capacity must stay "
                             "below 2^31 (the device event counter)")
        self.ev_shadow_state = torch.zeros(NR * 64, dtype=torch.uint8, device=d)
        self.ev_shadow_gen = torch.zeros(NR, dtype=torch.int32, device=d)
        self._ev_buf = torch.zeros(4 + 4 * self.event_cap, dtype=torch.int32, device=d)
        self.ev_count = self._ev_buf[0:1]
        self.ev_rec = self._ev_buf[4:]
        self._counters.append(self.ev_count)

    def _require_events(self, what: str) -> None:
        self._require_dynamic(True, what)
        if self.event_cap is None:
            raise RuntimeError(f"{what} needs the step journal (event_cap unset)")

    def _journal(self, phase: int) -> None:
        self.ext.wf_journal(self.step_state, self.run_life, self.run_gen,
                            self.tick_buf, phase, self.ev_shadow_state,
                            self.ev_shadow_gen, self.ev_rec, self.ev_count)

    def drain_events(self):
        """Every step transition journaled since the last drain, as (slots,
        gens, steps, from_states, to_states, stamps) in time order: sorted by
        (stamp, slot, step). If the device list had filled up, catch-up
        passes run and are drained until one fits, their sub-lists appended
        in that order; each such pass either finishes or emits event_cap
        events, so this ends. `event_overflows` counts the drains that
        needed one."""
        self._require_events("drain_events")
        cap = self.event_cap
        cols: List[List[int]] = [[], [], [], [], [], []]
        overflowed = False
        while True:
            n = int(self.ev_count.cpu()[0])          # synchronising
            m = min(n, cap)
            if n:
                self.ev_count.zero_()
            if m:
                rec = self._ev_buf[4:4 + 4 * m].cpu().view(m, 4).to(torch.int64)
                w2 = rec[:, 2]
                step = w2 & 0xFF
                order = torch.sort(rec[:, 0] * 64 + step, stable=True)[1]
                order = order[torch.sort(rec[order, 3], stable=True)[1]]
                rec, w2, step = rec[order], w2[order], step[order]
                for c, v in zip(cols, (rec[:, 0], rec[:, 1], step, (w2 >> 8) & 0xFF,
                                       (w2 >> 16) & 0xFF, rec[:, 3])):
                    c.extend(v.tolist())
            # a list left full may have turned changes away: look again
            if n < cap:
                break
            overflowed = True
            self._journal(1)
        self.event_overflows += int(overflowed)
        return tuple(cols)

    # ---- externally decided approvals (dynamic mode, approvals="external") ---
    # An APPROVAL step the sweep set WAITING is a hold. wf_hold_scan, directly
    # after the sweep in every tick, keeps the hold tables in step with the
    # run table: hold_mask[r] bit s = step s has an open hold, hold_tick the
    # tick it opened, hold_ttl its expiry in ticks (0 = never; the template's
    # ttl_ticks, copied at admission). A row's hold data counts only while
    # hold_gen[r] == run_gen[r], the row is LIVE and run_active[r] == 1: a
    # slot can change hands between two ticks with no pass in between, so a
    # stale row must read as empty rather than be cleaned up in time.
    #
    # Timing contract:
    # - a hold opened at tick h with ttl_ticks = T expires in the scan of tick
    #   h + T if it is still WAITING then (the step FAILS, the run fails in
    #   that tick); a decision made before that tick wins;
    # - a decision made between tick k and k+1 is seen by the sweep of tick
    #   k+1: dependents dispatch in that tick, and the journal records
    #   WAITING -> SUCCEEDED with tick k+1, phase 0;
    # - decide() writes the one state byte; the next scan closes the hold, and
    #   open_holds() filters on the state, so a decided hold is gone at once.
    # The tables are rank-local; world > 1 runs the same scan eagerly.
    def _init_holds(self) -> None:
        # hold_gen starts at generation 0, which no admitted run ever has. The
        # page buffer is [count, pad x3 | records], records 16-byte aligned.
        d, NR, TC = self.device, self.NR, self.template_cap
        if 64 * NR + 1024 > (1 << 31) - 1:
            raise ValueError("64 * dynamic_capacity must stay below 2^31 "
                             "(hold keys and counts are 32-bit)")
        if self.hold_cap is None:
            self.hold_cap = min(64 * NR, 65536)
        self.hold_cap = int(self.hold_cap)
        self.tmpl_ttl = torch.zeros(TC * 64, dtype=torch.int32, device=d)
        self._any_ttl = False
        self.hold_mask = torch.zeros(NR, dtype=torch.int64, device=d)
        self.hold_tick = torch.zeros(NR * 64, dtype=torch.int32, device=d)
        self.hold_ttl = torch.zeros(NR * 64, dtype=torch.int32, device=d)
        self.hold_gen = torch.zeros(NR, dtype=torch.int32, device=d)
        self.hold_counts = torch.zeros(4, dtype=torch.int64, device=d)
        self.hold_open = torch.zeros(1, dtype=torch.int32, device=d)
        self._hold_buf = torch.zeros(4 + 4 * self.hold_cap, dtype=torch.int32, device=d)
        self._hold_list_mask = torch.zeros(NR, dtype=torch.int64, device=d)
        self._hold_blk_scan = torch.zeros((NR + 255) // 256 + 1, dtype=torch.int32,
                                          device=d)
        self._counters += [self.hold_counts, self.hold_open]

    def _add_ttl_row(self, t: int, dag: DagSpec) -> None:
        ttl = torch.tensor([sp.ttl_ticks for sp in dag.steps]
                           + [0] * (64 - len(dag.steps)), dtype=torch.int32)
        self.tmpl_ttl[t * 64:t * 64 + 64].copy_(ttl)
        self._any_ttl = self._any_ttl or bool(ttl.any())

    def _admit_hold_ttl(self, slots, tmpl) -> None:
        # hold_ttl is a run column like max_parallel: the template's row goes
        # into every slot just filled (all zero until a template carries a
        # ttl, so nothing to copy before that)
        ok = slots >= 0
        self.hold_ttl.view(-1, 64)[slots[ok].long()] = \
            self.tmpl_ttl.view(-1, 64)[tmpl[ok].long()]

    def _require_external(self, what: str) -> None:
        self._require_dynamic(True, what)
        if not self.external:
            raise RuntimeError(f"{what} needs approvals='external'")

    def open_holds(self):
        """Every open hold as (slots, gens, steps, since_ticks), ascending in
        (slot, step). The device returns pages of hold_cap records, each an
        exact prefix of what is left, so paging never skips or repeats."""
        self._require_external("open_holds")
        cap = self.hold_cap
        cols: List[List[int]] = [[], [], [], []]
        cursor = 0
        while True:
            self.ext.wf_hold_list(self.step_state, self.run_life, self.run_active,
                                  self.run_gen, self.hold_mask, self.hold_tick,
                                  self.hold_gen, cursor, self._hold_list_mask,
                                  self._hold_blk_scan, self._hold_buf)
            n = int(self._hold_buf[0:1].cpu()[0])    # synchronising
            m = min(n, cap)
            if m:
                rec = self._hold_buf[4:4 + 4 * m].cpu().view(m, 4)
                for c, v in zip(cols, rec.t().tolist()):
                    c.extend(v)
            if n <= cap:
                break
            cursor = cols[0][-1] * 64 + cols[2][-1] + 1
        return tuple(cols)

    def decide(self, slots: Sequence[int], gens: Sequence[int],
               steps: Sequence[int], verdicts: Sequence[int]) -> List[int]:
        """Approve (verdict 1) or reject (0) the holds named by (slot, gen,
        step); returns one code per request: 0 applied, 1 stale handle, 2 run
        no longer active, 3 not a waiting approval, 4 the (slot, step) was
        already named earlier in this call (only the first is sent)."""
        self._require_external("decide")
        cols = [[int(x) for x in c] for c in (slots, gens, steps, verdicts)]
        n = len(cols[0])
        if any(len(c) != n for c in cols):
            raise ValueError("slots, gens, steps and verdicts must match in length")
        first = {}
        for i in range(n):           # the kernel assumes distinct (slot, step)
            first.setdefault((cols[0][i], cols[2][i]), i)
        keep = sorted(first.values())
        codes = [4] * n
        if not keep:
            return codes
        k = len(keep)
        req = torch.tensor([c[i] for c in cols for i in keep],
                           dtype=torch.int32).to(self.device)
        out = torch.zeros(k, dtype=torch.uint8, device=self.device)
        self.ext.wf_decide(req[:k], req[k:2 * k], req[2 * k:3 * k], req[3 * k:],
                           self.run_life, self.run_gen, self.run_active,
                           self.n_steps, self.step_kind, self.step_state,
                           self.hold_counts, out)
        for i, v in zip(keep, out.cpu().tolist()):
            codes[i] = v
        return codes

    def hold_stats(self) -> dict:
        """Cumulative holds opened / expired / approved / rejected, and the
        number open after the last tick's scan."""
        self._require_external("hold_stats")
        c = self.hold_counts.cpu().tolist()
        return {"opened": c[0], "expired": c[1], "approved": c[2],
                "rejected": c[3], "open": int(self.hold_open.cpu()[0])}

    # ---- run admission -------------------------------------------------------
    def reset_runs(self) -> None:
        """Re-admit the whole run wave: copy the creation image back into the
        device tables (this is the honest run-creation H2D cost when the
        template lives on the host; templates are staged once)."""
        self._require_dynamic(False, "reset_runs")
        t = self._ensure_tmpl_dev()
        self.step_state.copy_(t["step_state"])
        self.children_todo.copy_(t["children_todo"])
        self.next_ready.copy_(t["next_ready"])
        self.run_active.fill_(1)
        self.run_state.zero_()
        self.step_attempts.zero_()
        self.children_out.zero_()
        self.children_emitted.zero_()
        self.children_done.zero_()
        self.children_fail.zero_()
        self.rq_count.zero_()
        self.rq_prev_count.zero_()
        self.dead_count.zero_()
        self.dispatch_tick.zero_()
        self._pending_grants.clear()
        self._appr_deferred = False
        self._tick = 0  # delay gates + backoff are wave-relative ticks
        self.tick_buf.fill_(-1)

    # ---- collectives ---------------------------------------------------------
    def _heartbeats(self) -> None:
        if self.world > 1:
            dist.all_gather_into_tensor(self.w_active, self.w_active_local)
            if not getattr(self, "_hb_static_done", False):
                dist.all_gather_into_tensor(self.w_cpu, self.w_cpu_local)
                dist.all_gather_into_tensor(self.w_gpu, self.w_gpu_local)
                self._hb_static_done = True
        # world == 1: the global tensors alias the local ones — nothing to do

    def _exchange_out(self) -> None:
        if self.world > 1:
            dist.all_to_all_single(self.pad_recv_cnt, self.pad_send_cnt)
            dist.all_to_all_single(self.pad_recv_widx, self.pad_send_widx)
            dist.all_to_all_single(self.pad_recv_payload, self.pad_send_payload)
        else:
            self.pad_recv_cnt.copy_(self.pad_send_cnt)
            self.pad_recv_widx.copy_(self.pad_send_widx)
            self.pad_recv_payload.copy_(self.pad_send_payload)

    def _exchange_back(self) -> None:
        if self.world > 1:
            dist.all_to_all_single(self.pad_sums_back, self.pad_sums)
        else:
            self.pad_sums_back.copy_(self.pad_sums)

    def _refresh_order(self) -> None:
        if self._tick % 8 != 1:
            return
        self.order_buf.copy_(torch.argsort(self.w_keys).to(torch.int32))
        valid = ((self.w_keys >> 32) & 0xFFFFFFFF).ne(0xFFFFFFFE)
        self.valid_buf.copy_(valid.sum().to(torch.int32).reshape(1))

    # ---- one workflow tick ---------------------------------------------------
    def _tick_device_body(self) -> None:
        """The fixed kernel sequence of one tick (no host decisions): this is
        what gets hipGraph-captured on GPU (world == 1). The device tick
        counter increments in-graph; collectives stay outside (world > 1
        runs the same body eagerly with the exchanges inline)."""
        ext = self.ext
        cap, world, Wd = self.pad_cap, self.world, self.W
        self.tick_buf += 1
        if self.device_conditions:
            # predicates first: condition bits for the sweep to commit, and
            # false guards -> SKIPPED (see "conditions decided on the device")
            ext.wf_cond_eval(self.step_state, self.deps_mask, self.step_kind,
                             self.run_life, self.run_active, self.run_tmpl,
                             self.tmpl_cond, self.tmpl_cond_mask, self.run_input,
                             self.step_out, self.cond_bits, self.cond_counts,
                             self.input_words)
        # sweep: readiness -> dispatch list + fresh approval holds
        self.disp_count.zero_()
        self.appr_count.zero_()
        ext.wf_sweep(self.step_state, self.deps_mask, self.n_steps,
                     self.run_active, self.step_kind, self.cond_bits,
                     self.next_ready, self.tick_buf,
                     self.disp_runs, self.disp_steps, self.disp_count,
                     self.appr_runs, self.appr_steps, self.appr_count)
        if self.external:
            # open / expire / close approval holds from the run table itself
            # (the sweep's fresh-hold list is not read in this mode)
            self.hold_open.zero_()
            ext.wf_hold_scan(self.step_state, self.n_steps, self.run_life,
                             self.run_active, self.run_gen, self.tick_buf,
                             self.hold_ttl, self.hold_mask, self.hold_tick,
                             self.hold_gen, self.hold_counts, self.hold_open)

        # expand into the child arena, spread-routed over the global order
        self.child_count.zero_()
        ext.wf_expand(self.disp_runs, self.disp_steps, self.disp_count,
                      self.step_state, self.children_todo, self.children_out,
                      self.max_parallel,
                      self.child_tag, self.child_seq, self.child_widx,
                      self.child_count, self.children_emitted,
                      self.dispatch_tick, self.tick_buf,
                      self.order_buf, self.valid_buf)
        if self.device_conditions:
            # a child's payload is (run input, ordinal, step): its result is
            # then a function of those alone
            ext.wf_child_payload(self.child_tag, self.child_seq, self.child_count,
                                 self.run_input, self.child_payload,
                                 self.input_words, Wd)

        # K2 load view + routing order refresh
        ext.worker_precompute_into(self.w_pool, self.w_active, self.w_maxp,
                                   self.w_cpu, self.w_gpu, self.w_keys)
        self._heartbeats()

        # pack per destination: redeliveries first, then fresh children
        self.rq_prev_widx.copy_(self.rq_widx)
        self.rq_prev_attempts.copy_(self.rq_attempts)
        self.rq_prev_count.copy_(self.rq_count)
        self.rq_prev_payload.copy_(self.rq_payload)
        self.rq_prev_tag.copy_(self.rq_tag)
        self.rq_prev_seq.copy_(self.rq_seq)
        self.rq_count.zero_()
        self.dead_count.zero_()
        self.pad_send_cnt.zero_()
        ext.pack_requeue(self.rq_prev_widx, self.rq_prev_attempts, self.rq_prev_count,
                         self.pad_send_slots, self.pad_send_widx, self.pad_send_cnt,
                         self.NWL, cap,
                         self.rq_src, self.rq_widx, self.rq_attempts,
                         self.rq_count, self.rq_dead,
                         self.dead_src, self.dead_count)
        ext.pack_by_dest(self._iota, self.child_widx, self.child_count,
                         self.pad_send_slots, self.pad_send_widx, self.pad_send_cnt,
                         self.NWL, cap, self.CB,
                         self.rq_src, self.rq_widx, self.rq_attempts,
                         self.rq_count, self.rq_dead,
                         self.dead_src, self.dead_count)
        self.pad_send_cnt.clamp_(max=cap)
        ext.gather_payload_padded(self.child_payload, self.rq_prev_payload,
                                  self.pad_send_slots, self.pad_send_cnt,
                                  self.pad_send_payload, Wd, cap, world)
        # park-survival: payload + tag of newly parked children
        ext.materialize_rq_payload(self.child_payload, self.rq_prev_payload,
                                   self.rq_src, self.rq_count,
                                   self.rq_payload, Wd)
        ext.materialize_rq_payload(self.child_tag, self.rq_prev_tag,
                                   self.rq_src, self.rq_count,
                                   self.rq_tag, 1)
        ext.materialize_rq_payload(self.child_seq, self.rq_prev_seq,
                                   self.rq_src, self.rq_count,
                                   self.rq_seq, 1)

        # dispatch across ranks + device worker execution + results home
        self._exchange_out()
        ext.echo_padded(self.pad_recv_payload, self.pad_recv_cnt, self.pad_res,
                        self.pad_sums, Wd, cap, world)
        self.w_active_local.zero_()
        ext.load_feedback_padded(self.pad_recv_widx, self.pad_recv_cnt,
                                 self.w_active_local, cap, world)
        self._exchange_back()

        # owner-rank application + aggregation + roll-up
        if self.device_conditions:
            ext.wf_apply_out(self.pad_send_slots, self.pad_send_cnt, self.child_tag,
                             self.child_seq, self.rq_prev_tag, self.rq_prev_seq,
                             self.children_done, self.children_fail,
                             self.children_out, self.pad_sums_back, self.step_out,
                             self.fail_ppt, self.drop_ppt, cap, world)
        else:
            ext.wf_apply(self.pad_send_slots, self.pad_send_cnt, self.child_tag,
                         self.child_seq, self.rq_prev_tag, self.rq_prev_seq,
                         self.children_done, self.children_fail,
                         self.children_out, self.fail_ppt, self.drop_ppt, cap, world)
        ext.wf_apply_dead(self.dead_src, self.dead_count, self.child_tag,
                          self.rq_prev_tag, self.children_fail, self.children_out)
        # K4-WF: steps whose children were lost (worker crash) time out and
        # the remainder retries with backoff (reconciler.go:88-144)
        if self.step_policy:
            # the same two stages in one pass, with each step's own retry,
            # backoff and timeout (see "per-step policy")
            ext.wf_settle(self.step_state, self.step_attempts, self.children_todo,
                          self.children_out, self.children_fail, self.max_parallel,
                          self.next_ready, self.dispatch_tick, self.run_life,
                          self.run_tmpl, self.tmpl_policy, self.tmpl_timeout,
                          self.tick_buf, self.timeout_count, self.retry_count)
        else:
            ext.wf_timeout_scan(self.step_state, self.children_out,
                                self.children_fail, self.dispatch_tick,
                                self.tick_buf, self.timeout_cutoff, self.timeout_count)
            ext.wf_commit(self.step_state, self.step_attempts, self.children_todo,
                          self.children_out, self.children_done, self.children_fail,
                          self.max_parallel,
                          self.next_ready, self.tick_buf, self.max_retries,
                          self.retry_count)
        ext.wf_status(self.step_state, self.n_steps, self.run_active,
                      self.run_state, self.wf_counts)
        if self.event_cap is not None:
            self._journal(0)
        if self._appr_h_count is not None and not self.external:
            # stream-ordered async D2H of the approval count into pinned
            # memory: the host polls it with event.query() instead of a
            # blocking sync every tick (the grant hop already tolerates a
            # tick of lag)
            self._appr_h_count.copy_(self.appr_count, non_blocking=True)

    def _graph_allowed(self) -> bool:
        return self.device.type == "cuda" and self.world == 1 \
            and not os.environ.get("CORDUM_WF_NO_GRAPH")

    def _capture_tick(self) -> None:
        """Eager warm-up (allocator steady state), then capture of the tick
        body into _wf_graph, () if that fails. The warm-up ran for real: the
        counters an option registered are put back afterwards."""
        saved = [(t, t.clone()) for t in self._counters]
        for _ in range(2):
            self._tick_device_body()
        torch.cuda.synchronize(self.device)
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._tick_device_body()
            self._wf_graph = g
        except Exception as e:
            print(f"[cordum] wf-graph capture failed, running eager: {e!r}",
                  file=sys.stderr)
            self._wf_graph = ()
        for t, v in saved:
            t.copy_(v)
        torch.cuda.synchronize(self.device)

    def _run_body(self) -> None:
        """One tick body: the captured graph where there is one, else eager."""
        if not self.dynamic:
            # static mode captures on its first tick; the warm-up changed the
            # run tables too, so the wave is reset and the triggering tick
            # replays as tick 0 of a fresh one. (Dynamic mode captured at
            # construction, on the empty table.)
            if not self._graph_allowed():
                return self._tick_device_body()
            if self._wf_graph is None:
                self._capture_tick()
                self.reset_runs()
        if self._wf_graph:
            self._wf_graph.replay()
        else:
            self._tick_device_body()

    def _drain_approvals(self) -> None:
        na = int(self._appr_h_count[0]) if self._appr_h_count is not None \
            else int(self.appr_count.cpu()[0])
        if na > 0:
            na = min(na, self.NR)
            self._pending_grants.append(
                (self.appr_runs[:na].cpu().clone(), self.appr_steps[:na].cpu().clone()))

    def tick(self) -> None:
        ext = self.ext
        self._tick += 1

        # external approvals have no host hop: holds wait in the tables for
        # decide(). Nothing is granted, drained or polled here.
        if not self.external:
            # a drain deferred from last tick (its D2H event was still in
            # flight) MUST land before this tick's body overwrites the approval
            # ring — by now the event has long completed, so this rarely blocks
            if getattr(self, "_appr_deferred", False):
                self._appr_ev.synchronize()
                self._drain_approvals()
                self._appr_deferred = False

            # host hop: approvals drained LAST tick are granted now (1-tick
            # admin latency, like the reference's async approve endpoint)
            if self._pending_grants:
                runs, steps = self._pending_grants.pop()
                n = runs.shape[0]
                v = torch.full((n,), self.approval_verdict, dtype=torch.uint8,
                               device=self.device)
                ext.wf_grant(runs.to(self.device), steps.to(self.device), v, n,
                             self.step_state)

        self._run_body()
        self._refresh_order()
        if self.external:
            return

        # drain fresh approval holds for next tick's grant. On GPU the count
        # arrives via the in-body pinned D2H; poll non-blockingly — if the
        # tick is still in flight, defer the drain to the top of the next
        # tick (before the ring is overwritten) instead of stalling here
        if self._appr_h_count is not None:
            self._appr_ev.record()
            if not self._appr_ev.query():
                self._appr_deferred = True
                return
        self._drain_approvals()

    # ---- continuous mode (config #5) ----------------------------------------
    def _ensure_tmpl_dev(self):
        if not hasattr(self, "_tmpl_dev"):
            self._tmpl_dev = {k: v.to(self.device) for k, v in self._tmpl.items()}
        return self._tmpl_dev

    def _readmit(self, filter_state: int) -> None:
        t = self._ensure_tmpl_dev()
        self.ext.wf_readmit(self.run_active, self.run_state, self.n_steps,
                            self.step_state, self.step_attempts,
                            self.children_todo, self.children_out,
                            self.children_done, self.children_fail,
                            self.children_emitted, self.next_ready,
                            self.dispatch_tick, t["children_todo"],
                            t["next_ready"], filter_state, self.admit_count)

    def readmit_succeeded(self) -> None:
        """Terminal SUCCEEDED runs re-enter from the creation template so the
        table stays full (config #5 'hold 1M concurrent runs')."""
        self._require_dynamic(False, "readmit_succeeded")
        self._readmit(WFS_SUCCEEDED)

    def drain_failed_to_dlq(self, dlq=None) -> int:
        """Host DLQ drain (dlq_store.go analog): record every FAILED run,
        then re-admit those rows through the same template reset. Returns
        the number drained; the caller's DLQ bookkeeping must reconcile
        exactly with the device failed counter at the end of a soak."""
        self._require_dynamic(False, "drain_failed_to_dlq")
        failed = (self.run_state == WFS_FAILED) & (self.run_active == 0)
        ids = torch.nonzero(failed).flatten()
        n = int(ids.numel())
        if n and dlq is not None:
            from ..store.dlq_store import DLQEntry

            gen = int(self.admit_count.cpu()[0])
            for r in ids.cpu().tolist():
                dlq.add(DLQEntry(job_id=f"run-{r}-g{gen}", topic="job.soak",
                                 status="JOB_STATUS_FAILED",
                                 reason="max retries exceeded (soak)",
                                 reason_code="max_retries_exceeded",
                                 last_state="FAILED",
                                 attempts=self.max_retries))
        if n:
            self._readmit(WFS_FAILED)
        return n

    # ---- wave driver ---------------------------------------------------------
    def counts(self) -> tuple:
        c = self.wf_counts.cpu()
        return int(c[0]), int(c[1])

    def active(self) -> int:
        return int(self.run_active.sum().cpu())

    def run_wave(self, max_ticks: int = 256) -> WfStats:
        """Admit the full run wave and tick until every run is terminal."""
        self._require_dynamic(False, "run_wave")
        t0 = time.perf_counter()
        self.reset_runs()
        start_ok, start_fail = self.counts()
        ticks = 0
        # world>1: all ranks must tick in lockstep (collectives); keep
        # ticking until every rank's runs are done
        while ticks < max_ticks:
            self.tick()
            ticks += 1
            if ticks % 4 == 0:
                done = self.active() == 0
                if self.world > 1:
                    t = torch.tensor([0 if done else 1],
                                     dtype=torch.int64, device=self.device
                                     if self.device.type == "cuda" else "cpu")
                    dist.all_reduce(t)
                    done = int(t.item()) == 0
                if done:
                    break
        ok, fail = self.counts()
        return WfStats(runs_succeeded=ok - start_ok, runs_failed=fail - start_fail,
                       ticks=ticks, wall_s=time.perf_counter() - t0)
