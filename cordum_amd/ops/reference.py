"""Torch reference implementations of every HIP kernel.

These are the numerics oracles for the GPU tests (plain torch, fp32/int
exact) and the CPU execution path for environments without a GPU. Each
function mirrors its kernel in cordum_amd/ops/hip/cordum_kernels.hip
bit-for-bit (deterministic tie-breaks included).
"""
from __future__ import annotations


import torch

from ..protocol.states import transition_lut

OVERLOAD = 0.9


def least_loaded_pick_ref(
    w_pool: torch.Tensor,
    w_active: torch.Tensor,
    w_maxp: torch.Tensor,
    w_cpu: torch.Tensor,
    w_gpu: torch.Tensor,
    w_labels: torch.Tensor,
    j_poolmask: torch.Tensor,
    j_labels: torch.Tensor,
) -> torch.Tensor:
    """K2 oracle. Returns int32 [J]: worker idx, -1 no_workers, -2 overloaded."""
    NW = w_pool.shape[0]
    NJ = j_poolmask.shape[0]
    if NJ == 0:
        return torch.empty(0, dtype=torch.int32)
    pool_ok = ((j_poolmask.unsqueeze(1) >> w_pool.clamp(0, 63).unsqueeze(0)) & 1).bool()
    pool_ok &= (w_pool >= 0).unsqueeze(0) & (w_pool < 64).unsqueeze(0)
    labels_ok = (j_labels.unsqueeze(1) & ~w_labels.unsqueeze(0)) == 0
    eligible = pool_ok & labels_ok  # [J, W]

    util_over = (w_maxp > 0) & (w_active.float() / w_maxp.clamp(min=1).float() >= OVERLOAD)
    over = util_over | (w_cpu >= 90) | (w_gpu >= 90)  # [W]
    usable = eligible & ~over.unsqueeze(0)

    score = w_active.float() + w_cpu * 0.01 + w_gpu * 0.01
    key = (score.view(torch.int32).to(torch.int64) << 32) | torch.arange(NW, dtype=torch.int64)
    big = torch.iinfo(torch.int64).max
    keys = torch.where(usable, key.unsqueeze(0).expand(NJ, NW), torch.full((NJ, NW), big, dtype=torch.int64))
    best = keys.min(dim=1).values
    pick = (best & 0xFFFFFFFF).to(torch.int32)

    n_eligible = eligible.sum(dim=1)
    n_over = (eligible & over.unsqueeze(0)).sum(dim=1)
    none = best == big
    all_over = none & (n_eligible > 0) & (n_over == n_eligible)
    out = torch.where(none, torch.full_like(pick, -1), pick)
    out = torch.where(all_over, torch.full_like(pick, -2), out)
    return out


def worker_precompute_ref(w_pool, w_active, w_maxp, w_cpu, w_gpu) -> torch.Tensor:
    """K2a oracle: per-worker (score, idx) key; overloaded -> OVERLOADED tag."""
    NW = w_pool.shape[0]
    idx = torch.arange(NW, dtype=torch.int64)
    util_over = (w_maxp > 0) & (w_active.float() / w_maxp.clamp(min=1).float() >= OVERLOAD)
    over = util_over | (w_cpu >= 90) | (w_gpu >= 90)
    score = w_active.float() + w_cpu * 0.01 + w_gpu * 0.01
    key = (score.view(torch.int32).to(torch.int64) << 32) | idx
    # 0xFFFFFFFE00000000 as signed int64 (torch has no uint64)
    over_key = torch.tensor(0xFFFFFFFE00000000 - (1 << 64), dtype=torch.int64) | idx
    return torch.where(over, over_key, key)


def least_loaded_pick_keys_ref(
    w_pool: torch.Tensor,
    w_keys: torch.Tensor,
    w_labels: torch.Tensor,
    j_poolmask: torch.Tensor,
    j_labels: torch.Tensor,
) -> torch.Tensor:
    """K2 oracle over precomputed keys (must agree with least_loaded_pick_ref)."""
    NW = w_pool.shape[0]
    NJ = j_poolmask.shape[0]
    if NJ == 0:
        return torch.empty(0, dtype=torch.int32)
    pool_ok = ((j_poolmask.unsqueeze(1) >> w_pool.clamp(0, 63).unsqueeze(0)) & 1).bool()
    pool_ok &= (w_pool >= 0).unsqueeze(0) & (w_pool < 64).unsqueeze(0)
    labels_ok = (j_labels.unsqueeze(1) & ~w_labels.unsqueeze(0)) == 0
    eligible = pool_ok & labels_ok
    over = ((w_keys >> 32) & 0xFFFFFFFF) == 0xFFFFFFFE
    usable = eligible & ~over.unsqueeze(0)
    big = torch.iinfo(torch.int64).max
    keys = torch.where(usable, w_keys.unsqueeze(0).expand(NJ, NW), torch.full((NJ, NW), big, dtype=torch.int64))
    best = keys.min(dim=1).values
    pick = (best & 0xFFFFFFFF).to(torch.int32)
    n_eligible = eligible.sum(dim=1)
    n_over = (eligible & over.unsqueeze(0)).sum(dim=1)
    none = best == big
    all_over = none & (n_eligible > 0) & (n_over == n_eligible)
    out = torch.where(none, torch.full_like(pick, -1), pick)
    out = torch.where(all_over, torch.full_like(pick, -2), out)
    return out


def echo_execute_indexed_ref(ctx_arena, slots, res_arena, res_sum, stride: int):
    N = ctx_arena.numel() // stride
    ctx = ctx_arena.view(N, stride)
    res = res_arena.view(N, stride)
    sl = slots.long()
    res[sl] = ctx[sl]
    sums = ctx[sl].to(torch.int64).sum(dim=1).remainder(1 << 32).to(torch.int32)
    res_sum[sl] = sums
    return res_sum


def apply_transitions_ref(
    states: torch.Tensor,
    attempts: torch.Tensor,
    deadlines: torch.Tensor,
    slots: torch.Tensor,
    to_states: torch.Tensor,
) -> torch.Tensor:
    """K5 oracle (sequential; duplicate slots in one batch are applied in
    order, matching the kernel's per-slot independence assumption — the
    pipeline never puts the same slot twice in one batch)."""
    lut = torch.tensor(transition_lut(), dtype=torch.uint8)
    ok = torch.zeros(slots.shape[0], dtype=torch.uint8)
    for i in range(slots.shape[0]):
        s = int(slots[i])
        frm = int(states[s])
        to = int(to_states[i])
        if lut[frm, to]:
            ok[i] = 1
            states[s] = to
            if to == 3 and frm != 3:
                attempts[s] += 1
            if to >= 6:
                deadlines[s] = torch.iinfo(torch.int64).max
    return ok


def deadline_scan_ref(
    states: torch.Tensor,
    deadlines: torch.Tensor,
    updated_at: torch.Tensor,
    now_us: int,
    dispatch_cutoff_us: int,
    running_cutoff_us: int,
) -> torch.Tensor:
    """K4 oracle: sorted slot indices due for TIMEOUT."""
    active = (states >= 1) & (states <= 5)
    expired = active & (deadlines <= now_us)
    expired |= (states == 4) & (updated_at <= dispatch_cutoff_us)
    expired |= (states == 5) & (updated_at <= running_cutoff_us)
    return torch.nonzero(expired, as_tuple=False).flatten().to(torch.int32)


def echo_execute_ref(ctx_arena: torch.Tensor, res_arena: torch.Tensor, stride: int) -> torch.Tensor:
    """Echo worker oracle: copy payload, return per-job uint32 checksum."""
    B = ctx_arena.numel() // stride
    ctx = ctx_arena.view(B, stride)
    res_arena.view(B, stride).copy_(ctx)
    return ctx.to(torch.int64).sum(dim=1).remainder(1 << 32).to(torch.int32)


# device run-table step-state encoding (K3): 0 pending, 1 running, 2 waiting,
# 3 succeeded, 4 failed, 5 cancelled, 6 timed_out
RUN_STEP_PENDING, RUN_STEP_SUCCEEDED = 0, 3


def run_readiness_ref(step_state, deps_mask, n_steps, run_active):
    """K3 oracle: per-run 64-bit ready mask + (run, step) dispatch pairs."""
    NR = step_state.shape[0]
    ready = torch.zeros(NR, dtype=torch.int64)
    pairs = []
    for r in range(NR):
        if not bool(run_active[r]):
            continue
        ns = int(n_steps[r])
        succeeded = 0
        for t in range(ns):
            if int(step_state[r, t]) == RUN_STEP_SUCCEEDED:
                succeeded |= 1 << t
        m = 0
        for s_i in range(ns):
            if int(step_state[r, s_i]) != RUN_STEP_PENDING:
                continue
            need = int(deps_mask[r, s_i]) & ((1 << 64) - 1)
            if need & ~succeeded & ((1 << 64) - 1):
                continue
            m |= 1 << s_i
            pairs.append((r, s_i))
        ready[r] = m - (1 << 64) if m >= (1 << 63) else m
    return ready, pairs


# -- padded cross-rank dispatch references ------------------------------------


RQ_MAX_DELIVER = 5


def _rq_dead_mark(rq_dead, dead_src, dead_count, src: int) -> None:
    rq_dead[0] += 1
    if dead_src is not None:
        dp = int(dead_count[0])
        dead_count[0] = dp + 1
        if dp < dead_src.shape[0]:
            dead_src[dp] = src


def _rq_park(rq_src, rq_widx, rq_attempts, rq_count, rq_dead,
             src: int, widx: int, attempts: int,
             dead_src=None, dead_count=None) -> None:
    p = int(rq_count[0])
    rq_count[0] = p + 1
    if p < rq_src.shape[0]:
        rq_src[p] = src
        rq_widx[p] = widx
        rq_attempts[p] = attempts
    else:
        _rq_dead_mark(rq_dead, dead_src, dead_count, src)


def pack_by_dest_ref(routable_slots, routable_widx, routable_count,
                     send_slots, send_widx, send_cnt, nwl: int, cap: int,
                     rq_src, rq_widx, rq_attempts, rq_count, rq_dead,
                     dead_src=None, dead_count=None):
    n = int(routable_count[0])
    for i in range(n):
        slot = int(routable_slots[i])
        widx = int(routable_widx[i])
        dest = widx // nwl
        pos = int(send_cnt[dest])
        send_cnt[dest] += 1
        if pos < cap:
            send_slots[dest * cap + pos] = slot
            send_widx[dest * cap + pos] = widx % nwl
        else:
            _rq_park(rq_src, rq_widx, rq_attempts, rq_count, rq_dead,
                     slot, widx, 1, dead_src, dead_count)


def pack_requeue_ref(rq_prev_widx, rq_prev_attempts, rq_prev_count,
                     send_slots, send_widx, send_cnt, nwl: int, cap: int,
                     rq_src, rq_widx, rq_attempts, rq_count, rq_dead,
                     dead_src=None, dead_count=None):
    n = min(int(rq_prev_count[0]), int(rq_prev_widx.shape[0]))
    for j in range(n):
        widx = int(rq_prev_widx[j])
        dest = widx // nwl
        pos = int(send_cnt[dest])
        send_cnt[dest] += 1
        if pos < cap:
            send_slots[dest * cap + pos] = -1 - j
            send_widx[dest * cap + pos] = widx % nwl
        else:
            att = int(rq_prev_attempts[j]) + 1
            if att > RQ_MAX_DELIVER:
                _rq_dead_mark(rq_dead, dead_src, dead_count, -1 - j)
            else:
                _rq_park(rq_src, rq_widx, rq_attempts, rq_count, rq_dead,
                         -1 - j, widx, att, dead_src, dead_count)


def materialize_rq_payload_ref(payload, rq_prev_payload, rq_src, rq_count,
                               rq_payload, stride: int):
    pl = payload.view(-1, stride)
    prev = rq_prev_payload.view(-1, stride)
    dst = rq_payload.view(-1, stride)
    n = min(int(rq_count[0]), int(rq_src.shape[0]))
    for j in range(n):
        s = int(rq_src[j])
        dst[j] = pl[s] if s >= 0 else prev[-1 - s]


def gather_payload_padded_ref(payload, rq_prev_payload, send_slots, send_cnt,
                              send_payload, stride: int, cap: int, world: int):
    pl = payload.view(-1, stride)
    prev = rq_prev_payload.view(-1, stride)
    sp = send_payload.view(-1, stride)
    for r in range(world):
        for e in range(int(send_cnt[r])):
            i = r * cap + e
            s = int(send_slots[i])
            sp[i] = pl[s] if s >= 0 else prev[-1 - s]


def echo_padded_ref(recv_payload, recv_cnt, res_arena, res_sums,
                    stride: int, cap: int, world: int):
    rp = recv_payload.view(-1, stride)
    ra = res_arena.view(-1, stride)
    for r in range(world):
        for e in range(int(recv_cnt[r])):
            i = r * cap + e
            ra[i] = rp[i]
            res_sums[i] = int(rp[i].to(torch.int64).sum()) % (1 << 32) - (
                (1 << 32) if int(rp[i].to(torch.int64).sum()) % (1 << 32) >= (1 << 31) else 0
            )


def apply_transitions_padded_ref(states, attempts, deadlines, slots_pad, cnt,
                                 to_state: int, cap: int, world: int):
    from ..protocol.states import transition_lut

    lut = transition_lut()
    for r in range(world):
        for e in range(int(cnt[r])):
            slot = int(slots_pad[r * cap + e])
            if slot < 0:  # redelivered entry: its batch slot was recycled
                continue
            frm = int(states[slot])
            if lut[frm][to_state]:
                states[slot] = to_state
                if to_state == 3 and frm != 3:
                    attempts[slot] += 1
                if to_state >= 6:
                    deadlines[slot] = torch.iinfo(torch.int64).max


def load_feedback_padded_ref(recv_widx, recv_cnt, w_active_local, cap: int, world: int):
    for r in range(world):
        for e in range(int(recv_cnt[r])):
            w_active_local[int(recv_widx[r * cap + e])] += 1


# -- K3-WF device workflow engine references ----------------------------------
# States/kinds mirror the kernel constants (cordum_kernels.hip K3-WF section).

WFS_PENDING, WFS_DISPATCHED, WFS_WAITING = 0, 1, 2
WFS_SUCCEEDED, WFS_FAILED, WFS_SKIPPED = 3, 4, 5
WFK_WORKER, WFK_FOR_EACH, WFK_APPROVAL, WFK_CONDITION, WFK_DELAY = 0, 1, 2, 3, 4


def wf_sweep_ref(step_state, deps_mask, n_steps, run_active, step_kind,
                 cond_bits, next_ready, tick,
                 disp_runs, disp_steps, disp_count,
                 appr_runs, appr_steps, appr_count):
    tick = int(tick[0]) if hasattr(tick, "__getitem__") else int(tick)
    NR = int(n_steps.shape[0])
    cap, acap = int(disp_runs.shape[0]), int(appr_runs.shape[0])
    for run in range(NR):
        if not int(run_active[run]):
            continue
        ns = int(n_steps[run])
        base = run * 64
        satisfied = 0
        for t in range(ns):
            if int(step_state[base + t]) in (WFS_SUCCEEDED, WFS_SKIPPED):
                satisfied |= 1 << t
        for s in range(ns):
            if int(step_state[base + s]) != WFS_PENDING:
                continue
            need = int(deps_mask[base + s]) & ((1 << 64) - 1)
            if need & ~satisfied & ((1 << 64) - 1):
                continue
            if int(next_ready[base + s]) > tick:
                continue
            kind = int(step_kind[base + s])
            if kind in (WFK_WORKER, WFK_FOR_EACH):
                pos = int(disp_count[0])
                disp_count[0] = pos + 1
                if pos < cap:
                    disp_runs[pos] = run
                    disp_steps[pos] = s
            elif kind == WFK_APPROVAL:
                step_state[base + s] = WFS_WAITING
                pos = int(appr_count[0])
                appr_count[0] = pos + 1
                if pos < acap:
                    appr_runs[pos] = run
                    appr_steps[pos] = s
            elif kind == WFK_CONDITION:
                step_state[base + s] = (
                    WFS_SUCCEEDED if (int(cond_bits[run]) >> s) & 1 else WFS_SKIPPED)
            elif kind == WFK_DELAY:
                step_state[base + s] = WFS_SUCCEEDED


def wf_expand_ref(disp_runs, disp_steps, disp_count, step_state,
                  children_todo, children_out, max_parallel, child_tag,
                  child_seq, child_widx, child_count, children_emitted,
                  dispatch_tick, tick, order, valid_count):
    tick = int(tick[0]) if hasattr(tick, "__getitem__") else int(tick)
    CB = int(child_tag.shape[0])
    n = min(int(disp_count[0]), int(disp_runs.shape[0]))
    V = min(max(1, int(valid_count[0])), 1024)
    for e in range(n):
        run, step = int(disp_runs[e]), int(disp_steps[e])
        rs = run * 64 + step
        todo = int(children_todo[rs])
        # for_each max_parallel windowing (dataflow_test.go:71 semantics)
        maxp = int(max_parallel[rs])
        if maxp > 0:
            room = maxp - int(children_out[rs])
            if room < todo:
                todo = max(0, room)
        # monotone per-step emission counter -> deterministic per-child
        # ordinal stream (matches the kernel; retries get fresh ordinals)
        seq0 = int(children_emitted[rs])
        if todo <= 0:
            if int(children_out[rs]) > 0:
                step_state[rs] = WFS_DISPATCHED
            continue
        base = int(child_count[0])
        if base + todo > CB:
            continue  # arena full: retry next sweep
        child_count[0] = base + todo
        step_state[rs] = WFS_DISPATCHED
        children_out[rs] += todo
        children_emitted[rs] += todo
        children_todo[rs] -= todo
        dispatch_tick[rs] = tick
        tag = run * 64 + step
        for k in range(todo):
            child_tag[base + k] = tag
            child_seq[base + k] = seq0 + k
            child_widx[base + k] = int(order[(base + k) % V])


def _wf_mix(x: int) -> int:
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def wf_fail_hash(tag: int, seq: int) -> int:
    return _wf_mix((tag * 2654435761 ^ seq * 40503) & 0xFFFFFFFF)


def wf_drop_hash(tag: int, seq: int) -> int:
    return _wf_mix((tag * 0x85EBCA6B ^ seq * 0xC2B2AE35) & 0xFFFFFFFF)


def wf_apply_ref(send_slots, send_cnt, child_tag, child_seq, rq_prev_tag,
                 rq_prev_seq, children_done, children_fail, children_out,
                 fail_ppt: int, drop_ppt: int, cap: int, world: int,
                 sums_back=None, step_out=None):
    for r in range(world):
        for e in range(min(int(send_cnt[r]), cap)):
            i = r * cap + e
            s = int(send_slots[i])
            tag = int(child_tag[s]) if s >= 0 else int(rq_prev_tag[-1 - s])
            seq = int(child_seq[s]) if s >= 0 else int(rq_prev_seq[-1 - s])
            if wf_drop_hash(tag, seq) % 1000 < drop_ppt:
                continue  # lost result: K4-WF timeout scan recovers it
            if wf_fail_hash(tag, seq) % 1000 < fail_ppt:
                children_fail[tag] += 1
            else:
                children_done[tag] += 1
                if step_out is not None:    # wf_apply_out: the step's output word
                    v = (int(step_out[tag]) + int(sums_back[i])) & 0xFFFFFFFF
                    step_out[tag] = v - (1 << 32) if v >= (1 << 31) else v
            children_out[tag] -= 1


def wf_apply_dead_ref(dead_src, dead_count, child_tag, rq_prev_tag,
                      children_fail, children_out):
    n = min(int(dead_count[0]), int(dead_src.shape[0]))
    for i in range(n):
        s = int(dead_src[i])
        tag = int(child_tag[s]) if s >= 0 else int(rq_prev_tag[-1 - s])
        children_fail[tag] += 1
        children_out[tag] -= 1


def wf_commit_ref(step_state, step_attempts, children_todo, children_out,
                  children_done, children_fail, max_parallel, next_ready,
                  tick, max_retries: int, retry_count=None):
    tick = int(tick[0]) if hasattr(tick, "__getitem__") else int(tick)
    for i in range(int(step_state.numel())):
        if int(step_state[i]) != WFS_DISPATCHED:
            continue
        if int(children_out[i]) != 0:
            # window slide / arena resume: more work and room -> re-open
            if int(children_todo[i]) > 0 and (
                int(max_parallel[i]) == 0
                or int(children_out[i]) < int(max_parallel[i])
            ):
                step_state[i] = WFS_PENDING
            continue
        fail = int(children_fail[i])
        if fail > 0:
            if int(step_attempts[i]) < max_retries:
                step_attempts[i] += 1
                children_todo[i] += fail
                children_fail[i] = 0
                next_ready[i] = tick + min(1 << int(step_attempts[i]), 16)
                step_state[i] = WFS_PENDING
                if retry_count is not None:
                    retry_count[0] += fail
            else:
                step_state[i] = WFS_FAILED
        elif int(children_todo[i]) > 0:
            step_state[i] = WFS_PENDING
        else:
            step_state[i] = WFS_SUCCEEDED


def wf_status_ref(step_state, n_steps, run_active, run_state, counts):
    NR = int(n_steps.shape[0])
    for run in range(NR):
        if not int(run_active[run]):
            continue
        ns = int(n_steps[run])
        vals = [int(step_state[run * 64 + s]) for s in range(ns)]
        if any(v == WFS_FAILED for v in vals):
            run_active[run] = 0
            run_state[run] = WFS_FAILED
            counts[1] += 1
        elif all(v in (WFS_SUCCEEDED, WFS_SKIPPED) for v in vals):
            run_active[run] = 0
            run_state[run] = WFS_SUCCEEDED
            counts[0] += 1


def wf_grant_ref(grant_runs, grant_steps, verdicts, n: int, step_state):
    for i in range(n):
        rs = int(grant_runs[i]) * 64 + int(grant_steps[i])
        if int(step_state[rs]) == WFS_WAITING:
            step_state[rs] = WFS_SUCCEEDED if int(verdicts[i]) else WFS_FAILED


def wf_timeout_scan_ref(step_state, children_out, children_fail,
                        dispatch_tick, tick, cutoff: int, timeout_count):
    tick = int(tick[0]) if hasattr(tick, "__getitem__") else int(tick)
    for i in range(int(step_state.numel())):
        if int(step_state[i]) != WFS_DISPATCHED:
            continue
        lost = int(children_out[i])
        if lost <= 0 or int(dispatch_tick[i]) > tick - cutoff:
            continue
        children_fail[i] += lost
        children_out[i] = 0
        timeout_count[0] += lost


def wf_readmit_ref(run_active, run_state, n_steps, step_state, step_attempts,
                   children_todo, children_out, children_done, children_fail,
                   children_emitted, next_ready, dispatch_tick,
                   todo_tmpl, nready_tmpl, filter_state: int, admit_count):
    NR = int(n_steps.shape[0])
    for run in range(NR):
        if int(run_active[run]) or int(run_state[run]) != filter_state:
            continue
        for s in range(int(n_steps[run])):
            i = run * 64 + s
            step_state[i] = WFS_PENDING
            step_attempts[i] = 0
            children_todo[i] = int(todo_tmpl[i])
            children_out[i] = 0
            children_done[i] = 0
            children_fail[i] = 0
            children_emitted[i] = 0
            next_ready[i] = int(nready_tmpl[i])
            dispatch_tick[i] = 0
        run_state[run] = 0
        run_active[run] = 1
        admit_count[0] += 1


# -- K3-WF run lifecycle references (dynamic mode: admit / cancel / retire) ----
# Life states of a run slot; a cancelled run or step is WFS_CANCELLED, a code
# the tick kernels never act on.

WFS_CANCELLED = 6
WFL_FREE, WFL_LIVE, WFL_DRAINING = 0, 1, 2


def wf_admit_ref(req_tmpl, req_cond, req_fanout,
                 tmpl_deps, tmpl_kind, tmpl_todo, tmpl_maxp, tmpl_delay,
                 tmpl_nsteps,
                 step_state, step_attempts, deps_mask, step_kind,
                 children_todo, max_parallel, children_out, children_done,
                 children_fail, children_emitted, next_ready, dispatch_tick,
                 n_steps, cond_bits, run_state, run_active, run_life, run_gen,
                 tick, free_mask, blk_scan, out_slot, out_gen, admit_count):
    """Request i takes the i-th lowest FREE slot; requests past the free count
    get slot -1. free_mask / blk_scan are the kernel's workspaces: unused."""
    n = int(req_tmpl.shape[0])
    if n <= 0:
        return
    NR = int(n_steps.shape[0])
    TC = int(tmpl_nsteps.shape[0])
    tick1 = int(tick[0]) + 1  # the run's first tick
    free = torch.nonzero(run_life[:NR] == WFL_FREE).flatten().tolist()  # ascending
    admit_count[0] += min(n, len(free))
    for i in range(n):
        if i >= len(free):
            out_slot[i] = -1
            out_gen[i] = 0
            continue
        slot = free[i]
        tid = int(req_tmpl[i])
        known = 0 <= tid < TC  # the host rejects the rest
        ns = int(tmpl_nsteps[tid]) if known else 0
        fan = int(req_fanout[i])
        # the whole 64-entry row, one element per step (the kernel's lanes):
        # steps s < ns from the template, the rest zero
        row = slice(slot * 64, slot * 64 + 64)
        trow = slice((tid if known else 0) * 64, (tid if known else 0) * 64 + 64)
        inside = torch.arange(64) < ns
        kind = torch.where(inside, tmpl_kind[trow], 0)
        todo = tmpl_todo[trow]
        if fan > 0:
            todo = torch.where(kind == WFK_FOR_EACH, fan, todo)
        step_state[row] = WFS_PENDING
        step_attempts[row] = 0
        deps_mask[row] = torch.where(inside, tmpl_deps[trow], 0)
        step_kind[row] = kind
        children_todo[row] = torch.where(inside, todo, 0)
        max_parallel[row] = torch.where(inside, tmpl_maxp[trow], 0)
        children_out[row] = 0
        children_done[row] = 0
        children_fail[row] = 0
        children_emitted[row] = 0
        next_ready[row] = torch.where(inside, tick1 + tmpl_delay[trow], 0)
        dispatch_tick[row] = torch.where(inside, tick1, 0)
        n_steps[slot] = ns
        cond_bits[slot] = int(req_cond[i])
        run_state[slot] = 0
        run_active[slot] = 1
        run_life[slot] = WFL_LIVE
        run_gen[slot] += 1
        out_slot[i] = slot
        out_gen[i] = int(run_gen[slot])


def wf_admit_keep_ref(req_tmpl, req_cond, req_fanout,
                      tmpl_deps, tmpl_kind, tmpl_todo, tmpl_maxp, tmpl_delay,
                      tmpl_nsteps,
                      step_state, step_attempts, deps_mask, step_kind,
                      children_todo, max_parallel, children_out, children_done,
                      children_fail, children_emitted, next_ready, dispatch_tick,
                      n_steps, cond_bits, run_state, run_active, run_life, run_gen,
                      tick, free_mask, blk_scan, out_slot, out_gen, admit_count,
                      req_keep, req_skip):
    """wf_admit with steps already done: bit s of req_keep[i] presets step s
    as SUCCEEDED, or SKIPPED where req_skip[i] has the bit too. A kept set
    with a bit at or past the template's n_steps, or with a kept step that
    depends on a step not kept, gets slot -2 and writes nothing else; that
    is decided before the table is looked at, so -2 wins over -1. Request i
    takes the i-th lowest FREE slot whatever became of the requests before
    it: the slot of a refused request stays FREE."""
    n = int(req_tmpl.shape[0])
    if n <= 0:
        return
    NR = int(n_steps.shape[0])
    TC = int(tmpl_nsteps.shape[0])
    tick1 = int(tick[0]) + 1  # the run's first tick
    free = torch.nonzero(run_life[:NR] == WFL_FREE).flatten().tolist()  # ascending
    m64 = (1 << 64) - 1
    for i in range(n):
        tid = int(req_tmpl[i])
        known = 0 <= tid < TC  # the host rejects the rest
        t0 = tid if known else 0
        ns = int(tmpl_nsteps[tid]) if known else 0
        keep = int(req_keep[i]) & m64
        skip = int(req_skip[i]) & keep
        closed = keep >> ns == 0 and all(
            int(tmpl_deps[t0 * 64 + s]) & m64 & ~keep == 0
            for s in range(ns) if keep >> s & 1)
        if not closed:
            out_slot[i] = -2
            out_gen[i] = 0
            continue
        if i >= len(free):
            out_slot[i] = -1
            out_gen[i] = 0
            continue
        slot = free[i]
        fan = int(req_fanout[i])
        row = slice(slot * 64, slot * 64 + 64)
        trow = slice(t0 * 64, t0 * 64 + 64)
        inside = torch.arange(64) < ns
        kind = torch.where(inside, tmpl_kind[trow], 0)
        todo = tmpl_todo[trow]
        if fan > 0:
            todo = torch.where(kind == WFK_FOR_EACH, fan, todo)
        step_state[row] = torch.tensor(
            [WFS_SKIPPED if skip >> s & 1 else WFS_SUCCEEDED if keep >> s & 1
             else WFS_PENDING for s in range(64)], dtype=step_state.dtype)
        step_attempts[row] = 0
        deps_mask[row] = torch.where(inside, tmpl_deps[trow], 0)
        step_kind[row] = kind
        children_todo[row] = torch.where(inside, todo, 0)
        max_parallel[row] = torch.where(inside, tmpl_maxp[trow], 0)
        children_out[row] = 0
        children_done[row] = 0
        children_fail[row] = 0
        children_emitted[row] = 0
        next_ready[row] = torch.where(inside, tick1 + tmpl_delay[trow], 0)
        dispatch_tick[row] = torch.where(inside, tick1, 0)
        n_steps[slot] = ns
        cond_bits[slot] = int(req_cond[i])
        run_state[slot] = 0
        run_active[slot] = 1
        run_life[slot] = WFL_LIVE
        run_gen[slot] += 1
        out_slot[i] = slot
        out_gen[i] = int(run_gen[slot])
        admit_count[0] += 1


def wf_cancel_ref(req_slot, req_gen, run_life, run_gen, run_active, run_state,
                  n_steps, step_state, cancel_count, out_ok):
    NR = int(n_steps.shape[0])
    for i in range(int(req_slot.shape[0])):
        slot = int(req_slot[i])
        ok = (0 <= slot < NR and int(run_life[slot]) == WFL_LIVE
              and int(run_gen[slot]) == int(req_gen[i])
              and int(run_active[slot]) == 1)
        if not ok:
            out_ok[i] = 0
            continue
        for s in range(int(n_steps[slot])):
            ri = slot * 64 + s
            if int(step_state[ri]) in (WFS_PENDING, WFS_DISPATCHED, WFS_WAITING):
                step_state[ri] = WFS_CANCELLED
        run_active[slot] = 0
        run_state[slot] = WFS_CANCELLED
        out_ok[i] = 1
        cancel_count[0] += 1


def wf_retire_ref(run_life, run_active, run_state, run_gen, n_steps,
                  children_out, dispatch_tick, tick, cutoff: int,
                  done_slot, done_gen, done_state, done_count):
    NR = int(n_steps.shape[0])
    cap = int(done_slot.shape[0])
    stale = int(tick[0]) - cutoff
    for run in range(NR):
        life = int(run_life[run])
        if life == WFL_LIVE and int(run_active[run]) == 0:
            pos = int(done_count[0])
            done_count[0] = pos + 1
            if pos < cap:
                done_slot[pos] = run
                done_gen[pos] = int(run_gen[run])
                done_state[pos] = int(run_state[run])
            life = WFL_DRAINING
        if life != WFL_DRAINING:
            continue
        # quiescent: no step has a child out that can still apply
        quiet = all(
            int(children_out[run * 64 + s]) <= 0
            or int(dispatch_tick[run * 64 + s]) <= stale
            for s in range(int(n_steps[run])))
        life = WFL_FREE if quiet else WFL_DRAINING
        if life != int(run_life[run]):
            run_life[run] = life


def wf_journal_ref(step_state, run_life, run_gen, tick, phase: int,
                   ev_shadow_state, ev_shadow_gen, ev_rec, ev_count):
    """One pass of the step-transition journal. Rows and steps are visited in
    ascending order, so a full list keeps the lowest (slot, step) changes; a
    change that does not fit leaves its shadow byte where it was (PENDING
    after a generation change) and is found again by the next pass. The
    count stops at cap: nothing is added once it is at or above it."""
    NR = int(run_life.shape[0])
    cap = int(ev_rec.shape[0]) // 4
    stamp = 2 * int(tick[0]) + int(phase)
    live = run_life[:NR] != WFL_FREE
    regen = live & (run_gen[:NR] != ev_shadow_gen[:NR])
    st = step_state.view(NR, 64)
    sh = ev_shadow_state.view(NR, 64)
    sh[regen] = WFS_PENDING
    ev_shadow_gen[regen] = run_gen[:NR][regen]
    idx = torch.nonzero((st != sh) & live[:, None])      # ascending (row, step)
    count = int(ev_count[0])
    k = min(int(idx.shape[0]), max(0, cap - count))
    if k == 0:
        return
    rows, steps = idx[:k, 0], idx[:k, 1]
    frm, to = sh[rows, steps].to(torch.int32), st[rows, steps].to(torch.int32)
    rec = ev_rec.view(-1, 4)[count:count + k]
    rec[:, 0] = rows.to(torch.int32)
    rec[:, 1] = run_gen[:NR][rows]
    rec[:, 2] = steps.to(torch.int32) | (frm << 8) | (to << 16)
    rec[:, 3] = stamp
    sh[rows, steps] = st[rows, steps]
    ev_count[0] = count + k


# -- K3-WF externally decided approvals (hold scan / hold list / decide) --------
# A row's hold data counts only while hold_gen == run_gen, the row is LIVE and
# run_active == 1; otherwise it is empty, whatever the words hold.

_M64 = (1 << 64) - 1


def _to_i64(m: int) -> int:
    return m - (1 << 64) if m >= (1 << 63) else m


def wf_hold_scan_ref(step_state, n_steps, run_life, run_active, run_gen, tick,
                     hold_ttl, hold_mask, hold_tick, hold_gen, hold_counts,
                     hold_open):
    """One hold scan (inside the tick, after the sweep). Per LIVE and active
    row: a WAITING step with its bit clear opens a hold stamped `tick`; a
    continuing hold whose ttl has run out (tick - hold_tick >= ttl > 0) fails
    its step; a bit whose step left WAITING is cleared. A generation change
    empties the mask first. Rows that are not LIVE-and-active lose a valid
    nonzero mask; FREE rows are not visited. hold_open gains the number of
    bits left set."""
    NR = int(run_life.shape[0])
    now = int(tick[0])
    life = run_life[:NR]
    act = (life == WFL_LIVE) & (run_active[:NR] == 1)
    match = hold_gen[:NR] == run_gen[:NR]
    hold_mask[(life != WFL_FREE) & ~act & match & (hold_mask[:NR] != 0)] = 0
    st = step_state.view(NR, 64)
    waiting = (st == WFS_WAITING) & (torch.arange(64)[None, :] < n_steps[:NR, None])
    rows = torch.nonzero(act & (waiting.any(dim=1) | ~match | (hold_mask[:NR] != 0)))
    opened = expired = still = 0
    for r in rows.flatten().tolist():
        raw = int(hold_mask[r]) & _M64
        old = raw if bool(match[r]) else 0
        new = 0
        for s in torch.nonzero(waiting[r]).flatten().tolist():
            i = r * 64 + s
            if not (old >> s) & 1:
                hold_tick[i] = now
                opened += 1
            else:
                ttl = int(hold_ttl[i])
                if ttl > 0 and now - int(hold_tick[i]) >= ttl:
                    step_state[i] = WFS_FAILED
                    expired += 1
                    continue
            new |= 1 << s
        if new != raw:
            hold_mask[r] = _to_i64(new)
        if not bool(match[r]):
            hold_gen[r] = int(run_gen[r])
        still += bin(new).count("1")
    hold_counts[0] += opened
    hold_counts[1] += expired
    hold_open[0] += still


def wf_hold_list_ref(step_state, run_life, run_active, run_gen, hold_mask,
                     hold_tick, hold_gen, cursor: int, list_mask, blk_scan, out):
    """One page of open holds in ascending (slot, step): out[0] is the number
    of holds with key slot*64+step >= cursor, out[4:] the records (slot, gen,
    step, hold_tick) of the lowest min(count, cap) of them. list_mask /
    blk_scan are the kernel's workspaces: unused."""
    NR = int(run_life.shape[0])
    cap = (int(out.shape[0]) - 4) // 4
    valid = ((run_life[:NR] == WFL_LIVE) & (run_active[:NR] == 1)
             & (hold_gen[:NR] == run_gen[:NR]) & (hold_mask[:NR] != 0))
    rec = out[4:].view(-1, 4)
    count = 0
    for r in torch.nonzero(valid).flatten().tolist():
        m = int(hold_mask[r]) & _M64
        while m:                                   # set bits, ascending
            s = (m & -m).bit_length() - 1
            m &= m - 1
            if r * 64 + s < cursor or int(step_state[r * 64 + s]) != WFS_WAITING:
                continue
            if count < cap:
                rec[count, 0] = r
                rec[count, 1] = int(run_gen[r])
                rec[count, 2] = s
                rec[count, 3] = int(hold_tick[r * 64 + s])
            count += 1
    out[0] = count


def wf_decide_ref(req_slot, req_gen, req_step, req_verdict, run_life, run_gen,
                  run_active, n_steps, step_kind, step_state, hold_counts,
                  out_code):
    """Decisions by (slot, gen, step): code 0 applied (verdict 1 -> SUCCEEDED,
    0 -> FAILED), 1 stale handle, 2 run no longer active, 3 not a waiting
    approval. The hold tables are not touched."""
    NR = int(n_steps.shape[0])
    for i in range(int(req_slot.shape[0])):
        slot, step = int(req_slot[i]), int(req_step[i])
        if (not 0 <= slot < NR or int(run_life[slot]) != WFL_LIVE
                or int(run_gen[slot]) != int(req_gen[i])):
            out_code[i] = 1
        elif int(run_active[slot]) != 1:
            out_code[i] = 2
        elif (not 0 <= step < int(n_steps[slot])
              or int(step_kind[slot * 64 + step]) != WFK_APPROVAL
              or int(step_state[slot * 64 + step]) != WFS_WAITING):
            out_code[i] = 3
        else:
            yes = int(req_verdict[i]) != 0
            step_state[slot * 64 + step] = WFS_SUCCEEDED if yes else WFS_FAILED
            hold_counts[2 if yes else 3] += 1
            out_code[i] = 0


# -- K3-WF per-step retry / backoff / timeout policy (wf_settle) ----------------
def wf_backoff_ref(k: int, backoff_ticks: int, cap_ticks: int, multiplier_q8: int) -> int:
    """Ticks to wait before attempt k + 1 (k >= 1 failures so far): integers
    only, 16.16 fixed point with an 8.8 multiplier, the kernel's arithmetic.
    cap_ticks 0 means no cap; the delay then saturates at 2^20 ticks."""
    limit = (cap_ticks if cap_ticks > 0 else 1 << 20) << 16
    d = min(backoff_ticks << 16, limit)
    for _ in range(min(k - 1, 63)):
        if d == limit:
            break
        d = min((d * multiplier_q8) >> 8, limit)
    return (d + 65535) >> 16


def wf_settle_ref(step_state, step_attempts, children_todo, children_out,
                  children_fail, max_parallel, next_ready, dispatch_tick,
                  run_life, run_tmpl, tmpl_policy, tmpl_timeout, tick,
                  timeout_count, retry_count):
    """wf_timeout_scan followed by wf_commit, per DISPATCHED step of every row
    that is not FREE, with the step's own constants: its record
    tmpl_policy[(t*64+s)*4:+4] = (max_retries, backoff_ticks, cap_ticks,
    multiplier_q8) and tmpl_timeout[t*64+s], t = run_tmpl[row]. A row whose
    template id is outside the table is left alone."""
    NR = int(run_life.shape[0])
    TC = int(tmpl_timeout.shape[0]) // 64
    now = int(tick[0])
    st = step_state.view(NR, 64)
    rows = torch.nonzero((run_life[:NR] != WFL_FREE)
                         & (st == WFS_DISPATCHED).any(dim=1)).flatten().tolist()
    lost_sum = retry_sum = 0
    for r in rows:
        t = int(run_tmpl[r])
        if not 0 <= t < TC:
            continue
        for s in torch.nonzero(st[r] == WFS_DISPATCHED).flatten().tolist():
            i, p = r * 64 + s, t * 64 + s
            out, fail = int(children_out[i]), int(children_fail[i])
            if out > 0 and int(dispatch_tick[i]) <= now - int(tmpl_timeout[p]):
                fail += out
                lost_sum += out
                out = 0
                children_out[i] = 0
                children_fail[i] = fail
            if out != 0:
                mp = int(max_parallel[i])
                if int(children_todo[i]) > 0 and (mp == 0 or out < mp):
                    step_state[i] = WFS_PENDING
            elif fail > 0:
                max_retries, backoff, cap, mult = tmpl_policy[4 * p:4 * p + 4].tolist()
                att = int(step_attempts[i])
                if att < max_retries:
                    step_attempts[i] = att + 1
                    children_todo[i] += fail
                    children_fail[i] = 0
                    next_ready[i] = now + wf_backoff_ref(att + 1, backoff, cap, mult)
                    step_state[i] = WFS_PENDING
                    retry_sum += fail
                else:
                    step_state[i] = WFS_FAILED
            elif int(children_todo[i]) > 0:
                step_state[i] = WFS_PENDING
            else:
                step_state[i] = WFS_SUCCEEDED
    timeout_count[0] += lost_sum
    retry_count[0] += retry_sum


# -- K3-WF conditions decided on the device --------------------------------------
# Predicate record (code, a, b, imm), see the kernel section of the same name:
# code bits 0..3 op, bit 4 negate, bits 8..9 lhs kind, bits 12..13 rhs kind.
WFC_EQ, WFC_NE, WFC_LT, WFC_LE, WFC_GT, WFC_GE, WFC_TRUTHY = 1, 2, 3, 4, 5, 6, 7
WFC_NEGATE = 1 << 4
WFC_IMM, WFC_INPUT, WFC_OUT = 0, 1, 2


def wf_cond_value_ref(rec, in_row, out_row) -> bool:
    """Value of one predicate record over a run's input words and step output
    words; comparisons are signed 32-bit, an operand index outside its row
    reads as 0."""
    code, a, b, imm = (int(x) for x in rec)

    def operand(kind, idx, lit):
        if kind == WFC_INPUT:
            return int(in_row[idx]) if 0 <= idx < len(in_row) else 0
        if kind == WFC_OUT:
            return int(out_row[idx]) if 0 <= idx < 64 else 0
        return lit

    lk = (code >> 8) & 3
    lhs = operand(lk, a, 0) if lk else 0
    rhs = operand((code >> 12) & 3, b, imm)
    op = code & 15
    v = {WFC_EQ: lhs == rhs, WFC_NE: lhs != rhs, WFC_LT: lhs < rhs,
         WFC_LE: lhs <= rhs, WFC_GT: lhs > rhs, WFC_GE: lhs >= rhs,
         WFC_TRUTHY: lhs != 0}.get(op, False)
    return v != bool(code & WFC_NEGATE)


def wf_cond_eval_ref(step_state, deps_mask, step_kind, run_life, run_active,
                     run_tmpl, tmpl_cond, tmpl_cond_mask, run_input, step_out,
                     cond_bits, cond_counts, input_words: int):
    """The predicate pass before the sweep. Per LIVE, active row with a
    template id inside the table: every PENDING step that carries a predicate
    and whose deps are satisfied (SUCCEEDED or SKIPPED) is evaluated once. A
    CONDITION step gets its bit in cond_bits set or cleared and step_out 1 or
    0; any other step stays PENDING if true and becomes SKIPPED if false. A
    step skipped here can satisfy another one's deps, so the row repeats until
    no guard turned false."""
    NR = int(run_life.shape[0])
    TC = int(tmpl_cond_mask.shape[0])
    IW = int(input_words)
    st = step_state.view(NR, 64)
    look = ((run_life[:NR] == WFL_LIVE) & (run_active[:NR] != 0)
            & (run_tmpl[:NR] >= 0) & (run_tmpl[:NR] < TC))
    n_true = n_false = 0
    for r in torch.nonzero(look).flatten().tolist():
        t = int(run_tmpl[r])
        cmask = int(tmpl_cond_mask[t]) & _M64
        todo = [s for s in range(64)
                if (cmask >> s) & 1 and int(st[r, s]) == WFS_PENDING]
        if not todo:
            continue
        in_row = run_input[r * IW:(r + 1) * IW].tolist()
        setm = clrm = 0
        while todo:
            row = st[r].tolist()
            sat = sum(1 << s for s in range(64) if row[s] in (WFS_SUCCEEDED, WFS_SKIPPED))
            skipped, left = False, []
            for s in todo:
                i = r * 64 + s
                if (int(deps_mask[i]) & _M64) & ~sat:
                    left.append(s)
                    continue
                v = wf_cond_value_ref(tmpl_cond[(t * 64 + s) * 4:(t * 64 + s) * 4 + 4].tolist(),
                                      in_row, step_out[r * 64:r * 64 + 64].tolist())
                n_true += int(v)
                n_false += int(not v)
                if int(step_kind[i]) == WFK_CONDITION:
                    if v:
                        setm |= 1 << s
                    else:
                        clrm |= 1 << s
                    step_out[i] = int(v)
                elif not v:
                    step_state[i] = WFS_SKIPPED
                    skipped = True
            todo = left
            if not skipped:
                break
        if setm | clrm:
            cond_bits[r] = _to_i64(((int(cond_bits[r]) & _M64) & ~clrm) | setm)
    cond_counts[0] += n_true
    cond_counts[1] += n_false


def wf_child_payload_ref(child_tag, child_seq, child_count, run_input,
                         child_payload, input_words: int, payload_words: int):
    """Payload rows of arena slots 0 .. min(child_count, CB) - 1: the run's
    input words, the child's ordinal, its step index, then zeros."""
    CB = int(child_tag.shape[0])
    IW, W = int(input_words), int(payload_words)
    NR = int(run_input.shape[0]) // IW
    n = min(max(int(child_count[0]), 0), CB)
    pl = child_payload.view(-1, W)
    for c in range(n):
        tag = int(child_tag[c])
        run = tag >> 6
        pl[c].zero_()
        if 0 <= run < NR:
            pl[c, :IW] = run_input[run * IW:(run + 1) * IW]
        pl[c, IW] = int(child_seq[c])
        pl[c, IW + 1] = tag & 63


def wf_apply_out_ref(send_slots, send_cnt, child_tag, child_seq, rq_prev_tag,
                     rq_prev_seq, children_done, children_fail, children_out,
                     sums_back, step_out, fail_ppt: int, drop_ppt: int, cap: int,
                     world: int):
    """wf_apply_ref, and a child counted as done adds its result word
    sums_back[i] into step_out[tag], wrapping at 32 bits."""
    wf_apply_ref(send_slots, send_cnt, child_tag, child_seq, rq_prev_tag,
                 rq_prev_seq, children_done, children_fail, children_out,
                 fail_ppt, drop_ppt, cap, world, sums_back, step_out)
