"""Per-kernel GPU tests of the run lifecycle kernels (wf_admit, wf_cancel,
wf_retire): each extension function is called directly on small hand-built
tables and compared with its oracle in cordum_amd/ops/reference.py by exact
equality. The done list is appended through the wave-aggregated compaction
and has no defined order: it is compared as a sorted set, its counter
exactly.

The table builders and the "the case is the case" assertions are
module-level functions: tests/test_wf_admission_cases.py runs each builder
through its oracle on a machine without a GPU.
"""
import functools

import pytest
import torch

from cordum_amd.ops.reference import (
    WFK_FOR_EACH, WFK_WORKER, WFL_DRAINING, WFL_FREE, WFL_LIVE, WFS_CANCELLED,
    WFS_DISPATCHED, WFS_PENDING, WFS_WAITING,
)

pytestmark = pytest.mark.gpu

# one lane, the 64-lane wave edge, the 256-slot block edge, and a third
# block with a single slot
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
POISON = -7
I64_MIN = -(1 << 63)
BIG = 1 << 33  # preset of the 64-bit counters: a 32-bit add would show

ROW_TABLES = ("step_state", "step_attempts", "deps_mask", "step_kind",
              "children_todo", "max_parallel", "children_out", "children_done",
              "children_fail", "children_emitted", "next_ready", "dispatch_tick")
ARGS = {
    "wf_admit": ("req_tmpl", "req_cond", "req_fanout", "tmpl_deps", "tmpl_kind",
                 "tmpl_todo", "tmpl_maxp", "tmpl_delay", "tmpl_nsteps")
                + ROW_TABLES
                + ("n_steps", "cond_bits", "run_state", "run_active", "run_life",
                   "run_gen", "tick", "free_mask", "blk_scan", "out_slot",
                   "out_gen", "admit_count"),
    "wf_cancel": ("req_slot", "req_gen", "run_life", "run_gen", "run_active",
                  "run_state", "n_steps", "step_state", "cancel_count", "out_ok"),
    "wf_retire": ("run_life", "run_active", "run_state", "run_gen", "n_steps",
                  "children_out", "dispatch_tick", "tick", "cutoff", "done_slot",
                  "done_gen", "done_state", "done_count"),
}
WORKSPACES = ("free_mask", "blk_scan")  # kernel scratch: never compared


def ref_ops():
    from cordum_amd.ops.pipeline import _RefOps

    return _RefOps()


def call(ops, kernel, t, device="cpu"):
    """Run `kernel` of `ops` on clones of the tables in `t` (on `device`);
    returns every table as a CPU tensor. `t` itself is never written."""
    d = {k: (v.clone().to(device) if torch.is_tensor(v) else v) for k, v in t.items()}
    getattr(ops, kernel)(*[d[a] for a in ARGS[kernel]])
    if str(device) != "cpu":
        torch.cuda.synchronize()
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in d.items()}


def assert_tables_equal(got, want, skip=()):
    for k, w in want.items():
        if k in skip:
            continue
        if torch.is_tensor(w):
            assert got[k].dtype == w.dtype, k
            if not torch.equal(got[k], w):
                bad = torch.nonzero(got[k] != w).flatten()[:8].tolist()
                raise AssertionError(
                    f"{k} differs at {bad}: got {got[k][bad].tolist()} "
                    f"want {w[bad].tolist()}")
        else:
            assert got[k] == w, k


@functools.lru_cache(maxsize=None)
def oracle(kernel, builder, *args):
    """(tables, oracle output): computed once, shared, never written."""
    t = builder(*args)
    return t, call(ref_ops(), kernel, t)


def _rand_i64(n, g):
    hi = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int64, generator=g)
    lo = torch.randint(0, 1 << 32, (n,), dtype=torch.int64, generator=g)
    return (hi << 32) | lo


def _ri(lo, hi, n, g, dtype=torch.int32):
    return torch.randint(lo, hi, (n,), generator=g).to(dtype)


# ---------------------------------------------------------------------------
# wf_admit
# ---------------------------------------------------------------------------
ADMIT_TICK = 41
TC = 5                      # templates: 64 steps, 1 step, random, 3 steps, random
REQ_FANOUT = (7, 9, 0, 0, 3)  # request i uses template i % 5 with this override
N_MODES = ("zero", "one", "F", "F+1", "over_NR")
ADMIT_CASES = (
    [(NR, "random", nm) for NR in SIZES for nm in N_MODES]
    + [(NR, fm, "F+1") for NR in SIZES for fm in ("none", "all", "last", "alternating")]
    + [(513, "third_block_first", "F+1"), (513, "third_block_first", "one")]
)


def build_templates(g):
    n = TC * 64
    t = {
        "tmpl_deps": _rand_i64(n, g),
        "tmpl_kind": _ri(0, 5, n, g, torch.uint8),
        "tmpl_todo": _ri(1, 21, n, g),
        "tmpl_maxp": _ri(0, 6, n, g),
        "tmpl_delay": _ri(0, 6, n, g),
        "tmpl_nsteps": torch.tensor(
            [64, 1, int(_ri(2, 64, 1, g)[0]), 3, int(_ri(2, 64, 1, g)[0])],
            dtype=torch.uint8),
    }
    # template 0: all 64 steps, every kind, FOR_EACH and WORKER among them
    t["tmpl_kind"][0:64] = (torch.arange(64) % 5).to(torch.uint8)
    t["tmpl_deps"][63] = I64_MIN | 1          # a mask that uses bit 63
    t["tmpl_kind"][64] = WFK_WORKER           # template 1: one WORKER step
    t["tmpl_todo"][64] = 1
    t["tmpl_kind"][3 * 64:3 * 64 + 3] = torch.tensor(
        [WFK_FOR_EACH, WFK_FOR_EACH, WFK_WORKER], dtype=torch.uint8)
    # entries at or past n_steps hold garbage on purpose: the kernel must
    # write zeros there, not the template's value
    return t


def free_slots(NR, mode, g):
    if mode == "none":
        return []
    if mode == "all":
        return list(range(NR))
    if mode == "last":
        return [NR - 1]
    if mode == "third_block_first":
        return [512]
    if mode == "alternating":
        return list(range(0, NR, 2))
    free = torch.nonzero(torch.rand(NR, generator=g) < 0.4).flatten().tolist()
    return sorted(set(free) | {NR - 1})       # the table's last slot is free


def build_admit_tables(NR, free_mode, n_mode, seed=3):
    g = torch.Generator().manual_seed(seed * 1000 + NR)
    t = build_templates(g)
    n64 = NR * 64
    # every live table starts as garbage, so that each write shows
    for k in ROW_TABLES:
        if k == "deps_mask":
            t[k] = _rand_i64(n64, g)
        elif k in ("step_state", "step_kind"):
            t[k] = _ri(1, 7, n64, g, torch.uint8)
        else:
            t[k] = _ri(1, 90, n64, g)
    t["n_steps"] = _ri(1, 65, NR, g, torch.uint8)
    t["cond_bits"] = _rand_i64(NR, g)
    t["run_state"] = _ri(3, 7, NR, g, torch.uint8)
    t["run_active"] = _ri(0, 2, NR, g, torch.uint8)
    t["run_gen"] = _ri(0, 1000, NR, g)
    free = free_slots(NR, free_mode, g)
    life = _ri(1, 3, NR, g, torch.uint8)      # LIVE or DRAINING
    life[free] = WFL_FREE
    t["run_life"] = life
    F = len(free)
    n = {"zero": 0, "one": 1, "F": F, "F+1": F + 1, "over_NR": NR + 3}[n_mode]
    t["req_tmpl"] = (torch.arange(n) % TC).to(torch.int32)
    t["req_fanout"] = torch.tensor([REQ_FANOUT[i % TC] for i in range(n)],
                                   dtype=torch.int32)
    t["req_cond"] = _rand_i64(n, g)
    if n:
        t["req_cond"][0] = I64_MIN | 5        # bit 63 set
    t["tick"] = torch.tensor([ADMIT_TICK], dtype=torch.int32)
    nblk = (NR + 255) // 256
    t["free_mask"] = torch.full((nblk * 4,), POISON, dtype=torch.int64)
    t["blk_scan"] = torch.full((nblk + 1,), POISON, dtype=torch.int32)
    t["out_slot"] = torch.full((n,), POISON, dtype=torch.int32)
    t["out_gen"] = torch.full((n,), POISON, dtype=torch.int32)
    t["admit_count"] = torch.tensor([BIG], dtype=torch.int64)
    t["free"] = free                          # not a kernel argument
    return t


def assert_admit_case(t, want):
    """Placement, counters and the row image, stated independently of the
    oracle's code path."""
    free, n = t["free"], int(t["req_tmpl"].shape[0])
    acc = min(n, len(free))
    assert want["out_slot"].tolist() == free[:acc] + [-1] * (n - acc)
    assert int(want["admit_count"][0]) == BIG + acc
    taken = free[:acc]
    assert want["out_gen"][:acc].tolist() == (t["run_gen"][taken] + 1).tolist()
    assert bool((want["run_life"][taken] == WFL_LIVE).all())
    assert bool((want["run_active"][taken] == 1).all())
    assert bool((want["run_state"][taken] == 0).all())
    assert want["cond_bits"][taken].tolist() == t["req_cond"][:acc].tolist()
    # rows of slots that were not handed out are untouched
    keep = torch.ones(t["run_life"].shape[0], dtype=torch.bool)
    keep[taken] = False
    for k in ROW_TABLES:
        assert torch.equal(want[k].view(-1, 64)[keep], t[k].view(-1, 64)[keep]), k
    for k in ("n_steps", "cond_bits", "run_state", "run_active", "run_life", "run_gen"):
        assert torch.equal(want[k][keep], t[k][keep]), k
    for i, slot in enumerate(taken):
        tid = i % TC
        ns = int(t["tmpl_nsteps"][tid])
        assert int(want["n_steps"][slot]) == ns
        row = {k: want[k].view(-1, 64)[slot] for k in ROW_TABLES}
        for k in ROW_TABLES:                  # zero at and past n_steps
            assert not bool(row[k][ns:].any()), (k, slot)
        for k in ("step_state", "step_attempts", "children_out", "children_done",
                  "children_fail", "children_emitted"):
            assert not bool(row[k].any()), (k, slot)
        tr = slice(tid * 64, tid * 64 + ns)
        kind = t["tmpl_kind"][tr]
        assert torch.equal(row["step_kind"][:ns], kind)
        assert torch.equal(row["deps_mask"][:ns], t["tmpl_deps"][tr])
        assert torch.equal(row["max_parallel"][:ns], t["tmpl_maxp"][tr])
        assert torch.equal(row["next_ready"][:ns], ADMIT_TICK + 1 + t["tmpl_delay"][tr])
        assert bool((row["dispatch_tick"][:ns] == ADMIT_TICK + 1).all())
        fan = REQ_FANOUT[tid]
        todo = t["tmpl_todo"][tr].clone()
        if fan > 0:
            todo[kind == WFK_FOR_EACH] = fan  # ignored on every other kind
        assert torch.equal(row["children_todo"][:ns], todo)


# ---------------------------------------------------------------------------
# wf_cancel
# ---------------------------------------------------------------------------
# Special rows sit at the END of the table (role p is run NR-1-p), so the
# edge rows are always among the requests.
CANCEL_ROLES = ("effective64", "stale_gen", "terminal", "draining", "free",
                "effective1")


def build_cancel_tables(NR, seed=5):
    g = torch.Generator().manual_seed(seed * 1000 + NR)
    n64 = NR * 64
    t = {
        "run_life": _ri(0, 3, NR, g, torch.uint8),
        "run_gen": _ri(1, 50, NR, g),
        "run_active": _ri(0, 2, NR, g, torch.uint8),
        "run_state": _ri(0, 6, NR, g, torch.uint8),
        "n_steps": _ri(1, 65, NR, g, torch.uint8),
        "step_state": _ri(0, 7, n64, g, torch.uint8),
        "cancel_count": torch.tensor([BIG], dtype=torch.int64),
    }
    st = t["step_state"].view(-1, 64)
    roles = {}
    for p, role in enumerate(CANCEL_ROLES):
        r = NR - 1 - p
        if r < 0:
            break
        roles[role] = r
        t["run_life"][r] = WFL_LIVE
        t["run_active"][r] = 1
        t["run_state"][r] = 0
        if role == "effective64":
            t["n_steps"][r] = 64
            st[r] = (torch.arange(64) % 6).to(torch.uint8)  # all six states
        elif role == "terminal":
            t["run_active"][r] = 0
            t["run_state"][r] = 3
        elif role == "draining":
            t["run_life"][r] = WFL_DRAINING
        elif role == "free":
            t["run_life"][r] = WFL_FREE
        elif role == "effective1":
            t["n_steps"][r] = 1
            st[r] = WFS_PENDING                 # steps 1..63 must stay PENDING
    # distinct slots: every role row, a random half of the others, and the
    # handle of a rejected admission (slot -1)
    others = [r for r in range(NR - len(roles))
              if float(torch.rand(1, generator=g)) < 0.5]
    slots = sorted(roles.values()) + others + [-1]
    perm = torch.randperm(len(slots), generator=g).tolist()
    slots = [slots[i] for i in perm]
    gens = [int(t["run_gen"][s]) if s >= 0 else 1 for s in slots]
    if "stale_gen" in roles:
        gens[slots.index(roles["stale_gen"])] += 1
    t["req_slot"] = torch.tensor(slots, dtype=torch.int32)
    t["req_gen"] = torch.tensor(gens, dtype=torch.int32)
    t["out_ok"] = torch.full((len(slots),), 9, dtype=torch.uint8)
    t["roles"] = roles                          # not a kernel argument
    return t


def assert_cancel_case(t, want):
    slots, gens = t["req_slot"].tolist(), t["req_gen"].tolist()
    assert len(set(slots)) == len(slots)
    eff = [s >= 0 and int(t["run_life"][s]) == WFL_LIVE
           and int(t["run_gen"][s]) == g and int(t["run_active"][s]) == 1
           for s, g in zip(slots, gens)]
    assert want["out_ok"].tolist() == [int(e) for e in eff]
    assert int(want["cancel_count"][0]) == BIG + sum(eff)
    hit = [s for s, e in zip(slots, eff) if e]
    keep = torch.ones(t["run_life"].shape[0], dtype=torch.bool)
    keep[hit] = False
    for k in ("run_active", "run_state"):
        assert torch.equal(want[k][keep], t[k][keep]), k
    assert torch.equal(want["step_state"].view(-1, 64)[keep],
                       t["step_state"].view(-1, 64)[keep])
    for k in ("run_life", "run_gen", "n_steps"):
        assert torch.equal(want[k], t[k]), k
    open_states = (WFS_PENDING, WFS_DISPATCHED, WFS_WAITING)
    for s in hit:
        assert int(want["run_active"][s]) == 0
        assert int(want["run_state"][s]) == WFS_CANCELLED
        ns = int(t["n_steps"][s])
        before = t["step_state"].view(-1, 64)[s]
        after = want["step_state"].view(-1, 64)[s]
        assert torch.equal(after[ns:], before[ns:])
        for a, b in zip(after[:ns].tolist(), before[:ns].tolist()):
            assert a == (WFS_CANCELLED if b in open_states else b)
    roles = t["roles"]
    for role, r in roles.items():
        assert (r in hit) == role.startswith("effective"), role
    if "effective64" in roles:
        r = roles["effective64"]
        assert set(t["step_state"].view(-1, 64)[r].tolist()) == {0, 1, 2, 3, 4, 5}
        assert set(want["step_state"].view(-1, 64)[r].tolist()) == {3, 4, 5, 6}
    if "stale_gen" in roles:   # a LIVE, active slot named with another generation
        r = roles["stale_gen"]
        i = slots.index(r)
        assert int(t["run_life"][r]) == WFL_LIVE and int(t["run_active"][r]) == 1
        assert gens[i] != int(t["run_gen"][r])
    if "effective1" in roles:
        r = roles["effective1"]
        assert want["step_state"].view(-1, 64)[r].tolist() == [WFS_CANCELLED] + [0] * 63


# ---------------------------------------------------------------------------
# wf_retire
# ---------------------------------------------------------------------------
RETIRE_TICK, RETIRE_CUTOFF = 100, 8
FRESH = RETIRE_TICK - RETIRE_CUTOFF + 1       # youngest tick that still blocks
STALE = RETIRE_TICK - RETIRE_CUTOFF           # oldest tick that no longer does
# role -> (life before, run_active, life after, reported)
RETIRE_ROLES = {
    "live_active": (WFL_LIVE, 1, WFL_LIVE, False),
    "terminal_no_children": (WFL_LIVE, 0, WFL_FREE, True),
    "terminal_fresh_children": (WFL_LIVE, 0, WFL_DRAINING, True),
    "terminal_stale_children": (WFL_LIVE, 0, WFL_FREE, True),
    "draining_now_quiet": (WFL_DRAINING, 0, WFL_FREE, False),
    "draining_step63_blocks": (WFL_DRAINING, 0, WFL_DRAINING, False),
    "terminal_block_past_n_steps": (WFL_LIVE, 0, WFL_FREE, True),
    "draining_still_blocked": (WFL_DRAINING, 0, WFL_DRAINING, False),
    "free_garbage": (WFL_FREE, 0, WFL_FREE, False),
}


def build_retire_tables(NR, seed=9):
    g = torch.Generator().manual_seed(seed * 1000 + NR)
    n64 = NR * 64
    t = {
        "run_life": _ri(0, 3, NR, g, torch.uint8),
        "run_active": _ri(0, 2, NR, g, torch.uint8),
        "run_state": _ri(3, 7, NR, g, torch.uint8),
        "run_gen": _ri(1, 1000, NR, g),
        "n_steps": _ri(1, 65, NR, g, torch.uint8),
        "children_out": torch.tensor([-1, 0, 0, 0, 0, 2], dtype=torch.int32)[
            torch.randint(0, 6, (n64,), generator=g)],
        "dispatch_tick": _ri(RETIRE_TICK - 12, RETIRE_TICK + 1, n64, g),
        "tick": torch.tensor([RETIRE_TICK], dtype=torch.int32),
        "cutoff": RETIRE_CUTOFF,
        "done_slot": torch.full((NR,), POISON, dtype=torch.int32),
        "done_gen": torch.full((NR,), POISON, dtype=torch.int32),
        "done_state": torch.full((NR,), POISON, dtype=torch.int32),
        "done_count": torch.zeros(1, dtype=torch.int32),
    }
    # a FREE slot is never active
    t["run_active"][t["run_life"] == WFL_FREE] = 0
    co = t["children_out"].view(-1, 64)
    dt = t["dispatch_tick"].view(-1, 64)
    roles = {}
    for p, (role, (life, active, _, _)) in enumerate(RETIRE_ROLES.items()):
        r = NR - 1 - p
        if r < 0:
            break
        roles[role] = r
        t["run_life"][r], t["run_active"][r] = life, active
        t["n_steps"][r] = 7
        co[r] = 0
        dt[r] = RETIRE_TICK
        if role == "terminal_fresh_children":
            co[r, 3], dt[r, 3] = 2, FRESH
        elif role == "terminal_stale_children":
            co[r, 3], dt[r, 3] = 2, STALE
        elif role == "draining_now_quiet":
            co[r, 2] = -1                       # over-applied, not blocking
        elif role == "draining_step63_blocks":
            t["n_steps"][r] = 64
            co[r, 63], dt[r, 63] = 1, FRESH
        elif role == "terminal_block_past_n_steps":
            t["n_steps"][r] = 5
            co[r, 5], co[r, 63] = 4, 4          # steps 5 and 63 are no steps
        elif role == "draining_still_blocked":
            co[r, 0], dt[r, 0] = 1, RETIRE_TICK
        elif role == "free_garbage":
            co[r, 1] = 3
    t["roles"] = roles                          # not a kernel argument
    return t


def done_records(d):
    n = int(d["done_count"][0])
    return sorted(zip(d["done_slot"][:n].tolist(), d["done_gen"][:n].tolist(),
                      d["done_state"][:n].tolist()))


def assert_retire_case(t, want):
    for role, r in t["roles"].items():
        _, _, after, reported = RETIRE_ROLES[role]
        assert int(want["run_life"][r]) == after, role
        assert (r in [x[0] for x in done_records(want)]) == reported, role
    live_term = (t["run_life"] == WFL_LIVE) & (t["run_active"] == 0)
    rec = done_records(want)
    assert [x[0] for x in rec] == torch.nonzero(live_term).flatten().tolist()
    for slot, gen, state in rec:
        assert gen == int(t["run_gen"][slot]) and state == int(t["run_state"][slot])
    n = len(rec)
    assert bool((want["done_slot"][n:] == POISON).all())
    # LIVE and active, and FREE, are never written
    same = ((t["run_life"] == WFL_LIVE) & (t["run_active"] == 1)) | (t["run_life"] == WFL_FREE)
    assert torch.equal(want["run_life"][same], t["run_life"][same])
    for k in ("run_active", "run_state", "run_gen", "n_steps", "children_out",
              "dispatch_tick"):
        assert torch.equal(want[k], t[k]), k
    roles = t["roles"]
    if "terminal_stale_children" in roles:      # children out, but stale
        r = roles["terminal_stale_children"]
        assert int(t["children_out"][r * 64 + 3]) > 0
        assert int(t["dispatch_tick"][r * 64 + 3]) <= RETIRE_TICK - RETIRE_CUTOFF
    if "terminal_fresh_children" in roles:
        r = roles["terminal_fresh_children"]
        assert int(t["dispatch_tick"][r * 64 + 3]) == RETIRE_TICK - RETIRE_CUTOFF + 1


def assert_retire_matches(got, want):
    assert int(got["done_count"][0]) == int(want["done_count"][0])
    assert done_records(got) == done_records(want)
    n = int(want["done_count"][0])
    for k in ("done_slot", "done_gen", "done_state"):
        assert torch.equal(got[k][n:], want[k][n:]), k
    assert_tables_equal(got, want, skip=("done_slot", "done_gen", "done_state", "roles"))


# ---------------------------------------------------------------------------
# the tick kernels leave a cancelled step alone
# ---------------------------------------------------------------------------
TICK_KERNELS = ("wf_sweep", "wf_timeout_scan", "wf_commit", "wf_status")


def build_cancelled_tables(NR, seed=13):
    """ACTIVE runs whose steps are all CANCELLED or SUCCEEDED, with every
    other condition for action met: gates open, dependencies satisfied or
    on a cancelled step, children out and stale, failures pending. None of
    the four kernels may write anything."""
    g = torch.Generator().manual_seed(seed * 1000 + NR)
    n64 = NR * 64
    tick = 50
    st = torch.where(torch.rand(n64, generator=g) < 0.7,
                     torch.tensor(WFS_CANCELLED), torch.tensor(3)).to(torch.uint8)
    st.view(-1, 64)[:, 0] = WFS_CANCELLED       # no run is all-SUCCEEDED
    return {
        "step_state": st,
        "deps_mask": _rand_i64(n64, g) & 0x7,   # on steps 0..2
        "n_steps": _ri(3, 65, NR, g, torch.uint8),
        "run_active": torch.ones(NR, dtype=torch.uint8),
        "run_state": torch.zeros(NR, dtype=torch.uint8),
        "step_kind": _ri(0, 5, n64, g, torch.uint8),
        "cond_bits": _rand_i64(NR, g),
        "next_ready": _ri(0, tick + 1, n64, g),
        "tick": torch.tensor([tick], dtype=torch.int32),
        "disp_runs": torch.full((n64,), POISON, dtype=torch.int32),
        "disp_steps": torch.full((n64,), POISON, dtype=torch.int32),
        "disp_count": torch.zeros(1, dtype=torch.int32),
        "appr_runs": torch.full((NR,), POISON, dtype=torch.int32),
        "appr_steps": torch.full((NR,), POISON, dtype=torch.int32),
        "appr_count": torch.zeros(1, dtype=torch.int32),
        "step_attempts": _ri(0, 2, n64, g),
        "children_todo": _ri(0, 3, n64, g),
        "children_out": _ri(0, 3, n64, g),
        "children_done": _ri(0, 5, n64, g),
        "children_fail": _ri(0, 3, n64, g),
        "max_parallel": _ri(0, 3, n64, g),
        "dispatch_tick": _ri(0, tick - 20, n64, g),
        "cutoff": 8, "max_retries": 5,
        "timeout_count": torch.tensor([BIG], dtype=torch.int64),
        "retry_count": torch.tensor([BIG], dtype=torch.int64),
        "counts": torch.tensor([BIG, BIG], dtype=torch.int64),
    }


def assert_tick_kernels_write_nothing(ops, NR, device="cpu"):
    from tests import test_gpu_wf_kernels as K

    t = build_cancelled_tables(NR)
    assert bool((t["step_state"] == WFS_CANCELLED).any())
    for kernel in TICK_KERNELS:
        assert_tables_equal(K.call(ops, kernel, t, device), t)


# ---------------------------------------------------------------------------
# the GPU tests
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ext():
    from cordum_amd.ops import get_ext

    return get_ext(required=True)


@pytest.mark.parametrize("NR,free_mode,n_mode", ADMIT_CASES)
def test_wf_admit_matches_oracle(ext, NR, free_mode, n_mode):
    t, want = oracle("wf_admit", build_admit_tables, NR, free_mode, n_mode)
    got = call(ext, "wf_admit", t, "cuda")
    assert_tables_equal(got, want, skip=WORKSPACES + ("free",))


@pytest.mark.parametrize("NR", SIZES)
def test_wf_cancel_matches_oracle(ext, NR):
    t, want = oracle("wf_cancel", build_cancel_tables, NR)
    got = call(ext, "wf_cancel", t, "cuda")
    assert_tables_equal(got, want, skip=("roles",))


@pytest.mark.parametrize("NR", SIZES)
def test_wf_retire_matches_oracle(ext, NR):
    t, want = oracle("wf_retire", build_retire_tables, NR)
    got = call(ext, "wf_retire", t, "cuda")
    assert_retire_matches(got, want)


@pytest.mark.parametrize("NR", (1, 65, 257))
def test_tick_kernels_leave_cancelled_steps_alone(ext, NR):
    assert_tick_kernels_write_nothing(ext, NR, "cuda")


def test_wf_retire_appends_after_a_preset_count(ext):
    """The done list is appended at the counter, whatever it holds: records
    of an earlier call are kept below it."""
    t = dict(build_retire_tables(257))
    t["done_count"] = torch.tensor([3], dtype=torch.int32)
    for k in ("done_slot", "done_gen", "done_state"):
        t[k] = torch.cat([t[k], torch.full((3,), POISON, dtype=torch.int32)])
    want = call(ref_ops(), "wf_retire", t)
    got = call(ext, "wf_retire", t, "cuda")
    assert int(got["done_count"][0]) == int(want["done_count"][0]) > 3
    n = int(want["done_count"][0])
    key = lambda d: sorted(zip(d["done_slot"][3:n].tolist(), d["done_gen"][3:n].tolist(),
                               d["done_state"][3:n].tolist()))
    assert key(got) == key(want)
    assert got["done_slot"][:3].tolist() == [POISON] * 3
    assert torch.equal(got["run_life"], want["run_life"])
