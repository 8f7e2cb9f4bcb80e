"""Per-kernel GPU tests of the device workflow engine (K3 / K3-WF / K4-WF).

Every extension function is called directly on small hand-built tables and
compared with its line-for-line oracle in cordum_amd/ops/reference.py, run
on CPU clones of the same tables. All values are integers: every comparison
is exact equality. Lists appended through the wave-aggregated compaction
have no defined order, so they are compared as sorted sets and their
counters exactly.

The table builders and the "the case is the case" assertions are
module-level functions: tests/test_wf_kernel_cases.py runs each builder
through its oracle on a machine without a GPU, so a later edit to a builder
cannot quietly empty one of the GPU tests below.
"""
import functools

import pytest
import torch

from cordum_amd.ops import reference as ref
from cordum_amd.ops.reference import (
    WFK_APPROVAL, WFK_CONDITION, WFK_DELAY, WFK_FOR_EACH, WFK_WORKER,
    WFS_DISPATCHED, WFS_FAILED, WFS_PENDING, WFS_SKIPPED, WFS_SUCCEEDED,
    WFS_WAITING,
)

pytestmark = pytest.mark.gpu

# one lane, the 64-lane wave edge, the 256-thread block edge, and a third
# block with a single live lane
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
POISON = -7
I64_MIN = -(1 << 63)
BIG = 1 << 33  # preset of the 64-bit counters: a 32-bit add would show

WF_ARGS = {
    "wf_sweep": ("step_state", "deps_mask", "n_steps", "run_active", "step_kind",
                 "cond_bits", "next_ready", "tick", "disp_runs", "disp_steps",
                 "disp_count", "appr_runs", "appr_steps", "appr_count"),
    "wf_expand": ("disp_runs", "disp_steps", "disp_count", "step_state",
                  "children_todo", "children_out", "max_parallel", "child_tag",
                  "child_seq", "child_widx", "child_count", "children_emitted",
                  "dispatch_tick", "tick", "order", "valid_count"),
    "wf_apply": ("send_slots", "send_cnt", "child_tag", "child_seq", "rq_prev_tag",
                 "rq_prev_seq", "children_done", "children_fail", "children_out",
                 "fail_ppt", "drop_ppt", "cap", "world"),
    "wf_apply_dead": ("dead_src", "dead_count", "child_tag", "rq_prev_tag",
                      "children_fail", "children_out"),
    "wf_timeout_scan": ("step_state", "children_out", "children_fail",
                        "dispatch_tick", "tick", "cutoff", "timeout_count"),
    "wf_commit": ("step_state", "step_attempts", "children_todo", "children_out",
                  "children_done", "children_fail", "max_parallel", "next_ready",
                  "tick", "max_retries", "retry_count"),
    "wf_status": ("step_state", "n_steps", "run_active", "run_state", "counts"),
    "wf_grant": ("grant_runs", "grant_steps", "verdicts", "n", "step_state"),
    "wf_readmit": ("run_active", "run_state", "n_steps", "step_state",
                   "step_attempts", "children_todo", "children_out",
                   "children_done", "children_fail", "children_emitted",
                   "next_ready", "dispatch_tick", "todo_tmpl", "nready_tmpl",
                   "filter_state", "admit_count"),
}


def ref_ops():
    from cordum_amd.ops.pipeline import _RefOps

    return _RefOps()


def call(ops, kernel, t, device="cpu"):
    """Run `kernel` of `ops` on clones of the tables in `t` (on `device`);
    returns every table as a CPU tensor. `t` itself is never written."""
    d = {k: (v.clone().to(device) if torch.is_tensor(v) else v) for k, v in t.items()}
    getattr(ops, kernel)(*[d[a] for a in WF_ARGS[kernel]])
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


def _i64(m: int) -> int:
    return m - (1 << 64) if m >= (1 << 63) else m


def _bits(ix) -> int:
    m = 0
    for i in ix:
        m |= 1 << i
    return m


def _rand_i64(n, g):
    hi = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int64, generator=g)
    lo = torch.randint(0, 1 << 32, (n,), dtype=torch.int64, generator=g)
    return (hi << 32) | lo


def _pairs(runs, steps, n):
    return sorted(zip(runs[:n].tolist(), steps[:n].tolist()))


# ---------------------------------------------------------------------------
# run_readiness / wf_sweep: the 64-step row
# ---------------------------------------------------------------------------
# Special rows sit at the END of the table (role p is run NR-1-p), so the
# tail lane of a partially filled wave or block always carries an edge row.
SWEEP_ROLES = ("all64", "only63", "both0_63", "cond63_set", "cond63_clear",
               "deps62", "resolve", "gates", "inactive", "dep_on_63")


def build_sweep_tables(NR, cap=None, acap=None, tick=5, seed=1):
    g = torch.Generator().manual_seed(seed * 1000 + NR)
    n = NR * 64
    s_idx = torch.arange(n) % 64
    t = {
        "n_steps": torch.randint(1, 65, (NR,), dtype=torch.uint8, generator=g),
        "step_state": torch.randint(0, 6, (n,), dtype=torch.uint8, generator=g),
        "step_kind": torch.randint(0, 5, (n,), dtype=torch.uint8, generator=g),
        "next_ready": (tick - 1 + torch.randint(0, 3, (n,), generator=g)).to(torch.int32),
        "run_active": (torch.rand(NR, generator=g) < 0.85).to(torch.uint8),
        "cond_bits": _rand_i64(NR, g),
        "tick": torch.tensor([tick], dtype=torch.int32),
    }
    t["step_state"][torch.rand(n, generator=g) < 0.4] = WFS_PENDING
    deps = torch.zeros(n, dtype=torch.int64)
    one = torch.ones(n, dtype=torch.int64)
    for _ in range(3):  # up to three dependencies on lower steps (bits <= 62)
        d = (torch.rand(n, generator=g) * s_idx).long()
        use = (torch.rand(n, generator=g) < 0.3) & (s_idx > 0)
        deps |= torch.where(use, one << d, torch.zeros_like(one))
    t["deps_mask"] = deps

    def fill(r, ns, states, kinds=None, deps=None, nready=None, cond=0, active=1):
        b = r * 64
        t["n_steps"][r] = ns
        t["run_active"][r] = active
        t["cond_bits"][r] = _i64(cond)
        for s in range(ns):
            t["step_state"][b + s] = states[s]
            t["step_kind"][b + s] = kinds[s] if kinds else WFK_WORKER
            t["deps_mask"][b + s] = _i64(deps.get(s, 0)) if deps else 0
            t["next_ready"][b + s] = nready[s] if nready else tick

    OK, PE = WFS_SUCCEEDED, WFS_PENDING
    roles = {}
    for p, name in enumerate(SWEEP_ROLES):
        r = NR - 1 - p
        if r < 0:
            break
        roles[name] = r
        if name == "all64":       # every step ready and dependency-free
            fill(r, 64, [PE] * 64, kinds=[s % 5 for s in range(64)],
                 nready=[tick - (s % 2) for s in range(64)],
                 cond=_bits(range(1, 64, 2)))
        elif name == "only63":    # the ready mask is the sign bit alone
            st = [OK] * 63 + [PE]
            st[10], st[20], st[30], st[40] = (WFS_DISPATCHED, WFS_WAITING,
                                              WFS_FAILED, WFS_SKIPPED)
            fill(r, 64, st, deps={63: _bits(s for s in range(63) if st[s] == OK)})
        elif name == "both0_63":  # lowest and highest bit together
            kinds = [WFK_WORKER] * 64
            kinds[0], kinds[63] = WFK_FOR_EACH, WFK_APPROVAL
            fill(r, 64, [PE] + [OK] * 62 + [PE], kinds=kinds)
        elif name in ("cond63_set", "cond63_clear"):
            fill(r, 64, [OK] * 63 + [PE], kinds=[WFK_WORKER] * 63 + [WFK_CONDITION],
                 deps={63: _bits(range(63))},
                 cond=(1 << 63) if name == "cond63_set" else (1 << 63) - 1)
        elif name == "deps62":    # 61 needs bits 0..60, 63 needs (unmet) bit 62
            kinds = [WFK_WORKER] * 64
            kinds[62] = WFK_FOR_EACH
            fill(r, 64, [OK] * 61 + [PE] * 3, kinds=kinds,
                 deps={61: _bits(range(61)), 63: 1 << 62})
        elif name == "resolve":   # steps that resolve now gate their dependents
            fill(r, 4, [PE] * 4,
                 kinds=[WFK_CONDITION, WFK_WORKER, WFK_DELAY, WFK_APPROVAL],
                 deps={1: 1, 3: 1 << 2}, cond=0)
        elif name == "gates":     # next_ready at tick-1, tick, tick+1
            fill(r, 3, [PE] * 3, nready=[tick - 1, tick, tick + 1])
        elif name == "inactive":
            fill(r, 64, [PE] * 64, kinds=[s % 5 for s in range(64)],
                 nready=[tick - 1] * 64, cond=-1 & ((1 << 64) - 1), active=0)
        elif name == "dep_on_63":  # bit 63 as a dependency (negative mask)
            fill(r, 64, [PE, PE] + [OK] * 60 + [WFS_FAILED, OK],
                 deps={0: 1 << 63, 1: (1 << 63) | (1 << 62)})
    t["roles"] = roles
    cap = NR * 64 if cap is None else cap
    acap = NR * 64 if acap is None else acap
    for nm, c in (("disp", cap), ("appr", acap)):
        t[nm + "_runs"] = torch.full((c,), POISON, dtype=torch.int32)
        t[nm + "_steps"] = torch.full((c,), POISON, dtype=torch.int32)
        t[nm + "_count"] = torch.zeros(1, dtype=torch.int32)
    return t


def resweep_tables(out):
    """The tables of a finished sweep, readied for the next one."""
    t = dict(out)
    for nm in ("disp", "appr"):
        t[nm + "_runs"] = torch.full_like(out[nm + "_runs"], POISON)
        t[nm + "_steps"] = torch.full_like(out[nm + "_steps"], POISON)
        t[nm + "_count"] = torch.zeros(1, dtype=torch.int32)
    return t


SWEEP_LISTS = ("disp_runs", "disp_steps", "appr_runs", "appr_steps")


def sweep_lists(out):
    nd, na = int(out["disp_count"][0]), int(out["appr_count"][0])
    nd_s, na_s = min(nd, out["disp_runs"].numel()), min(na, out["appr_runs"].numel())
    return (_pairs(out["disp_runs"], out["disp_steps"], nd_s),
            _pairs(out["appr_runs"], out["appr_steps"], na_s))


def assert_sweep_case(t, out, out2):
    """The case is the case, on the oracle's output of two sweeps."""
    NR = t["n_steps"].numel()
    roles, tick = t["roles"], int(t["tick"][0])
    assert "all64" in roles
    assert len(roles) == (len(SWEEP_ROLES) if NR >= 63 else min(NR, len(SWEEP_ROLES)))
    disp, appr = sweep_lists(out)
    disp2, _ = sweep_lists(out2)
    pre, post, kind = t["step_state"], out["step_state"], t["step_kind"]
    # each of the five step kinds fired at least once
    fired = {int(kind[r * 64 + s]) for r, s in disp}
    assert {WFK_WORKER, WFK_FOR_EACH} <= fired
    assert appr and all(int(post[r * 64 + s]) == WFS_WAITING for r, s in appr)
    was_pending = pre == WFS_PENDING
    assert bool((was_pending & (kind == WFK_CONDITION) & (post == WFS_SUCCEEDED)).any())
    assert bool((was_pending & (kind == WFK_CONDITION) & (post == WFS_SKIPPED)).any())
    assert bool((was_pending & (kind == WFK_DELAY) & (post == WFS_SUCCEEDED)).any())
    r = roles["all64"]
    assert sum(1 for p in disp if p[0] == r) + sum(1 for p in appr if p[0] == r) \
        + int(((kind[r * 64:r * 64 + 64] >= WFK_CONDITION)
               & (post[r * 64:r * 64 + 64] != WFS_PENDING)).sum()) == 64
    assert int(post[r * 64 + 63]) == WFS_SUCCEEDED  # CONDITION, bit 63 set
    if NR < 63:
        return
    r = roles["only63"]
    assert [p for p in disp if p[0] == r] == [(r, 63)]
    r = roles["both0_63"]
    assert [p for p in disp if p[0] == r] == [(r, 0)]
    assert [p for p in appr if p[0] == r] == [(r, 63)]
    assert int(post[roles["cond63_set"] * 64 + 63]) == WFS_SUCCEEDED
    assert int(post[roles["cond63_clear"] * 64 + 63]) == WFS_SKIPPED
    r = roles["deps62"]
    assert [p for p in disp if p[0] == r] == [(r, 61), (r, 62)]
    r = roles["resolve"]  # the pre-sweep satisfied mask gates the dependents
    assert post[r * 64:r * 64 + 4].tolist() == [WFS_SKIPPED, WFS_PENDING,
                                                WFS_SUCCEEDED, WFS_PENDING]
    assert not [p for p in disp + appr if p[0] == r]
    assert (r, 1) in disp2
    assert int(out2["step_state"][r * 64 + 3]) == WFS_WAITING
    r = roles["gates"]
    assert [p for p in disp if p[0] == r] == [(r, 0), (r, 1)]
    assert t["next_ready"][r * 64:r * 64 + 3].tolist() == [tick - 1, tick, tick + 1]
    r = roles["inactive"]
    assert not [p for p in disp + appr if p[0] == r]
    assert torch.equal(post[r * 64:r * 64 + 64], pre[r * 64:r * 64 + 64])
    r = roles["dep_on_63"]
    assert [p for p in disp if p[0] == r] == [(r, 0)]
    assert int(t["deps_mask"][r * 64]) == I64_MIN


@functools.lru_cache(maxsize=None)
def sweep_oracle(NR, cap=None, acap=None):
    t = build_sweep_tables(NR, cap, acap)
    out = call(ref_ops(), "wf_sweep", t)
    out2 = call(ref_ops(), "wf_sweep", resweep_tables(out))
    return t, out, out2


@functools.lru_cache(maxsize=None)
def readiness_oracle(NR):
    t = build_sweep_tables(NR)
    ready, pairs = ref.run_readiness_ref(t["step_state"].view(NR, 64),
                                         t["deps_mask"].view(NR, 64),
                                         t["n_steps"], t["run_active"])
    return t, ready, sorted(pairs)


def assert_readiness_case(t, ready, pairs):
    NR, roles = t["n_steps"].numel(), t["roles"]
    r = roles["all64"]
    assert int(ready[r]) == -1 and [p for p in pairs if p[0] == r] == [(r, s) for s in range(64)]
    if NR < 63:
        return
    assert int(ready[roles["only63"]]) == I64_MIN
    assert int(ready[roles["both0_63"]]) == _i64((1 << 63) | 1)
    assert int(ready[roles["deps62"]]) == _i64(_bits([61, 62]))
    assert int(ready[roles["dep_on_63"]]) == 1
    assert int(ready[roles["inactive"]]) == 0


def run_readiness_dev(ext, t, cap):
    NR, d = t["n_steps"].numel(), "cuda:0"
    ready, runs, steps, count = ext.run_readiness(
        t["step_state"].view(NR, 64).to(d), t["deps_mask"].view(NR, 64).to(d),
        t["n_steps"].to(d), t["run_active"].to(d), cap)
    return ready.cpu(), runs.cpu(), steps.cpu(), int(count.cpu()[0])


def assert_capped_prefix(got_pairs, count, cap, full):
    """A compaction that overflowed: `cap` distinct entries, all drawn from
    the set an ample cap yields."""
    assert count > cap, "the case must overflow"
    assert len(got_pairs) == cap
    assert len(set(got_pairs)) == cap
    assert set(got_pairs) <= set(full)


# ---------------------------------------------------------------------------
# deadline_scan overflow
# ---------------------------------------------------------------------------
def build_deadline_tables(N, seed=9):
    g = torch.Generator().manual_seed(seed + N)
    t = {
        "states": torch.randint(0, 11, (N,), dtype=torch.uint8, generator=g),
        "deadlines": torch.randint(0, 2_000_000, (N,), dtype=torch.int64, generator=g),
        "updated_at": torch.randint(0, 2_000_000, (N,), dtype=torch.int64, generator=g),
        "now": 1_000_000, "dispatch_cutoff": 500_000, "running_cutoff": 100_000,
    }
    # the output buffer is allocated by the launcher and cannot be poisoned:
    # slot 0 is kept un-expired instead, so a stale zero is not a valid entry
    t["states"][0] = 0
    t["want"] = ref.deadline_scan_ref(t["states"], t["deadlines"], t["updated_at"],
                                      t["now"], t["dispatch_cutoff"], t["running_cutoff"])
    return t


# ---------------------------------------------------------------------------
# wf_expand
# ---------------------------------------------------------------------------
TODOS = (1, 63, 64, 65, 200)
ORDER_LEN = 1500


def std_entries(n_entries, NR=65, todos=None):
    """(run, step, todo, out, maxp, emitted) on distinct cells, never cell 0."""
    out = []
    for i in range(n_entries):
        todo = todos[i] if todos else TODOS[(i + n_entries) % 5]
        out.append(((3 + 29 * i) % NR, (63 - 5 * i) % 64, todo,
                    0 if i % 2 == 0 else 4, 0, 3 + 11 * i))
    cells = {(e[0], e[1]) for e in out}
    assert len(cells) == n_entries and (0, 0) not in cells
    return out


def build_expand_tables(entries, NR=65, CB=2048, disp_len=None, disp_count=None,
                        valid_count=ORDER_LEN, child_count0=0, tick=9, seed=3):
    g = torch.Generator().manual_seed(seed)
    n = NR * 64
    disp_len = len(entries) if disp_len is None else disp_len
    assert len(entries) <= disp_len
    t = {
        "step_state": torch.randint(0, 6, (n,), dtype=torch.uint8, generator=g),
        "children_todo": torch.randint(0, 50, (n,), dtype=torch.int32, generator=g),
        "children_out": torch.randint(0, 50, (n,), dtype=torch.int32, generator=g),
        "max_parallel": torch.randint(0, 50, (n,), dtype=torch.int32, generator=g),
        "children_emitted": torch.randint(0, 1000, (n,), dtype=torch.int32, generator=g),
        "dispatch_tick": torch.randint(0, tick, (n,), dtype=torch.int32, generator=g),
        # unused list slots name cell 0, which no entry uses: a stray read of
        # them shows up as a change to cell 0
        "disp_runs": torch.zeros(disp_len, dtype=torch.int32),
        "disp_steps": torch.zeros(disp_len, dtype=torch.int32),
        "disp_count": torch.tensor(
            [len(entries) if disp_count is None else disp_count], dtype=torch.int32),
        "child_tag": torch.full((CB,), POISON, dtype=torch.int32),
        "child_seq": torch.full((CB,), POISON, dtype=torch.int32),
        "child_widx": torch.full((CB,), POISON, dtype=torch.int32),
        "child_count": torch.tensor([child_count0], dtype=torch.int32),
        "tick": torch.tensor([tick], dtype=torch.int32),
        "order": torch.randint(0, 5000, (ORDER_LEN,), dtype=torch.int32, generator=g),
        "valid_count": torch.tensor([valid_count], dtype=torch.int32),
    }
    for e, (run, step, todo, out, maxp, emitted) in enumerate(entries):
        rs = run * 64 + step
        t["disp_runs"][e], t["disp_steps"][e] = run, step
        t["step_state"][rs] = WFS_PENDING
        t["children_todo"][rs], t["children_out"][rs] = todo, out
        t["max_parallel"][rs], t["children_emitted"][rs] = maxp, emitted
    t["entries"] = list(entries)
    return t


EXPAND_TABLES = ("step_state", "children_todo", "children_out", "children_emitted",
                 "dispatch_tick", "child_count")
EXPAND_ARENA = ("child_tag", "child_seq", "child_widx")


def expand_layout(pre, got):
    """Order-free layout facts of the child arena after a wf_expand call.
    Returns {tag: children emitted for it}."""
    c0, cnt = int(pre["child_count"][0]), int(got["child_count"][0])
    CB = pre["child_tag"].numel()
    assert c0 <= cnt <= CB
    for k in EXPAND_ARENA:  # untouched outside [c0, cnt)
        assert bool((got[k][cnt:] == POISON).all()), k
        assert torch.equal(got[k][:c0], pre[k][:c0]), k
    V = min(max(1, int(pre["valid_count"][0])), 1024)
    pos = torch.arange(c0, cnt)
    assert torch.equal(got["child_widx"][c0:cnt], pre["order"][pos % V])
    tags, seqs = got["child_tag"][c0:cnt].tolist(), got["child_seq"][c0:cnt].tolist()
    cells = {e[0] * 64 + e[1] for e in pre["entries"]}
    seen, p = {}, 0
    while p < len(tags):  # one contiguous range per tag, seq ascending
        tg, q = tags[p], p
        assert tg in cells and tg not in seen
        while q < len(tags) and tags[q] == tg:
            q += 1
        e0 = int(pre["children_emitted"][tg])
        assert seqs[p:q] == list(range(e0, e0 + q - p))
        seen[tg], p = q - p, q
    return seen


def assert_expand_matches(pre, got, want):
    """Equal to the oracle in everything that does not depend on the order
    in which the waves reserved their ranges."""
    assert_tables_equal(got, want, skip=EXPAND_ARENA + ("entries",))
    seen = expand_layout(pre, got)
    c0, cnt = int(pre["child_count"][0]), int(want["child_count"][0])
    pairs = lambda o: sorted(zip(o["child_tag"][c0:cnt].tolist(),
                                 o["child_seq"][c0:cnt].tolist()))
    assert pairs(got) == pairs(want)
    return seen


def expand_window(todo, out, maxp):
    """Children one entry may emit now (the max_parallel window)."""
    if maxp > 0 and maxp - out < todo:
        return max(0, maxp - out)
    return todo


def assert_expand_all_or_nothing(pre, got):
    """Arena backpressure invariants: each entry fully emitted or wholly
    untouched, ranges dense and disjoint, the counter equal to their sum."""
    seen = expand_layout(pre, got)
    tick = int(pre["tick"][0])
    touched = torch.zeros(pre["step_state"].numel(), dtype=torch.bool)
    total = 0
    for run, step, todo, out, maxp, emitted in pre["entries"]:
        rs = run * 64 + step
        touched[rs] = True
        k = seen.get(rs, 0)
        if k:
            assert k == expand_window(todo, out, maxp)
            assert int(got["step_state"][rs]) == WFS_DISPATCHED
            assert int(got["children_todo"][rs]) == todo - k
            assert int(got["children_out"][rs]) == out + k
            assert int(got["children_emitted"][rs]) == emitted + k
            assert int(got["dispatch_tick"][rs]) == tick
            total += k
        else:
            for name in EXPAND_TABLES[:-1]:
                assert int(got[name][rs]) == int(pre[name][rs]), (name, rs)
    assert int(got["child_count"][0]) == int(pre["child_count"][0]) + total
    for name in EXPAND_TABLES[:-1]:  # cells that were not dispatched
        assert torch.equal(got[name][~touched], pre[name][~touched]), name
    return seen


MAXP_ENTRIES = (
    # run, step, todo, out, maxp, emitted
    (5, 63, 50, 5, 20, 7),    # window smaller than todo: emits 15
    (6, 1, 10, 8, 8, 0),      # window equal to children_out: DISPATCHED, emits 0
    (7, 2, 10, 3, 0, 9),      # maxp == 0: unlimited
    (8, 3, 5, 9, 8, 2),       # window overrun: DISPATCHED, emits 0
    (9, 4, 0, 0, 0, 4),       # nothing to do, nothing in flight: stays PENDING
    (64, 62, 4, 0, 100, 1),   # window larger than todo
)

ARENA_CB = 130  # no multiple of the wave
ARENA_SINGLE = {
    # name: (todo, child_count0, fits)
    "exact_fit": (ARENA_CB, 0, True),
    "one_over": (ARENA_CB + 1, 0, False),
    "preset_over": (31, 100, False),
    "preset_exact": (30, 100, True),
}


def build_arena_single(name):
    todo, c0, _ = ARENA_SINGLE[name]
    t = build_expand_tables([(64, 63, todo, 2, 0, 17)], CB=ARENA_CB, child_count0=c0)
    for k in EXPAND_ARENA:  # the reserved prefix holds earlier children
        t[k][:c0] = torch.arange(c0, dtype=torch.int32) + 100000
    return t


ARENA_MANY = {
    # name: (CB, todos) — the total exceeds CB
    "fits_each_9": (300, (63, 64, 65, 200, 1, 63, 64, 65, 200)),
    "fits_each_40": (300, tuple(TODOS[i % 5] for i in range(40))),
    # the first entry can never fit; the oracle still emits the others
    "oversized_2": (300, (301, 200)),
    "oversized_4": (300, (301, 1, 63, 64)),
    "oversized_9": (300, (301, 63, 64, 65, 1, 63, 64, 65, 200)),
}


def build_arena_many(name):
    CB, todos = ARENA_MANY[name]
    ents = std_entries(len(todos), todos=todos)
    ents = [(r, s, td, 0, 0, em) for r, s, td, _, _, em in ents]
    return build_expand_tables(ents, CB=CB)


# ---------------------------------------------------------------------------
# wf_apply / wf_apply_dead
# ---------------------------------------------------------------------------
APPLY_PPT = ((0, 0), (1000, 0), (0, 1000), (150, 100))
APPLY_NR, APPLY_CB, APPLY_RQ = 65, 700, 200


def _apply_common(one_tag, g):
    n = APPLY_NR * 64
    if one_tag:  # every atomic lands on one address (the last cell)
        ctag = torch.full((APPLY_CB,), n - 1, dtype=torch.int32)
        rtag = torch.full((APPLY_RQ,), n - 1, dtype=torch.int32)
    else:
        ctag = torch.randint(0, n, (APPLY_CB,), dtype=torch.int32, generator=g)
        rtag = torch.randint(0, n, (APPLY_RQ,), dtype=torch.int32, generator=g)
    return {
        "child_tag": ctag, "rq_prev_tag": rtag,
        "child_seq": torch.arange(APPLY_CB, dtype=torch.int32) + 1000,
        "rq_prev_seq": torch.arange(APPLY_RQ, dtype=torch.int32) + 50000,
        "children_done": torch.randint(0, 100, (n,), dtype=torch.int32, generator=g),
        "children_fail": torch.randint(0, 100, (n,), dtype=torch.int32, generator=g),
        "children_out": torch.randint(500, 1000, (n,), dtype=torch.int32, generator=g),
    }


def _slots_with_redeliveries(n, g):
    """About a third negative: -1-j names row j of the requeue carry."""
    s = torch.randint(0, APPLY_CB, (n,), dtype=torch.int32, generator=g)
    j = torch.randint(0, APPLY_RQ, (n,), dtype=torch.int32, generator=g)
    return torch.where(torch.rand(n, generator=g) < 1 / 3, -1 - j, s)


def apply_send_counts(world, cap, ppt_idx):
    """Per rank: 0, below cap, equal to cap, above cap (must clamp)."""
    modes = (0, cap // 2, cap, cap + 7)
    return [modes[(r + ppt_idx) % 4] for r in range(world)]


def build_apply_tables(world, cap, one_tag, ppt_idx):
    g = torch.Generator().manual_seed(5 + world * 1000 + cap * 10 + ppt_idx)
    t = _apply_common(one_tag, g)
    t["send_slots"] = _slots_with_redeliveries(world * cap, g)
    t["send_cnt"] = torch.tensor(apply_send_counts(world, cap, ppt_idx), dtype=torch.int32)
    t["fail_ppt"], t["drop_ppt"] = APPLY_PPT[ppt_idx]
    t["cap"], t["world"] = cap, world
    return t


def apply_outcomes(t):
    """(dropped, failed, done, redelivered) among the entries wf_apply reads."""
    drop = fail = done = neg = 0
    cap = t["cap"]
    for r in range(t["world"]):
        for e in range(min(int(t["send_cnt"][r]), cap)):
            s = int(t["send_slots"][r * cap + e])
            neg += s < 0
            tag = int(t["child_tag"][s]) if s >= 0 else int(t["rq_prev_tag"][-1 - s])
            seq = int(t["child_seq"][s]) if s >= 0 else int(t["rq_prev_seq"][-1 - s])
            if ref.wf_drop_hash(tag, seq) % 1000 < t["drop_ppt"]:
                drop += 1
            elif ref.wf_fail_hash(tag, seq) % 1000 < t["fail_ppt"]:
                fail += 1
            else:
                done += 1
    return drop, fail, done, neg


def assert_apply_case(t):
    cap, world = t["cap"], t["world"]
    cnt = t["send_cnt"].tolist()
    if world == 4:
        assert sorted(cnt) == sorted((0, cap // 2, cap, cap + 7))
    drop, fail, done, neg = apply_outcomes(t)
    total = drop + fail + done
    assert total == sum(min(c, cap) for c in cnt)
    ppt = (t["fail_ppt"], t["drop_ppt"])
    if ppt == (0, 0):
        assert done == total
    elif ppt == (1000, 0):
        assert fail == total
    elif ppt == (0, 1000):
        assert drop == total
    elif total >= 100:  # ~15% fail, ~10% drop: all three outcomes occur
        assert drop > 0 and fail > 0 and done > 0
    if total >= 30:
        assert 0 < neg < total


DEAD_COUNTS = ("zero", "below", "above")


def build_apply_dead_tables(dcap, one_tag, count_mode):
    g = torch.Generator().manual_seed(17 + dcap)
    t = _apply_common(one_tag, g)
    t["dead_src"] = _slots_with_redeliveries(dcap, g)
    t["dead_count"] = torch.tensor(
        [{"zero": 0, "below": (dcap + 1) // 2, "above": dcap + 9}[count_mode]],
        dtype=torch.int32)
    return t


# ---------------------------------------------------------------------------
# wf_timeout_scan
# ---------------------------------------------------------------------------
TIMEOUT_TICK, TIMEOUT_CUTOFF = 100, 8


def build_timeout_tables(NR):
    g = torch.Generator().manual_seed(23 + NR)
    n = NR * 64
    i = torch.arange(n)
    edge = TIMEOUT_TICK - TIMEOUT_CUTOFF
    # the 3 x 3 x 6 product of (dispatch_tick, children_out, state), cycled
    dticks = torch.tensor([edge - 1, edge, edge + 1], dtype=torch.int32)
    outs = torch.tensor([0, 1, 70], dtype=torch.int32)
    return {
        "dispatch_tick": dticks[i % 3],
        "children_out": outs[(i // 3) % 3],
        "step_state": ((i // 9) % 6).to(torch.uint8),
        "children_fail": torch.randint(0, 50, (n,), dtype=torch.int32, generator=g),
        "tick": torch.tensor([TIMEOUT_TICK], dtype=torch.int32),
        "cutoff": TIMEOUT_CUTOFF,
        "timeout_count": torch.tensor([BIG + 5], dtype=torch.int64),
    }


def assert_timeout_case(t, out):
    edge = TIMEOUT_TICK - TIMEOUT_CUTOFF
    fired = out["children_out"] != t["children_out"]
    disp = t["step_state"] == WFS_DISPATCHED
    assert bool(fired.any()) and not bool((fired & ~disp).any())
    assert bool((fired & (t["dispatch_tick"] == edge)).any())       # boundary fires
    assert bool((fired & (t["dispatch_tick"] == edge - 1)).any())
    assert not bool((fired & (t["dispatch_tick"] == edge + 1)).any())
    assert bool((disp & (t["dispatch_tick"] == edge + 1) & (t["children_out"] > 0)).any())
    assert bool((fired & (t["children_out"] == 70)).any())
    assert bool((fired & (t["children_out"] == 1)).any())
    for s in range(6):  # every step state meets an expired, in-flight cell
        assert bool(((t["step_state"] == s) & (t["dispatch_tick"] <= edge)
                     & (t["children_out"] > 0)).any())
    lost = int(t["children_out"][fired].sum())
    assert int(out["timeout_count"][0]) == BIG + 5 + lost > BIG + 5


# ---------------------------------------------------------------------------
# wf_commit
# ---------------------------------------------------------------------------
COMMIT_TICK, COMMIT_MAX_RETRIES = 1000, 64
BACKOFF_ATTEMPTS = (0, 3, 4, 29, 30, 31, 40)
# branch: (state, attempts, todo, out, fail, maxp) -> expected state after
COMMIT_BRANCHES = {
    "pending_untouched": ((WFS_PENDING, 1, 3, 0, 2, 0), WFS_PENDING),
    "waiting_untouched": ((WFS_WAITING, 1, 3, 0, 2, 0), WFS_WAITING),
    "succeeded_untouched": ((WFS_SUCCEEDED, 1, 3, 0, 2, 0), WFS_SUCCEEDED),
    "failed_untouched": ((WFS_FAILED, 1, 3, 0, 2, 0), WFS_FAILED),
    "skipped_untouched": ((WFS_SKIPPED, 1, 3, 0, 2, 0), WFS_SKIPPED),
    "inflight_more_unlimited": ((WFS_DISPATCHED, 0, 5, 3, 1, 0), WFS_PENDING),
    "inflight_more_room": ((WFS_DISPATCHED, 0, 5, 3, 1, 4), WFS_PENDING),
    "inflight_window_limit": ((WFS_DISPATCHED, 0, 5, 3, 1, 3), WFS_DISPATCHED),
    "inflight_window_over": ((WFS_DISPATCHED, 0, 5, 3, 1, 2), WFS_DISPATCHED),
    "inflight_no_more": ((WFS_DISPATCHED, 0, 0, 3, 1, 0), WFS_DISPATCHED),
    "retries_exhausted": ((WFS_DISPATCHED, COMMIT_MAX_RETRIES, 2, 0, 4, 0), WFS_FAILED),
    "retries_over": ((WFS_DISPATCHED, COMMIT_MAX_RETRIES + 1, 2, 0, 4, 0), WFS_FAILED),
    "partial_resume": ((WFS_DISPATCHED, 2, 6, 0, 0, 0), WFS_PENDING),
    "success": ((WFS_DISPATCHED, 2, 0, 0, 0, 0), WFS_SUCCEEDED),
}
for _a in BACKOFF_ATTEMPTS + (COMMIT_MAX_RETRIES - 1,):
    COMMIT_BRANCHES[f"retry_{_a}"] = ((WFS_DISPATCHED, _a, 2, 0, 3 + _a % 3, 0), WFS_PENDING)
COMMIT_NAMES = tuple(COMMIT_BRANCHES)


def build_commit_tables(NR):
    g = torch.Generator().manual_seed(29 + NR)
    n = NR * 64
    assert len(COMMIT_NAMES) <= 64  # a single run holds every branch
    rows = torch.tensor([COMMIT_BRANCHES[k][0] for k in COMMIT_NAMES], dtype=torch.int32)
    # a stride coprime to the catalogue length walks the branches across
    # wave and block boundaries
    branch = (torch.arange(n) * 5 + torch.arange(n) // 64) % len(COMMIT_NAMES)
    if NR == 1:
        branch = torch.arange(n) % len(COMMIT_NAMES)
    c = rows[branch]
    return {
        "branch": branch,
        "step_state": c[:, 0].to(torch.uint8),
        "step_attempts": c[:, 1].contiguous(),
        "children_todo": c[:, 2].contiguous(),
        "children_out": c[:, 3].contiguous(),
        "children_fail": c[:, 4].contiguous(),
        "max_parallel": c[:, 5].contiguous(),
        "children_done": torch.randint(0, 100, (n,), dtype=torch.int32, generator=g),
        "next_ready": torch.randint(-50, 50, (n,), dtype=torch.int32, generator=g),
        "tick": torch.tensor([COMMIT_TICK], dtype=torch.int32),
        "max_retries": COMMIT_MAX_RETRIES,
        "retry_count": torch.tensor([BIG + 1], dtype=torch.int64),
    }


def assert_commit_case(t, out):
    """Every branch is present and the oracle took it."""
    retried = 0
    for b, name in enumerate(COMMIT_NAMES):
        (st, att, todo, _, fail, _), want_state = COMMIT_BRANCHES[name]
        cells = torch.nonzero(t["branch"] == b).flatten()
        assert cells.numel() > 0, name
        assert bool((out["step_state"][cells] == want_state).all()), name
        if name.startswith("retry_"):
            # the oracle's rule: tick + min(2**attempts, 16)
            want = COMMIT_TICK + min(2 ** (att + 1), 16)
            assert out["next_ready"][cells].tolist() == [want] * cells.numel(), name
            assert bool((out["step_attempts"][cells] == att + 1).all())
            assert bool((out["children_todo"][cells] == todo + fail).all())
            assert bool((out["children_fail"][cells] == 0).all())
            retried += fail * cells.numel()
        else:
            for k in ("step_attempts", "children_todo", "children_fail", "next_ready"):
                assert torch.equal(out[k][cells], t[k][cells]), (name, k)
    assert {COMMIT_TICK + 2, COMMIT_TICK + 16} <= set(out["next_ready"].tolist())
    assert int(out["retry_count"][0]) == BIG + 1 + retried > BIG + 1


# ---------------------------------------------------------------------------
# wf_status / wf_grant / wf_readmit
# ---------------------------------------------------------------------------
STATUS_ROLES = {
    # name: (n_steps, states, active, want run_state (None: untouched))
    "failed_at_63": (64, [WFS_SUCCEEDED] * 63 + [WFS_FAILED], 1, WFS_FAILED),
    "one_step_ok": (1, [WFS_SUCCEEDED], 1, WFS_SUCCEEDED),
    "one_step_pending": (1, [WFS_PENDING], 1, None),
    "skipped_satisfies": (64, [WFS_SUCCEEDED, WFS_SKIPPED] * 32, 1, WFS_SUCCEEDED),
    "failed_and_pending": (64, [WFS_PENDING] + [WFS_SUCCEEDED] * 62 + [WFS_FAILED], 1,
                           WFS_FAILED),
    "inactive": (64, [WFS_SUCCEEDED] * 64, 0, None),
    "pending_at_63": (64, [WFS_SUCCEEDED] * 63 + [WFS_PENDING], 1, None),
    "failed_past_end": (5, [WFS_SUCCEEDED] * 5 + [WFS_FAILED] * 59, 1, WFS_SUCCEEDED),
}
STATUS_NAMES = tuple(STATUS_ROLES)
RUN_STATE_POISON = 9


def build_status_tables(NR):
    g = torch.Generator().manual_seed(31 + NR)
    n = NR * 64
    t = {
        "n_steps": torch.randint(1, 65, (NR,), dtype=torch.uint8, generator=g),
        "run_active": (torch.rand(NR, generator=g) < 0.8).to(torch.uint8),
        "run_state": torch.full((NR,), RUN_STATE_POISON, dtype=torch.uint8),
        "counts": torch.tensor([BIG, 2 * BIG + 1], dtype=torch.int64),
    }
    # mostly satisfied cells, so random runs reach all three verdicts
    st = torch.full((n,), WFS_SUCCEEDED, dtype=torch.uint8)
    u = torch.rand(n, generator=g)
    st[u < 0.3] = WFS_SKIPPED
    st[u < 0.02] = WFS_PENDING
    st[u < 0.01] = WFS_FAILED
    t["step_state"] = st
    roles = {}
    for p, name in enumerate(STATUS_NAMES):
        r = NR - 1 - p
        if r < 0:
            break
        ns, states, active, _ = STATUS_ROLES[name]
        roles[name] = r
        t["n_steps"][r], t["run_active"][r] = ns, active
        st[r * 64:r * 64 + len(states)] = torch.tensor(states, dtype=torch.uint8)
    t["roles"] = roles
    return t


def assert_status_case(t, out):
    NR = t["n_steps"].numel()
    assert len(t["roles"]) == min(NR, len(STATUS_NAMES))
    for name, r in t["roles"].items():
        want = STATUS_ROLES[name][3]
        if want is None:
            assert int(out["run_state"][r]) == RUN_STATE_POISON, name
            assert int(out["run_active"][r]) == int(t["run_active"][r]), name
        else:
            assert int(out["run_state"][r]) == want and int(out["run_active"][r]) == 0, name
    ok = int(((out["run_state"] == WFS_SUCCEEDED)).sum())
    bad = int(((out["run_state"] == WFS_FAILED)).sum())
    assert out["counts"].tolist() == [BIG + ok, 2 * BIG + 1 + bad]
    assert ok + bad > 0
    assert torch.equal(out["step_state"], t["step_state"])


GRANT_NS = (0, 1, 65, 257, 600)
GRANT_NR = 65


def build_grant_tables(n_grants):
    g = torch.Generator().manual_seed(37 + n_grants)
    n = GRANT_NR * 64
    total = 700  # the lists are longer than n: the tail must be ignored
    # distinct cells; the first grant names the last cell (run 64, step 63)
    cells = torch.cat([torch.tensor([n - 1]),
                       torch.randperm(n - 1, generator=g)[:total - 1]])
    st = torch.randint(0, 6, (n,), dtype=torch.uint8, generator=g)
    st[cells[::2]] = WFS_WAITING  # half the grants hit a WAITING cell
    st[cells[GRANT_NS[-1]:]] = WFS_WAITING  # ... and so does the ignored tail
    return {
        "grant_runs": (cells // 64).to(torch.int32),
        "grant_steps": (cells % 64).to(torch.int32),
        "verdicts": (torch.arange(total) % 4 < 2).to(torch.uint8),
        "n": n_grants,
        "step_state": st,
    }


def assert_grant_case(t, out):
    n = t["n"]
    cells = (t["grant_runs"].long() * 64 + t["grant_steps"].long())
    assert cells.unique().numel() == cells.numel()  # no duplicate grants
    pre, post = t["step_state"], out["step_state"]
    changed = torch.nonzero(pre != post).flatten()
    assert set(changed.tolist()) <= set(cells[:n].tolist())
    assert bool((pre[changed] == WFS_WAITING).all())
    assert bool((pre[cells[n:]] == post[cells[n:]]).all())
    if n == 0:
        assert changed.numel() == 0
        return
    assert int(cells[0]) == GRANT_NR * 64 - 1 and int(pre[cells[0]]) == WFS_WAITING
    assert int(post[cells[0]]) == WFS_SUCCEEDED
    if n >= 65:  # both verdicts land, and non-WAITING cells are passed over
        hit = pre[cells[:n]] == WFS_WAITING
        assert bool(hit.any()) and bool((~hit).any())
        assert {WFS_SUCCEEDED, WFS_FAILED} <= set(post[cells[:n]][hit].tolist())


READMIT_TABLES = ("step_state", "step_attempts", "children_todo", "children_out",
                  "children_done", "children_fail", "children_emitted",
                  "next_ready", "dispatch_tick")


def build_readmit_tables(NR, filter_state):
    g = torch.Generator().manual_seed(41 + NR)
    n = NR * 64
    t = {k: torch.randint(100, 200, (n,), dtype=torch.int32, generator=g)
         for k in READMIT_TABLES[1:]}
    t["step_state"] = torch.randint(1, 6, (n,), dtype=torch.uint8, generator=g)
    t["todo_tmpl"] = torch.randint(0, 50, (n,), dtype=torch.int32, generator=g)
    t["nready_tmpl"] = torch.randint(0, 9, (n,), dtype=torch.int32, generator=g)
    t["n_steps"] = torch.randint(1, 65, (NR,), dtype=torch.uint8, generator=g)
    t["n_steps"][NR - 1] = 1 if NR > 1 else 63
    if NR > 1:
        t["n_steps"][NR - 2] = 64
    # the last rows: terminal in each state (one of them matches the filter)
    t["run_active"] = (torch.arange(NR) % 3 == 2).to(torch.uint8)
    t["run_state"] = torch.tensor([WFS_SUCCEEDED, WFS_FAILED, 0, WFS_SUCCEEDED],
                                  dtype=torch.uint8)[torch.arange(NR) % 4]
    if NR == 1:
        t["run_state"][0] = WFS_SUCCEEDED
    for r in range(max(0, NR - 2), NR if NR > 1 else 0):  # the 1- and 64-step runs match
        t["run_active"][r], t["run_state"][r] = 0, filter_state
    t["filter_state"] = filter_state
    t["admit_count"] = torch.tensor([BIG + 3], dtype=torch.int64)
    return t


def assert_readmit_case(t, out):
    NR, f = t["n_steps"].numel(), t["filter_state"]
    hit = (t["run_active"] == 0) & (t["run_state"] == f)
    assert int(out["admit_count"][0]) == BIG + 3 + int(hit.sum())
    if NR >= 63:
        assert bool(hit.any()) and bool((~hit & (t["run_active"] == 0)).any())
        assert bool((t["n_steps"][hit] < 64).any())
    elif f == WFS_SUCCEEDED:
        assert bool(hit.all())
    s_idx = (torch.arange(NR * 64) % 64)
    live = hit.repeat_interleave(64) & (s_idx < t["n_steps"].long().repeat_interleave(64))
    for k in READMIT_TABLES:  # steps at index >= n_steps, and other runs: untouched
        assert torch.equal(out[k][~live], t[k][~live]), k
    assert bool((out["step_state"][live] == WFS_PENDING).all())
    assert torch.equal(out["children_todo"][live], t["todo_tmpl"][live])
    assert torch.equal(out["next_ready"][live], t["nready_tmpl"][live])
    for k in ("step_attempts", "children_out", "children_done", "children_fail",
              "children_emitted", "dispatch_tick"):
        assert bool((out[k][live] == 0).all()), k
    assert bool((out["run_active"][hit] == 1).all()) and bool((out["run_state"][hit] == 0).all())


@functools.lru_cache(maxsize=None)
def oracle(kernel, builder, *args):
    """(tables, oracle output) of one builder call; shared and never written."""
    t = builder(*args)
    return t, call(ref_ops(), kernel, t)


# ===========================================================================
# the GPU tests
# ===========================================================================
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ext():
    from cordum_amd.ops import get_ext

    return get_ext(required=True)


@pytest.mark.parametrize("NR", SIZES)
def test_run_readiness_64_step_rows(ext, NR):
    t, want_ready, want_pairs = readiness_oracle(NR)
    assert_readiness_case(t, want_ready, want_pairs)
    ready, runs, steps, count = run_readiness_dev(ext, t, NR * 64)
    assert torch.equal(ready, want_ready)
    assert count == len(want_pairs)
    assert _pairs(runs, steps, count) == want_pairs


@pytest.mark.parametrize("NR", SIZES)
def test_wf_sweep_64_step_rows(ext, NR):
    t, want, want2 = sweep_oracle(NR)
    assert_sweep_case(t, want, want2)
    got = call(ext, "wf_sweep", t, DEV)
    assert_tables_equal(got, want, skip=SWEEP_LISTS + ("roles",))
    assert sweep_lists(got) == sweep_lists(want)
    for k in SWEEP_LISTS:  # nothing written past the counters
        n = int(want[k.split("_")[0] + "_count"][0])
        assert bool((got[k][n:] == POISON).all()), k
    # the next sweep sees what this one resolved
    got2 = call(ext, "wf_sweep", resweep_tables(got), DEV)
    assert_tables_equal(got2, want2, skip=SWEEP_LISTS + ("roles",))
    assert sweep_lists(got2) == sweep_lists(want2)


@pytest.mark.parametrize("NR,cap,acap", [(65, 1, 1), (257, 63, 7), (513, 300, 65)])
def test_wf_sweep_list_overflow(ext, NR, cap, acap):
    t, want, _ = sweep_oracle(NR, cap, acap)
    _, full, _ = sweep_oracle(NR)
    full_disp, full_appr = sweep_lists(full)
    got = call(ext, "wf_sweep", t, DEV)
    assert_tables_equal(got, want, skip=SWEEP_LISTS + ("roles",))  # counters too
    assert int(want["disp_count"][0]) == len(full_disp)
    assert int(want["appr_count"][0]) == len(full_appr)
    got_disp, got_appr = sweep_lists(got)
    assert_capped_prefix(got_disp, int(got["disp_count"][0]), cap, full_disp)
    assert_capped_prefix(got_appr, int(got["appr_count"][0]), acap, full_appr)


@pytest.mark.parametrize("NR,cap", [(65, 1), (257, 64), (513, 1000)])
def test_run_readiness_list_overflow(ext, NR, cap):
    t, want_ready, want_pairs = readiness_oracle(NR)
    ready, runs, steps, count = run_readiness_dev(ext, t, cap)
    assert torch.equal(ready, want_ready)
    assert count == len(want_pairs)
    assert_capped_prefix(_pairs(runs, steps, cap), count, cap, want_pairs)


@pytest.mark.parametrize("N,cap", [(257, 1), (257, 64), (1000, 65), (1000, None)])
def test_deadline_scan_overflow(ext, N, cap):
    t = build_deadline_tables(N)
    want = t["want"].tolist()
    cap = len(want) - 1 if cap is None else cap
    assert 0 not in want
    slots, count = ext.deadline_scan(t["states"].to(DEV), t["deadlines"].to(DEV),
                                     t["updated_at"].to(DEV), t["now"],
                                     t["dispatch_cutoff"], t["running_cutoff"], cap)
    assert slots.numel() == cap
    assert int(count.cpu()[0]) == len(want)
    assert_capped_prefix(slots.cpu().tolist(), len(want), cap, want)


def _expand_vs_oracle(ext, t):
    want = call(ref_ops(), "wf_expand", t)
    got = call(ext, "wf_expand", t, DEV)
    return want, got, assert_expand_matches(t, got, want)


@pytest.mark.parametrize("valid_count", [0, 1, 7, 1024, 1500])
@pytest.mark.parametrize("n_entries", [1, 3, 4, 5, 9])
def test_wf_expand_entries_and_spread(ext, n_entries, valid_count):
    t = build_expand_tables(std_entries(n_entries), valid_count=valid_count)
    want, got, seen = _expand_vs_oracle(ext, t)
    assert len(seen) == n_entries  # the arena is ample: every entry emitted
    assert int(want["child_count"][0]) == sum(e[2] for e in t["entries"])
    if n_entries >= 5:
        assert {e[2] for e in t["entries"]} == set(TODOS)


@pytest.mark.parametrize("todo", TODOS)
def test_wf_expand_single_entry(ext, todo):
    t = build_expand_tables(std_entries(1, todos=[todo]), valid_count=7)
    want, got, seen = _expand_vs_oracle(ext, t)
    assert list(seen.values()) == [todo]
    assert_tables_equal(got, want, skip=("entries",))  # one entry: no race at all


def test_wf_expand_max_parallel_window(ext):
    t = build_expand_tables(list(MAXP_ENTRIES))
    want, got, seen = _expand_vs_oracle(ext, t)
    cell = lambda e: e[0] * 64 + e[1]
    assert [seen.get(cell(e), 0) for e in MAXP_ENTRIES] == [15, 0, 10, 0, 0, 4]
    states = [int(want["step_state"][cell(e)]) for e in MAXP_ENTRIES]
    assert states == [WFS_DISPATCHED] * 4 + [WFS_PENDING, WFS_DISPATCHED]
    for e in (MAXP_ENTRIES[1], MAXP_ENTRIES[3]):  # window full: only the state moves
        for k in EXPAND_TABLES[1:-1]:
            assert int(want[k][cell(e)]) == int(t[k][cell(e)])


@pytest.mark.parametrize("disp_len,disp_count,expanded", [(5, 9, 5), (9, 5, 5), (9, 4, 4)])
def test_wf_expand_dispatch_count_clamp(ext, disp_len, disp_count, expanded):
    t = build_expand_tables(std_entries(disp_len), disp_count=disp_count)
    want, got, seen = _expand_vs_oracle(ext, t)
    cells = [e[0] * 64 + e[1] for e in t["entries"]]
    assert sorted(seen) == sorted(cells[:expanded])
    for rs in cells[expanded:]:
        assert int(got["step_state"][rs]) == WFS_PENDING


@pytest.mark.parametrize("name", list(ARENA_SINGLE))
def test_wf_expand_arena_full_single_entry(ext, name):
    t = build_arena_single(name)
    todo, c0, fits = ARENA_SINGLE[name]
    want, got, seen = _expand_vs_oracle(ext, t)
    assert_tables_equal(got, want, skip=("entries",))  # one entry: exact
    if fits:
        assert list(seen.values()) == [todo] and int(want["child_count"][0]) == ARENA_CB
    else:  # every table and the counter exactly as before
        assert c0 + todo == ARENA_CB + 1 and not seen
        assert_tables_equal(got, t, skip=("entries",))


@pytest.mark.parametrize("name", list(ARENA_MANY))
def test_wf_expand_arena_full_many_entries(ext, name):
    """The oracle is sequential and the kernel is not, so which entries win
    may differ: invariants, not equality. With the add-then-subtract rollback
    the kernel once had, `oversized_2` emitted nothing on the MI355X (the
    entry that can never fit inflated the counter while the other one
    reserved), where the oracle emits one entry."""
    t = build_arena_many(name)
    CB, todos = ARENA_MANY[name]
    want = call(ref_ops(), "wf_expand", t)
    assert sum(todos) > CB
    assert len(assert_expand_all_or_nothing(t, want)) >= 1  # the oracle emits some
    got = call(ext, "wf_expand", t, DEV)
    seen = assert_expand_all_or_nothing(t, got)
    assert int(got["child_count"][0]) <= CB
    assert len(seen) >= 1, "every entry rolled back although some fit"


@pytest.mark.parametrize("ppt_idx", range(4))
@pytest.mark.parametrize("one_tag", [True, False])
@pytest.mark.parametrize("cap", [1, 63, 65, 300])
@pytest.mark.parametrize("world", [1, 4])
def test_wf_apply_matches_reference(ext, world, cap, one_tag, ppt_idx):
    t, want = oracle("wf_apply", build_apply_tables, world, cap, one_tag, ppt_idx)
    assert_apply_case(t)
    got = call(ext, "wf_apply", t, DEV)
    assert_tables_equal(got, want)


@pytest.mark.parametrize("count_mode", DEAD_COUNTS)
@pytest.mark.parametrize("one_tag", [True, False])
@pytest.mark.parametrize("dcap", [1, 63, 65, 300])
def test_wf_apply_dead_matches_reference(ext, dcap, one_tag, count_mode):
    t, want = oracle("wf_apply_dead", build_apply_dead_tables, dcap, one_tag, count_mode)
    n = min(int(t["dead_count"][0]), dcap)
    assert n == {"zero": 0, "below": (dcap + 1) // 2, "above": dcap}[count_mode]
    assert int((want["children_fail"] - t["children_fail"]).sum()) == n
    assert int((t["children_out"] - want["children_out"]).sum()) == n
    got = call(ext, "wf_apply_dead", t, DEV)
    assert_tables_equal(got, want)


@pytest.mark.parametrize("NR", [1, 63, 65, 257])
def test_wf_timeout_scan_matches_reference(ext, NR):
    t, want = oracle("wf_timeout_scan", build_timeout_tables, NR)
    assert_timeout_case(t, want)
    assert NR == 1 or (NR * 64) % 256 != 0
    got = call(ext, "wf_timeout_scan", t, DEV)
    assert_tables_equal(got, want)


@pytest.mark.parametrize("NR", [1, 65, 257])
def test_wf_commit_matches_reference(ext, NR):
    """One cell per branch. The backoff rule is the oracle's,
    tick + min(2**attempts, 16): with `min(1 << attempts, 16)` the kernel
    gave tick + INT_MIN after 31 attempts and tick + 1 after 32 and 64."""
    t, want = oracle("wf_commit", build_commit_tables, NR)
    assert_commit_case(t, want)
    got = call(ext, "wf_commit", t, DEV)
    assert_tables_equal(got, want)


@pytest.mark.parametrize("NR", SIZES)
def test_wf_status_matches_reference(ext, NR):
    t, want = oracle("wf_status", build_status_tables, NR)
    assert_status_case(t, want)
    got = call(ext, "wf_status", t, DEV)
    assert_tables_equal(got, want, skip=("roles",))


@pytest.mark.parametrize("n_grants", GRANT_NS)
def test_wf_grant_matches_reference(ext, n_grants):
    t, want = oracle("wf_grant", build_grant_tables, n_grants)
    assert_grant_case(t, want)
    got = call(ext, "wf_grant", t, DEV)
    assert_tables_equal(got, want)


@pytest.mark.parametrize("filter_state", [WFS_SUCCEEDED, WFS_FAILED])
@pytest.mark.parametrize("NR", SIZES)
def test_wf_readmit_matches_reference(ext, NR, filter_state):
    t, want = oracle("wf_readmit", build_readmit_tables, NR, filter_state)
    assert_readmit_case(t, want)
    got = call(ext, "wf_readmit", t, DEV)
    assert_tables_equal(got, want)
