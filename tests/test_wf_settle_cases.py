"""The per-step-policy pass (wf_settle) on hand-built tables, oracle only: no
GPU is needed here.

The table builders and the checks are module-level functions, and
tests/test_gpu_wf_settle.py imports them to run the HIP kernel on the same
cases. A builder plants steps by role and records what a correct pass owes
for each, so the expected tables are known without running the code under
test; every cell nobody owes anything for holds a poison value before and
must hold it afterwards.

Layout edges. The pass has 4 lanes per row (16 steps each), 16 rows per wave
and 64 rows per block: one row, the wave edge (15, 16, 17), the block edge
(64, 65) and a fifth block with one row (257).
"""
import functools
import random

import pytest
import torch

from cordum_amd.ops.reference import (
    WFL_DRAINING,
    WFL_FREE,
    WFL_LIVE,
    WFS_DISPATCHED,
    WFS_FAILED,
    WFS_PENDING,
    WFS_SUCCEEDED,
    wf_backoff_ref,
)

TICK = 41
TC = 3                                   # templates; row r runs template r % TC
POISON = -77
NOT_DISPATCHED = (0, 2, 3, 4, 5, 6)      # every step state but WFS_DISPATCHED
TIMEOUTS0, RETRIES0 = 1000, 2000         # the counters before the pass
SIZES = (1, 15, 16, 17, 64, 65, 257)
PATTERNS = ("none", "edge", "all", "free", "draining", "mixed", "bad_tmpl")
CASES = [(NR, p) for NR in SIZES for p in PATTERNS]
ARGS = ("step_state", "step_attempts", "children_todo", "children_out",
        "children_fail", "max_parallel", "next_ready", "dispatch_tick", "run_life",
        "run_tmpl", "tmpl_policy", "tmpl_timeout", "tick", "timeout_count",
        "retry_count")
STEP_COLS = ("step_attempts", "children_todo", "children_out", "children_fail",
             "max_parallel", "next_ready", "dispatch_tick")

# role -> (step, policy of template t as (max_retries, backoff, cap, mult_q8),
#          timeout of template t). The policy differs between templates where
# the role reads it, so neighbouring rows owe different results.
FAR = 1000                               # a timeout that is never due here


def _stock(t):
    return (2, 2, 16, 512)


ROLES = {
    # commit branches without failures
    "succeed": (0, _stock, lambda t: FAR),
    "resume": (1, _stock, lambda t: FAR),
    "slide": (2, _stock, lambda t: FAR),
    "slide_unlimited": (3, _stock, lambda t: FAR),
    "window_full": (4, _stock, lambda t: FAR),
    "in_flight": (5, _stock, lambda t: FAR),
    # retry / exhaustion
    "retry": (6, lambda t: (2, 2 + t, 16, 512), lambda t: FAR),
    "exhausted": (7, _stock, lambda t: FAR),
    "no_retry": (8, lambda t: (0, 2, 16, 512), lambda t: FAR),
    # timeouts: exactly due (into a retry), one tick early, due into FAILED
    "timeout_exact": (9, lambda t: (3, 3, 10, 384), lambda t: 12 + t),
    "timeout_minus1": (10, lambda t: (3, 3, 10, 384), lambda t: 12 + t),
    "timeout_fail": (11, lambda t: (1, 2, 16, 512), lambda t: 8),
    # the backoff formula: (3, x1.5, cap 10) gives 3, 5, 7, 10, 10
    "schedule_k3": (13, lambda t: (9, 3, 10, 384), lambda t: FAR),
    "cap": (31, lambda t: (9, 3, 10, 384), lambda t: FAR),
    "k_past_63": (32, lambda t: (32767, 100, 0, 257), lambda t: FAR),
    "saturate": (47, lambda t: (10, 1000, 0, 65535), lambda t: FAR),
    "retry_63": (63, lambda t: (2, 2, 16, 512), lambda t: FAR),
}
# what the formula gives for the roles above, worked out by hand:
# 100 * (257/256)^63 = 127.8 -> 128 (70 multiplications would give 132);
# 1000 * 255.996^2 is far past 2^20
BACKOFF = {"retry": lambda t: 2 + t, "timeout_exact": lambda t: 3, "schedule_k3": lambda t: 7,
           "cap": lambda t: 10, "k_past_63": lambda t: 128, "saturate": lambda t: 1 << 20,
           "retry_63": lambda t: 4}


def ref_ops():
    from cordum_amd.ops.pipeline import _RefOps

    return _RefOps()


def _run(ops, name, t, args, device):
    """One call of `ops.<name>` on clones of the tables in `t`; returns every
    table as a CPU tensor. `t` itself is never written."""
    d = {k: (v.clone().to(device) if torch.is_tensor(v) else v) for k, v in t.items()}
    getattr(ops, name)(*[d[a] for a in args])
    if str(device) != "cpu":
        torch.cuda.synchronize()
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in d.items()}


def settle_call(ops, t, device="cpu"):
    return _run(ops, "wf_settle", t, ARGS, device)


def build_tables(NR, pattern):
    rng = random.Random(500 * NR + PATTERNS.index(pattern))
    life = [WFL_LIVE] * NR
    tmpl = [r % TC for r in range(NR)]
    state = [[rng.choice(NOT_DISPATCHED) for _ in range(64)] for _ in range(NR)]
    cols = {k: [[POISON] * 64 for _ in range(NR)] for k in STEP_COLS}
    policy = [[(POISON,) * 4 for _ in range(64)] for _ in range(TC)]
    timeout = [[POISON] * 64 for _ in range(TC)]
    for role, (s, pol, tmo) in ROLES.items():
        for t in range(TC):
            policy[t][s], timeout[t][s] = pol(t), tmo(t)
    # what a correct pass leaves: (column, row, step) -> value
    want = {"cells": {}, "timeouts": 0, "retries": 0, "planted": {k: 0 for k in ROLES}}

    def put(r, s, **kv):
        for k, v in kv.items():
            cols[k][r][s] = v

    def owe(r, s, **kv):
        for k, v in kv.items():
            want["cells"][(k, r, s)] = v

    def retried(r, role, fail, att, todo):
        s, t = ROLES[role][0], tmpl[r]
        owe(r, s, step_state=WFS_PENDING, step_attempts=att + 1, children_fail=0,
            children_todo=todo + fail, next_ready=TICK + BACKOFF[role](t))
        want["retries"] += fail

    def plant(r, acted=True):
        """Every role once in row r. `acted` False: the row is one the pass
        must not touch, so nothing is owed."""
        t = tmpl[r] if 0 <= tmpl[r] < TC else 0
        for role, (s, pol, tmo) in ROLES.items():
            state[r][s] = WFS_DISPATCHED
            want["planted"][role] += int(acted)
            # cells a step's branch reads are real; the rest stays poison
            put(r, s, children_out=0, children_fail=0, children_todo=0)
        s = ROLES["resume"][0]
        put(r, s, children_todo=3)
        s = ROLES["slide"][0]
        put(r, s, children_out=2, children_todo=4, max_parallel=3, dispatch_tick=TICK - 1)
        s = ROLES["slide_unlimited"][0]
        put(r, s, children_out=2, children_todo=1, max_parallel=0, dispatch_tick=TICK - 1)
        s = ROLES["window_full"][0]
        put(r, s, children_out=3, children_todo=4, max_parallel=3, dispatch_tick=TICK - 1)
        s = ROLES["in_flight"][0]
        put(r, s, children_out=2, children_todo=0, dispatch_tick=TICK - 30)
        put(r, ROLES["retry"][0], children_fail=2, step_attempts=0, children_todo=1)
        put(r, ROLES["exhausted"][0], children_fail=1, step_attempts=2)
        put(r, ROLES["no_retry"][0], children_fail=1, step_attempts=0)
        put(r, ROLES["timeout_exact"][0], children_out=2, step_attempts=0,
            dispatch_tick=TICK - (12 + t))
        # past the stock cutoff of 8, one tick short of the step's own timeout
        put(r, ROLES["timeout_minus1"][0], children_out=2, max_parallel=0,
            dispatch_tick=TICK - (12 + t) + 1)
        put(r, ROLES["timeout_fail"][0], children_out=1, children_fail=1,
            step_attempts=1, dispatch_tick=TICK - 8)
        put(r, ROLES["schedule_k3"][0], children_fail=1, step_attempts=2)
        put(r, ROLES["cap"][0], children_fail=1, step_attempts=4)
        put(r, ROLES["k_past_63"][0], children_fail=1, step_attempts=70)
        put(r, ROLES["saturate"][0], children_fail=3, step_attempts=2)
        put(r, ROLES["retry_63"][0], children_fail=1, step_attempts=1, children_todo=5)
        if not acted:
            return
        owe(r, ROLES["succeed"][0], step_state=WFS_SUCCEEDED)
        owe(r, ROLES["resume"][0], step_state=WFS_PENDING)
        owe(r, ROLES["slide"][0], step_state=WFS_PENDING)
        owe(r, ROLES["slide_unlimited"][0], step_state=WFS_PENDING)
        retried(r, "retry", fail=2, att=0, todo=1)
        owe(r, ROLES["exhausted"][0], step_state=WFS_FAILED)
        owe(r, ROLES["no_retry"][0], step_state=WFS_FAILED)
        retried(r, "timeout_exact", fail=2, att=0, todo=0)
        owe(r, ROLES["timeout_exact"][0], children_out=0)
        want["timeouts"] += 2
        owe(r, ROLES["timeout_fail"][0], step_state=WFS_FAILED, children_out=0,
            children_fail=2)
        want["timeouts"] += 1
        retried(r, "schedule_k3", fail=1, att=2, todo=0)
        retried(r, "cap", fail=1, att=4, todo=0)
        retried(r, "k_past_63", fail=1, att=70, todo=0)
        retried(r, "saturate", fail=3, att=2, todo=0)
        retried(r, "retry_63", fail=1, att=1, todo=5)

    edge = sorted({0, NR // 2, NR - 1})
    if pattern == "edge":
        for r in edge:
            plant(r)
    elif pattern == "all":
        for r in range(NR):
            life[r] = WFL_LIVE if r % 3 else WFL_DRAINING
            plant(r)
    elif pattern == "free":
        for r in edge:
            life[r] = WFL_FREE
            plant(r, acted=False)
    elif pattern == "draining":
        for r in edge:
            life[r] = WFL_DRAINING
            plant(r)
    elif pattern == "mixed":
        for r in range(NR):
            kind = (r + 1) % 4                 # every kind from 4 rows on
            if kind == 0:
                life[r] = WFL_FREE
                plant(r, acted=False)
            elif kind == 1:
                plant(r)
            elif kind == 2:
                life[r] = WFL_DRAINING
                plant(r)
    elif pattern == "bad_tmpl":
        for k, r in enumerate(edge):
            tmpl[r] = (-1, TC, 1 << 30)[k % 3]
            plant(r, acted=False)
    t = {
        "step_state": torch.tensor(state, dtype=torch.uint8).flatten(),
        "run_life": torch.tensor(life, dtype=torch.uint8),
        "run_tmpl": torch.tensor(tmpl, dtype=torch.int32),
        "tmpl_policy": torch.tensor(policy, dtype=torch.int32).flatten(),
        "tmpl_timeout": torch.tensor(timeout, dtype=torch.int32).flatten(),
        "tick": torch.tensor([TICK], dtype=torch.int32),
        "timeout_count": torch.tensor([TIMEOUTS0], dtype=torch.int64),
        "retry_count": torch.tensor([RETRIES0], dtype=torch.int64),
        "want": want, "edge": edge,
    }
    for k in STEP_COLS:
        t[k] = torch.tensor(cols[k], dtype=torch.int32).flatten()
    return t


def expected_after(t):
    """The tables a correct pass leaves, from what the builder planted."""
    w = t["want"]
    out = {k: t[k].clone() for k in ARGS}
    for (k, r, s), v in w["cells"].items():
        out[k][r * 64 + s] = v
    out["timeout_count"][0] += w["timeouts"]
    out["retry_count"][0] += w["retries"]
    return out


def assert_exact(t, got):
    """Every table, owed cell and poison cell alike, and both counters."""
    want = expected_after(t)
    for k in ARGS:
        assert torch.equal(got[k], want[k]), k


def assert_case_is_the_case(t, NR, pattern):
    w, edge = t["want"], t["edge"]
    disp = (t["step_state"].view(NR, 64) == WFS_DISPATCHED)
    if pattern == "none":
        assert not bool(disp.any()) and not w["cells"]
    else:
        for r in edge if pattern != "mixed" else ():
            assert int(disp[r].sum()) == len(ROLES)
            assert bool(disp[r, 0]) and bool(disp[r, 63])       # step 0 and step 63
    if pattern in ("edge", "all", "draining"):
        assert all(n >= len(edge) for n in w["planted"].values())
        assert w["timeouts"] == 3 * w["planted"]["timeout_exact"] > 0
        assert w["retries"] > 0
        states = {v for (k, _, _), v in w["cells"].items() if k == "step_state"}
        assert states == {WFS_PENDING, WFS_SUCCEEDED, WFS_FAILED}
        # poison cells exist next to the owed ones, in the acted rows too
        r = edge[0]
        assert int(t["next_ready"][r * 64]) == POISON
        assert int(t["step_attempts"][r * 64 + 20]) == POISON
    if pattern == "all" and NR >= 17:
        # rows of different templates side by side in one wave owe different
        # delays and are due at different ticks
        s = ROLES["retry"][0]
        assert {w["cells"][("next_ready", r, s)] for r in (0, 1, 2)} == \
            {TICK + 2, TICK + 3, TICK + 4}
        assert len({int(t["dispatch_tick"][r * 64 + 9]) for r in (0, 1, 2)}) == 3
        assert {WFL_LIVE, WFL_DRAINING} == set(t["run_life"].tolist())
    if pattern == "draining":
        assert all(int(t["run_life"][r]) == WFL_DRAINING for r in edge)
    if pattern in ("free", "bad_tmpl"):
        assert not w["cells"] and w["timeouts"] == w["retries"] == 0
        assert bool(disp.any())
    if pattern == "free":
        assert all(int(t["run_life"][r]) == WFL_FREE for r in edge)
        # a FREE row with a DISPATCHED step whose children are overdue
        r = edge[0]
        i = r * 64 + ROLES["timeout_exact"][0]
        assert int(t["children_out"][i]) > 0 and int(t["dispatch_tick"][i]) <= TICK - 12
    if pattern == "bad_tmpl":
        assert all(not 0 <= int(t["run_tmpl"][r]) < TC for r in edge)
    if pattern == "mixed" and NR >= 15:
        assert {WFL_FREE, WFL_LIVE, WFL_DRAINING} == set(t["run_life"].tolist())
        assert w["cells"] and w["timeouts"] > 0


@functools.lru_cache(maxsize=None)
def settle_oracle(NR, pattern):
    """(tables, oracle output): computed once, shared, never written."""
    t = build_tables(NR, pattern)
    return t, settle_call(ref_ops(), t)


@pytest.mark.parametrize("NR,pattern", CASES)
def test_oracle_settle_on_a_hand_built_table(NR, pattern):
    t, out = settle_oracle(NR, pattern)
    assert_case_is_the_case(t, NR, pattern)
    assert_exact(t, out)


def test_the_hand_worked_delays_are_what_the_formula_gives():
    """The delays the builder owes are written down, not computed; this ties
    them to the formula, and the formula to the two schedules it was checked
    against: the stock 2, 4, 8, 16, 16 and (3, x1.5, cap 10) = 3, 5, 7, 10, 10."""
    assert [wf_backoff_ref(k, 2, 16, 512) for k in range(1, 8)] == [2, 4, 8, 16, 16, 16, 16]
    assert [wf_backoff_ref(k, 2, 16, 512) for k in range(1, 8)] == \
        [1 << min(k, 4) for k in range(1, 8)]
    assert [wf_backoff_ref(k, 3, 10, 384) for k in range(1, 6)] == [3, 5, 7, 10, 10]
    assert wf_backoff_ref(71, 100, 0, 257) == wf_backoff_ref(64, 100, 0, 257) == 128
    d = 100 << 16                        # 70 multiplications, were k - 1 not capped
    for _ in range(70):
        d = (d * 257) >> 8
    assert (d + 65535) >> 16 == 132
    assert wf_backoff_ref(3, 1000, 0, 65535) == 1 << 20
    assert wf_backoff_ref(2, 1000, 0, 65535) < 1 << 20
    assert wf_backoff_ref(10 ** 6, 1 << 20, 1 << 20, 65535) == 1 << 20
    for role, (s, pol, _) in ROLES.items():
        if role not in BACKOFF:
            continue
        att = {"retry": 0, "timeout_exact": 0, "schedule_k3": 2, "cap": 4,
               "k_past_63": 70, "saturate": 2, "retry_63": 1}[role]
        for t in range(TC):
            p = pol(t)
            assert wf_backoff_ref(att + 1, p[1], p[2], p[3]) == BACKOFF[role](t), role


# ---- equivalence with the stock pair -------------------------------------------
# On a table with no DISPATCHED step in a FREE row and every policy at the stock
# values (max_retries R, 2, x2, cap 16, timeout = cutoff), wf_settle computes
# what wf_timeout_scan followed by wf_commit computes, bit for bit.
CUTOFF = 8
EQUIV_R = (0, 2, 5)
EQUIV_CASES = [(NR, R) for NR in SIZES for R in EQUIV_R]
PAIR_TABLES = ("step_state", "step_attempts", "children_todo", "children_out",
               "children_done", "children_fail", "max_parallel", "next_ready",
               "dispatch_tick", "timeout_count", "retry_count")


@functools.lru_cache(maxsize=None)
def build_equiv_tables(NR, R):
    rng = random.Random(9000 + 10 * NR + R)
    life = [rng.choice((WFL_FREE, WFL_LIVE, WFL_LIVE, WFL_DRAINING)) for _ in range(NR)]
    state = [[rng.choice(NOT_DISPATCHED if life[r] == WFL_FREE or rng.random() < 0.5
                         else (WFS_DISPATCHED,)) for _ in range(64)] for r in range(NR)]
    n = NR * 64

    def col(lo, hi):
        return torch.tensor([rng.randint(lo, hi) for _ in range(n)], dtype=torch.int32)

    t = {
        "step_state": torch.tensor(state, dtype=torch.uint8).flatten(),
        "step_attempts": col(0, R + 1),
        "children_todo": col(0, 2),
        "children_out": torch.tensor([rng.choice((0, 0, 1, 3)) for _ in range(n)],
                                     dtype=torch.int32),
        "children_done": col(0, 5),
        "children_fail": col(0, 2),
        "max_parallel": torch.tensor([rng.choice((0, 2, 3)) for _ in range(n)],
                                     dtype=torch.int32),
        "next_ready": col(0, TICK),
        "dispatch_tick": col(TICK - CUTOFF - 2, TICK),
        "run_life": torch.tensor(life, dtype=torch.uint8),
        "run_tmpl": torch.tensor([r % TC for r in range(NR)], dtype=torch.int32),
        "tmpl_policy": torch.tensor([R, 2, 16, 512], dtype=torch.int32).repeat(TC * 64),
        "tmpl_timeout": torch.full((TC * 64,), CUTOFF, dtype=torch.int32),
        "tick": torch.tensor([TICK], dtype=torch.int32),
        "timeout_count": torch.tensor([TIMEOUTS0], dtype=torch.int64),
        "retry_count": torch.tensor([RETRIES0], dtype=torch.int64),
    }
    return t


def pair_call(ops, t, R, device="cpu"):
    """wf_timeout_scan then wf_commit, as the tick without step_policy runs
    them, on clones of the tables in `t`."""
    d = {k: (v.clone().to(device) if torch.is_tensor(v) else v) for k, v in t.items()}
    ops.wf_timeout_scan(d["step_state"], d["children_out"], d["children_fail"],
                        d["dispatch_tick"], d["tick"], CUTOFF, d["timeout_count"])
    ops.wf_commit(d["step_state"], d["step_attempts"], d["children_todo"],
                  d["children_out"], d["children_done"], d["children_fail"],
                  d["max_parallel"], d["next_ready"], d["tick"], R, d["retry_count"])
    if str(device) != "cpu":
        torch.cuda.synchronize()
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in d.items()}


def assert_equiv_case_is_the_case(t, pair, NR, R):
    """The random table reaches the branches the comparison is about."""
    if NR < 15:
        return
    assert int(pair["timeout_count"][0]) > TIMEOUTS0
    assert (int(pair["retry_count"][0]) > RETRIES0) == (R > 0)
    changed = pair["step_state"] != t["step_state"]
    assert {WFS_PENDING, WFS_SUCCEEDED, WFS_FAILED} == \
        set(pair["step_state"][changed].tolist())
    free = (t["run_life"] == WFL_FREE)[:, None].expand(NR, 64)
    assert not bool(((t["step_state"].view(NR, 64) == WFS_DISPATCHED) & free).any())


def assert_settle_equals_pair(settle, pair):
    for k in PAIR_TABLES:
        assert torch.equal(settle[k], pair[k]), k


@pytest.mark.parametrize("NR,R", EQUIV_CASES)
def test_oracle_settle_equals_the_stock_pair_at_stock_policies(NR, R):
    t = build_equiv_tables(NR, R)
    pair = pair_call(ref_ops(), t, R)
    assert_equiv_case_is_the_case(t, pair, NR, R)
    assert_settle_equals_pair(settle_call(ref_ops(), t), pair)
