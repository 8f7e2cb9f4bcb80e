"""The approval-hold kernels (wf_hold_scan, wf_hold_list, wf_decide) on
hand-built tables, oracle only: no GPU is needed here.

The table builders and the checks are module-level functions, and
tests/test_gpu_wf_holds.py imports them to run the HIP kernels on the same
cases. A builder records what it plants and what a correct pass owes for it,
so the expected tables are known without running the code under test.

Layout edges. The scan has 4 lanes per row, 16 rows per wave, 64 rows per
block: one row, the wave edge (15, 16, 17), the block edge (64, 65) and a
fifth block with one row (257). The list has one thread per row, 64 rows per
wave, 256 per block: the wave edge (63, 64, 65), the block edge (255, 256,
257) and a third block with one row (513). Decide has one thread per request.
"""
import functools
import random

import pytest
import torch

from cordum_amd.ops.reference import (
    WFK_APPROVAL,
    WFK_WORKER,
    WFL_DRAINING,
    WFL_FREE,
    WFL_LIVE,
    WFS_FAILED,
    WFS_PENDING,
    WFS_SUCCEEDED,
    WFS_WAITING,
)

TICK = 41
NOT_WAITING = (0, 1, 3, 4, 5, 6)         # every step state but WFS_WAITING


def ref_ops():
    from cordum_amd.ops.pipeline import _RefOps

    return _RefOps()


def _i64(m):
    return m - (1 << 64) if m >= (1 << 63) else m


def _run(ops, name, t, args, device):
    """One call of `ops.<name>` on clones of the tables in `t`; returns every
    table as a CPU tensor. `t` itself is never written."""
    d = {k: (v.clone().to(device) if torch.is_tensor(v) else v) for k, v in t.items()}
    getattr(ops, name)(*[d[a] for a in args])
    if str(device) != "cpu":
        torch.cuda.synchronize()
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in d.items()}


# ---- scan --------------------------------------------------------------------
SCAN_SIZES = (1, 15, 16, 17, 64, 65, 257)
SCAN_PATTERNS = ("none", "fresh", "continuing", "left", "step63", "beyond_nsteps",
                 "inactive_stale", "free_garbage", "regen", "ttl0", "ttl_minus1",
                 "ttl_due", "random")
SCAN_CASES = [(NR, p) for NR in SCAN_SIZES for p in SCAN_PATTERNS]
SCAN_ARGS = ("step_state", "n_steps", "run_life", "run_active", "run_gen", "tick",
             "hold_ttl", "hold_mask", "hold_tick", "hold_gen", "hold_counts",
             "hold_open")
SCAN_TABLES = ("step_state", "hold_mask", "hold_tick", "hold_gen", "hold_counts",
               "hold_open")
SCAN_INPUTS = ("n_steps", "run_life", "run_active", "run_gen", "tick", "hold_ttl")
COUNTS0 = (100, 200, 300, 400)
OPEN0 = 3          # the pass adds to hold_open; the pipeline zeroes it first


def build_scan_tables(NR, pattern):
    rng = random.Random(1000 * NR + SCAN_PATTERNS.index(pattern))
    life = [WFL_LIVE] * NR
    active = [1] * NR
    gen = [rng.randint(2, 49) for _ in range(NR)]
    hgen = list(gen)
    ns = [rng.randint(1, 64) for _ in range(NR)]
    state = [[rng.choice(NOT_WAITING) for _ in range(64)] for _ in range(NR)]
    mask = [0] * NR
    htick = [[rng.randint(-5, 30) for _ in range(64)] for _ in range(NR)]  # garbage
    ttl = [[rng.randint(0, 5) for _ in range(64)] for _ in range(NR)]
    # what a correct pass leaves: filled in by the planting functions
    want = {"mask": None, "tick": {}, "failed": set(), "gen": {},
            "opened": 0, "expired": 0}
    wmask = [0] * NR
    roles = {}

    def fresh(r, s):
        ns[r] = max(ns[r], s + 1)
        state[r][s] = WFS_WAITING
        mask[r] &= ~(1 << s)
        wmask[r] |= 1 << s
        want["tick"][(r, s)] = TICK
        want["opened"] += 1

    def cont(r, s, age, t):
        """An open hold of `age` ticks with ttl `t`."""
        ns[r] = max(ns[r], s + 1)
        state[r][s] = WFS_WAITING
        mask[r] |= 1 << s
        htick[r][s] = TICK - age
        ttl[r][s] = t
        if t > 0 and age >= t:
            want["failed"].add((r, s))
            want["expired"] += 1
        else:
            wmask[r] |= 1 << s

    def left(r, s):
        """The step was decided (or cancelled) since the hold opened."""
        ns[r] = max(ns[r], s + 1)
        state[r][s] = rng.choice((WFS_SUCCEEDED, WFS_FAILED))
        mask[r] |= 1 << s

    def beyond(r):
        """WAITING bytes at s >= n_steps are no steps."""
        ns[r] = rng.randint(1, 63)
        for s in range(ns[r], 64):
            state[r][s] = WFS_WAITING

    def inactive(r, how):
        """Not LIVE-and-active, a WAITING step and a valid stale mask."""
        if how == 0:
            active[r] = 0
        else:
            life[r] = WFL_DRAINING
            active[r] = 0
        ns[r] = 64
        state[r][3] = WFS_WAITING
        mask[r] = (1 << 3) | (1 << 40)
        wmask[r] = 0

    def free(r):
        life[r] = WFL_FREE
        active[r] = rng.randint(0, 1)
        state[r] = [WFS_WAITING] * 64
        mask[r] = rng.getrandbits(64) | 1
        hgen[r] = rng.choice((gen[r], gen[r] - 1))
        wmask[r] = mask[r]                 # untouched

    def regen(r):
        """Re-admitted since its hold words were written: the mask and ticks
        of the generation before, one of its bits on a step that is WAITING
        again. The stale tick is old enough to expire under the row's ttl."""
        hgen[r] = gen[r] - 1
        ns[r] = 64
        state[r] = [rng.choice(NOT_WAITING) for _ in range(64)]
        mask[r] = (1 << 2) | (1 << 17) | (1 << 63)
        wmask[r] = 0
        for s in (2, 17, 63):
            htick[r][s] = TICK - 30
            ttl[r][s] = 4
        for s in (17, 20):
            state[r][s] = WFS_WAITING
            wmask[r] |= 1 << s
            want["tick"][(r, s)] = TICK
            want["opened"] += 1
        want["gen"][r] = gen[r]

    edge = sorted({0, NR // 2, NR - 1})
    if pattern == "fresh":
        for r in edge:
            fresh(r, (7 * r + 1) % 64)
    elif pattern == "continuing":
        for r in edge:
            cont(r, (5 * r + 16) % 64, age=9, t=0)
            cont(r, (5 * r + 33) % 64, age=2, t=50)
    elif pattern == "left":
        for r in edge:
            left(r, 0)
            left(r, 31)
            cont(r, 32, age=1, t=0)
    elif pattern == "step63":
        fresh(NR - 1, 63)
        cont(0, 63, age=3, t=0) if NR > 1 else None
    elif pattern == "beyond_nsteps":
        for r in edge:
            beyond(r)
    elif pattern == "inactive_stale":
        for k, r in enumerate(edge):
            inactive(r, k % 2)
    elif pattern == "free_garbage":
        for r in edge:
            free(r)
    elif pattern == "regen":
        for r in edge:
            regen(r)
    elif pattern == "ttl0":
        for r in edge:
            cont(r, 15, age=10 ** 6, t=0)
    elif pattern == "ttl_minus1":
        for r in edge:
            cont(r, 16, age=6, t=7)
    elif pattern == "ttl_due":
        for r in edge:
            cont(r, 47, age=7, t=7)
            cont(r, 48, age=1, t=1)
    elif pattern == "random":
        for r in range(NR):
            kind = (r + 3) % 8                 # every kind from 8 rows on
            if kind == 0:
                free(r)
            elif kind == 1:
                inactive(r, r % 2)
            elif kind == 2:
                regen(r)
            elif kind == 3:
                beyond(r)
            elif kind >= 5:
                for s in rng.sample(range(64), rng.randint(1, 12)):
                    what = rng.randrange(3)
                    if what == 0:
                        fresh(r, s)
                    elif what == 1:
                        cont(r, s, age=rng.randint(0, 6), t=rng.randint(0, 6))
                    else:
                        left(r, s)
    roles["edge"] = edge
    want["mask"] = wmask
    return {
        "step_state": torch.tensor(state, dtype=torch.uint8).flatten(),
        "n_steps": torch.tensor(ns, dtype=torch.uint8),
        "run_life": torch.tensor(life, dtype=torch.uint8),
        "run_active": torch.tensor(active, dtype=torch.uint8),
        "run_gen": torch.tensor(gen, dtype=torch.int32),
        "tick": torch.tensor([TICK], dtype=torch.int32),
        "hold_ttl": torch.tensor(ttl, dtype=torch.int32).flatten(),
        "hold_mask": torch.tensor([_i64(m) for m in mask], dtype=torch.int64),
        "hold_tick": torch.tensor(htick, dtype=torch.int32).flatten(),
        "hold_gen": torch.tensor(hgen, dtype=torch.int32),
        "hold_counts": torch.tensor(COUNTS0, dtype=torch.int64),
        "hold_open": torch.tensor([OPEN0], dtype=torch.int32),
        "want": want, "roles": roles,
    }


def scan_call(ops, t, device="cpu"):
    return _run(ops, "wf_hold_scan", t, SCAN_ARGS, device)


def expected_after_scan(t):
    """The tables a correct pass leaves, from what the builder planted."""
    w = t["want"]
    NR = int(t["run_life"].shape[0])
    state = t["step_state"].clone()
    for r, s in w["failed"]:
        state[r * 64 + s] = WFS_FAILED
    tick = t["hold_tick"].clone()
    for (r, s), v in w["tick"].items():
        tick[r * 64 + s] = v
    hgen = t["hold_gen"].clone()
    for r, g in w["gen"].items():
        hgen[r] = g
    live = [r for r in range(NR) if int(t["run_life"][r]) == WFL_LIVE
            and int(t["run_active"][r]) == 1]
    n_open = sum(bin(w["mask"][r]).count("1") for r in live)
    counts = torch.tensor(COUNTS0, dtype=torch.int64)
    counts[0] += w["opened"]
    counts[1] += w["expired"]
    return {
        "step_state": state, "hold_tick": tick, "hold_gen": hgen,
        "hold_mask": torch.tensor([_i64(m) for m in w["mask"]], dtype=torch.int64),
        "hold_counts": counts,
        "hold_open": torch.tensor([OPEN0 + n_open], dtype=torch.int32),
    }


def assert_scan_is_exact(t, out):
    want = expected_after_scan(t)
    for k in SCAN_TABLES:
        assert torch.equal(out[k], want[k]), k
    for k in SCAN_INPUTS:
        assert torch.equal(out[k], t[k]), k


def assert_second_scan_only_expires(ops, t, out, device="cpu"):
    """A second pass one tick later on the first pass's output changes
    nothing, except that holds whose ttl has come due by then expire."""
    u = dict(t)
    u.update({k: out[k] for k in SCAN_TABLES})
    u["tick"] = torch.tensor([TICK + 1], dtype=torch.int32)
    out2 = scan_call(ops, u, device)
    NR = int(t["run_life"].shape[0])
    state, mask = out["step_state"].clone(), out["hold_mask"].clone()
    counts, n_open = out["hold_counts"].clone(), 0
    for r in range(NR):
        if int(t["run_life"][r]) != WFL_LIVE or int(t["run_active"][r]) != 1:
            continue
        m = int(mask[r]) & ((1 << 64) - 1)
        for s in range(64):
            if not (m >> s) & 1:
                continue
            i = r * 64 + s
            ttl = int(t["hold_ttl"][i])
            if ttl > 0 and TICK + 1 - int(out["hold_tick"][i]) >= ttl:
                state[i] = WFS_FAILED
                m &= ~(1 << s)
                counts[1] += 1
        mask[r] = _i64(m)
        n_open += bin(m).count("1")
    assert torch.equal(out2["step_state"], state)
    assert torch.equal(out2["hold_mask"], mask)
    assert torch.equal(out2["hold_counts"], counts)
    assert torch.equal(out2["hold_tick"], out["hold_tick"])
    assert torch.equal(out2["hold_gen"], out["hold_gen"])
    assert int(out2["hold_open"][0]) == int(out["hold_open"][0]) + n_open
    return int(counts[1]) - int(out["hold_counts"][1])


@functools.lru_cache(maxsize=None)
def scan_oracle(NR, pattern):
    """(tables, oracle output): computed once, shared, never written."""
    t = build_scan_tables(NR, pattern)
    return t, scan_call(ref_ops(), t)


def assert_scan_case_is_the_case(t, NR, pattern):
    w, edge = t["want"], t["roles"]["edge"]
    state = t["step_state"].view(NR, 64)
    waiting = state == WFS_WAITING
    if pattern == "none":
        assert not bool(waiting.any()) and not bool(t["hold_mask"].any())
        assert w["opened"] == w["expired"] == 0 and not any(w["mask"])
    if pattern == "fresh":
        assert w["opened"] == len(edge) and not bool(t["hold_mask"].any())
    if pattern == "continuing":
        assert w["opened"] == w["expired"] == 0
        assert [int(m) for m in t["hold_mask"]] == [_i64(m) for m in w["mask"]]
        assert bool(t["hold_mask"].any())
    if pattern == "left":
        for r in edge:
            assert int(t["hold_mask"][r]) & 1 and not w["mask"][r] & 1
            assert w["mask"][r] == 1 << 32
    if pattern == "step63":
        assert w["mask"][NR - 1] >> 63 == 1
    if pattern == "beyond_nsteps":
        for r in edge:
            assert bool(waiting[r, int(t["n_steps"][r]):].all()) and w["mask"][r] == 0
        assert w["opened"] == 0
    if pattern == "inactive_stale":
        for r in edge:
            assert int(t["run_active"][r]) == 0 and int(t["hold_mask"][r]) != 0
            assert int(t["hold_gen"][r]) == int(t["run_gen"][r]) and w["mask"][r] == 0
        assert {int(t["run_life"][r]) for r in edge} <= {WFL_LIVE, WFL_DRAINING}
    if pattern == "free_garbage":
        for r in edge:
            assert int(t["run_life"][r]) == WFL_FREE and bool(waiting[r].all())
            assert int(t["hold_mask"][r]) != 0
    if pattern == "regen":
        for r in edge:
            assert int(t["hold_gen"][r]) == int(t["run_gen"][r]) - 1
            assert (int(t["hold_mask"][r]) >> 17) & 1 and bool(waiting[r, 17])
            assert w["mask"][r] == (1 << 17) | (1 << 20)
        assert w["opened"] == 2 * len(edge) and w["expired"] == 0
    if pattern in ("ttl0", "ttl_minus1"):
        assert w["expired"] == 0 and all(w["mask"][r] for r in edge)
    if pattern == "ttl_due":
        assert w["expired"] == 2 * len(edge) and not any(w["mask"])
    if pattern == "random" and NR >= 15:
        assert w["opened"] > 0 and w["expired"] > 0 and w["gen"]
        assert {WFL_FREE, WFL_LIVE} <= set(t["run_life"].tolist())


@pytest.mark.parametrize("NR,pattern", SCAN_CASES)
def test_oracle_scan_on_a_hand_built_table(NR, pattern):
    t, out = scan_oracle(NR, pattern)
    assert_scan_case_is_the_case(t, NR, pattern)
    assert_scan_is_exact(t, out)
    due = assert_second_scan_only_expires(ref_ops(), t, out)
    if pattern == "ttl_minus1":
        assert due == len(t["roles"]["edge"])      # one tick later they are due
    if pattern in ("none", "ttl0", "continuing"):
        assert due == 0


# ---- list --------------------------------------------------------------------
LIST_SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
LIST_CAPS = ("ample", "exact", "minus1", "one")
LIST_CURSORS = ("zero", "mid_row", "past_end")
LIST_CASES = [(NR, c, cur) for NR in LIST_SIZES for c in LIST_CAPS
              for cur in LIST_CURSORS]
LIST_ARGS = ("step_state", "run_life", "run_active", "run_gen", "hold_mask",
             "hold_tick", "hold_gen", "cursor", "list_mask", "blk_scan", "list")
LIST_INPUTS = LIST_ARGS[:7]
POISON = -7


def build_list_tables(NR, cap_mode="ample", cursor_mode="zero"):
    rng = random.Random(7000 + NR)
    life = [WFL_LIVE] * NR
    active = [1] * NR
    gen = [rng.randint(2, 49) for _ in range(NR)]
    hgen = list(gen)
    state = [[rng.choice(NOT_WAITING) for _ in range(64)] for _ in range(NR)]
    mask = [0] * NR
    htick = [[rng.randint(0, 40) for _ in range(64)] for _ in range(NR)]
    planted = []                       # (slot, gen, step, hold_tick), ascending

    def holds(r, steps, listable=True):
        for s in steps:
            state[r][s] = WFS_WAITING
            mask[r] |= 1 << s
            if listable:
                planted.append((r, gen[r], s, htick[r][s]))

    for r in range(NR):
        kind = r % 7 if NR > 1 else 0
        if kind == 0:                  # the row edges and both sides of a mid cursor
            holds(r, [0, 5, 30, 63])
        elif kind == 1:                # decided since: bit set, state moved on
            holds(r, [9])
            mask[r] |= 1 << 10
            state[r][10] = WFS_SUCCEEDED
        elif kind == 2:                # another generation's words
            holds(r, [1, 2], listable=False)
            hgen[r] = gen[r] - 1
        elif kind == 3:                # cancelled / finished
            holds(r, [3], listable=False)
            active[r] = 0
        elif kind == 4:                # FREE or DRAINING
            holds(r, [4, 63], listable=False)
            life[r] = WFL_FREE if r % 2 else WFL_DRAINING
        elif kind == 5:                # WAITING but no hold bit yet
            state[r][6] = WFS_WAITING
        else:
            holds(r, sorted(rng.sample(range(64), rng.randint(1, 20))))
    planted.sort()
    mid_row = (NR // 2) // 7 * 7       # a row of kind 0 near the middle
    cursor = {"zero": 0, "mid_row": mid_row * 64 + 30, "past_end": NR * 64}[cursor_mode]
    expect = [p for p in planted if p[0] * 64 + p[2] >= cursor]
    total = len(expect)
    cap = {"ample": total + 5, "exact": max(1, total), "minus1": max(1, total - 1),
           "one": 1}[cap_mode]
    nblk = (NR + 255) // 256
    return {
        "step_state": torch.tensor(state, dtype=torch.uint8).flatten(),
        "run_life": torch.tensor(life, dtype=torch.uint8),
        "run_active": torch.tensor(active, dtype=torch.uint8),
        "run_gen": torch.tensor(gen, dtype=torch.int32),
        "hold_mask": torch.tensor([_i64(m) for m in mask], dtype=torch.int64),
        "hold_tick": torch.tensor(htick, dtype=torch.int32).flatten(),
        "hold_gen": torch.tensor(hgen, dtype=torch.int32),
        "cursor": cursor,
        "list_mask": torch.zeros(NR, dtype=torch.int64),
        "blk_scan": torch.zeros(nblk + 1, dtype=torch.int32),
        "list": torch.full((4 + 4 * cap,), POISON, dtype=torch.int32),
        "planted": planted, "expect": expect, "cap": cap,
    }


def list_call(ops, t, device="cpu"):
    return _run(ops, "wf_hold_list", t, LIST_ARGS, device)


def assert_list_is_exact(t, out):
    expect, cap = t["expect"], t["cap"]
    assert int(out["list"][0]) == len(expect)
    assert out["list"][1:4].tolist() == [POISON] * 3          # the pad is left alone
    m = min(len(expect), cap)
    rec = out["list"][4:].view(-1, 4)
    assert [tuple(x) for x in rec[:m].tolist()] == expect[:m]  # in order, no sorting
    assert bool((rec[m:] == POISON).all())
    for k in LIST_INPUTS:
        assert torch.equal(out[k], t[k]), k


def page_all(ops, t, cap, device="cpu"):
    """Every hold of `t` in pages of `cap`, as the pipeline pages."""
    got, cursor, pages = [], 0, 0
    while True:
        u = dict(t)
        u["cursor"] = cursor
        u["list"] = torch.full((4 + 4 * cap,), POISON, dtype=torch.int32)
        out = list_call(ops, u, device)
        n = int(out["list"][0])
        m = min(n, cap)
        got += [tuple(x) for x in out["list"][4:].view(-1, 4)[:m].tolist()]
        pages += 1
        if n <= cap:
            return got, pages
        cursor = got[-1][0] * 64 + got[-1][2] + 1


@functools.lru_cache(maxsize=None)
def list_oracle(NR, cap_mode, cursor_mode):
    t = build_list_tables(NR, cap_mode, cursor_mode)
    return t, list_call(ref_ops(), t)


@pytest.mark.parametrize("NR,cap_mode,cursor_mode", LIST_CASES)
def test_oracle_list_on_a_hand_built_table(NR, cap_mode, cursor_mode):
    t, out = list_oracle(NR, cap_mode, cursor_mode)
    planted, expect = t["planted"], t["expect"]
    assert planted == sorted(planted) and len(planted) >= 4
    if cursor_mode == "zero":
        assert expect == planted
    if cursor_mode == "mid_row":       # the cursor splits a row that has holds
        row = t["cursor"] // 64
        assert [p[2] for p in planted if p[0] == row][:3] == [0, 5, 30]
        assert 0 < len(expect) < len(planted) and expect[0][:3:2] == (row, 30)
    if cursor_mode == "past_end":
        assert expect == []
    assert_list_is_exact(t, out)


@pytest.mark.parametrize("NR", LIST_SIZES)
def test_oracle_pages_reassemble_to_the_planted_set(NR):
    t = build_list_tables(NR)
    for cap in (1, 7) if NR <= 65 else (64,):
        got, pages = page_all(ref_ops(), t, cap)
        assert got == t["planted"]
        assert pages == max(1, -(-len(got) // cap))


# ---- decide ------------------------------------------------------------------
DECIDE_COUNTS = (1, 63, 64, 65, 257)
DECIDE_ARGS = ("req_slot", "req_gen", "req_step", "req_verdict", "run_life",
               "run_gen", "run_active", "n_steps", "step_kind", "step_state",
               "hold_counts", "out_code")
# role -> the code it owes
ROLES = (("approve", 0), ("reject", 0), ("stale_gen", 1), ("free", 1),
         ("draining", 1), ("slot_low", 1), ("slot_high", 1), ("inactive", 2),
         ("not_approval", 3), ("not_waiting", 3), ("step_past_n", 3),
         ("step_negative", 3), ("step_64", 3))


def build_decide_tables(n, two_steps=False):
    """Request i names row i in role i % len(ROLES); with `two_steps` a last
    request names a second waiting approval of row 0."""
    rng = random.Random(300 + n)
    NR = n
    life = [WFL_LIVE] * NR
    active = [1] * NR
    gen = [rng.randint(2, 49) for _ in range(NR)]
    ns = [8] * NR
    kind = [[WFK_APPROVAL if s % 2 else WFK_WORKER for s in range(64)] for _ in range(NR)]
    state = [[WFS_WAITING if s in (1, 3) else WFS_PENDING for s in range(64)]
             for _ in range(NR)]
    req, codes, writes, approved, rejected = [], [], {}, 0, 0
    for i in range(n):
        role, code = ROLES[i % len(ROLES)]
        slot, g, step, verdict = i, gen[i], 1, i % 3 != 0
        if role == "approve":
            verdict = 1
        elif role == "reject":
            verdict = 0
        elif role == "stale_gen":
            g -= 1
        elif role == "free":
            life[i] = WFL_FREE
        elif role == "draining":
            life[i], active[i] = WFL_DRAINING, 0
        elif role == "slot_low":
            slot = -1
        elif role == "slot_high":
            slot = NR
        elif role == "inactive":
            active[i] = 0
        elif role == "not_approval":
            step = 2
            state[i][2] = WFS_WAITING          # WAITING, but a worker step
        elif role == "not_waiting":
            step = 5
        elif role == "step_past_n":
            step = 9
            state[i][9] = WFS_WAITING          # an approval byte past n_steps
        elif role == "step_negative":
            step = -1
        elif role == "step_64":
            step = 64
        req.append((slot, g, step, int(verdict)))
        codes.append(code)
        if code == 0:
            writes[(slot, step)] = WFS_SUCCEEDED if verdict else WFS_FAILED
            approved += int(verdict)
            rejected += int(not verdict)
    if two_steps:
        req.append((0, gen[0], 3, 0))
        codes.append(0)
        writes[(0, 3)] = WFS_FAILED
        rejected += 1
    cols = list(zip(*req))
    return {
        "req_slot": torch.tensor(cols[0], dtype=torch.int32),
        "req_gen": torch.tensor(cols[1], dtype=torch.int32),
        "req_step": torch.tensor(cols[2], dtype=torch.int32),
        "req_verdict": torch.tensor(cols[3], dtype=torch.int32),
        "run_life": torch.tensor(life, dtype=torch.uint8),
        "run_gen": torch.tensor(gen, dtype=torch.int32),
        "run_active": torch.tensor(active, dtype=torch.uint8),
        "n_steps": torch.tensor(ns, dtype=torch.uint8),
        "step_kind": torch.tensor(kind, dtype=torch.uint8).flatten(),
        "step_state": torch.tensor(state, dtype=torch.uint8).flatten(),
        "hold_counts": torch.tensor(COUNTS0, dtype=torch.int64),
        "out_code": torch.full((len(req),), 99, dtype=torch.uint8),
        "codes": codes, "writes": writes, "approved": approved, "rejected": rejected,
    }


def decide_call(ops, t, device="cpu"):
    return _run(ops, "wf_decide", t, DECIDE_ARGS, device)


def assert_decide_is_exact(t, out):
    assert out["out_code"].tolist() == t["codes"]
    state = t["step_state"].clone()
    for (slot, step), v in t["writes"].items():
        state[slot * 64 + step] = v
    assert torch.equal(out["step_state"], state)       # one byte per applied request
    c = list(COUNTS0)
    c[2] += t["approved"]
    c[3] += t["rejected"]
    assert out["hold_counts"].tolist() == c
    for k in DECIDE_ARGS[:9]:
        assert torch.equal(out[k], t[k]), k


@functools.lru_cache(maxsize=None)
def decide_oracle(n, two_steps=False):
    t = build_decide_tables(n, two_steps)
    return t, decide_call(ref_ops(), t)


@pytest.mark.parametrize("n", DECIDE_COUNTS)
def test_oracle_decide_on_a_hand_built_table(n):
    t, out = decide_oracle(n)
    if n >= len(ROLES):
        assert set(t["codes"]) == {0, 1, 2, 3}
    assert_decide_is_exact(t, out)


def test_oracle_decide_every_role_and_two_steps_of_one_run():
    t, out = decide_oracle(len(ROLES), True)
    assert [r[1] for r in ROLES] + [0] == t["codes"]
    assert t["writes"][(0, 1)] == WFS_SUCCEEDED and t["writes"][(0, 3)] == WFS_FAILED
    assert (t["approved"], t["rejected"]) == (1, 2)
    assert_decide_is_exact(t, out)
