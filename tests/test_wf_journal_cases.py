"""The step-transition journal pass (wf_journal) on hand-built tables, oracle
only: no GPU is needed here.

The table builders and the checks are module-level functions, and
tests/test_gpu_wf_journal.py imports them to run the HIP kernel on the same
cases. A builder records every change it plants, so the expected events are
known without running the code under test; each case asserts that it is the
case it names.

Layout edges of the kernel: 4 lanes per row, 16 rows per wave, 64 rows per
block, so the table sizes are one row, the wave edge (15, 16, 17), the block
edge (64, 65) and a fifth block with one row (257).
"""
import functools
import random

import pytest
import torch

from cordum_amd.ops.reference import WFL_DRAINING, WFL_FREE, WFL_LIVE, WFS_PENDING

SIZES = (1, 15, 16, 17, 64, 65, 257)
PATTERNS = ("none", "last_step", "one_row_all", "all", "regen", "free_differs",
            "draining", "random")
# cap / preload of the event list, relative to the number of planted changes
CAP_MODES = ("ample", "ample_preload", "exact", "minus1", "one", "preload_cap",
             "preload_above")
OVERFLOW_PATTERNS = ("all", "regen", "random")   # every one plants >= 2 changes
CASES = ([(NR, p, "ample") for NR in SIZES for p in PATTERNS]
         + [(NR, p, m) for NR in SIZES for p in OVERFLOW_PATTERNS
            for m in CAP_MODES[1:]])
ARGS = ("step_state", "run_life", "run_gen", "tick", "phase", "ev_shadow_state",
        "ev_shadow_gen", "ev_rec", "ev_count")
TICK, PHASE = 41, 1
STAMP = 2 * TICK + PHASE
POISON = -7
N_STATES = 7                # WFS_PENDING .. WFS_CANCELLED


def ref_ops():
    from cordum_amd.ops.pipeline import _RefOps

    return _RefOps()


def call(ops, t, device="cpu"):
    """One journal pass of `ops` on clones of the tables in `t`; returns every
    table as a CPU tensor. `t` itself is never written."""
    d = {k: (v.clone().to(device) if torch.is_tensor(v) else v) for k, v in t.items()}
    ops.wf_journal(*[d[a] for a in ARGS])
    if str(device) != "cpu":
        torch.cuda.synchronize()
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in d.items()}


def build_journal_tables(NR, pattern, cap_mode):
    rng = random.Random(
        1000 * NR + 10 * PATTERNS.index(pattern) + CAP_MODES.index(cap_mode))
    # plain lists while the case is planted; tensors at the end
    life = [WFL_LIVE] * NR
    gen = [rng.randint(1, 49) for _ in range(NR)]
    sgen = list(gen)
    shadow = [[rng.randrange(N_STATES) for _ in range(64)] for _ in range(NR)]
    state = [list(row) for row in shadow]
    changes = {}            # (row, step) -> (from, to): the events one pass owes

    def change(r, s):
        old = shadow[r][s]
        new = (old + 1 + rng.randrange(N_STATES - 1)) % N_STATES
        state[r][s] = new
        changes[(r, s)] = (old, new)

    def regen(r, steps):
        """Row r was re-admitted: stale non-zero shadow of the generation
        before, a fresh row with `steps` already past PENDING."""
        shadow[r] = [rng.randrange(1, N_STATES) for _ in range(64)]
        sgen[r] = gen[r] - 1
        state[r] = [WFS_PENDING] * 64
        for s in steps:
            new = rng.randrange(1, N_STATES)
            state[r][s] = new
            changes[(r, s)] = (WFS_PENDING, new)

    def free(r):
        """A FREE row whose shadow differs everywhere, generation included."""
        life[r] = WFL_FREE
        state[r] = [(v + 1) % N_STATES for v in shadow[r]]
        sgen[r] = gen[r] - 1

    roles = {}
    if pattern == "last_step":
        change(NR - 1, 63)
    elif pattern == "one_row_all":
        roles["row"] = NR // 2
        for s in range(64):
            change(NR // 2, s)
    elif pattern == "all":
        for r in range(NR):
            for s in range(64):
                change(r, s)
    elif pattern == "regen":
        rows = sorted({0, NR // 2, NR - 1})
        roles["regen"] = rows
        for r in rows:
            regen(r, [0, 15, 16, 63])
        for r in range(NR):
            if r not in rows and r % 3 == 0:
                change(r, (5 * r) % 64)
    elif pattern == "free_differs":
        rows = sorted({0, NR - 1, NR // 2})
        roles["free"] = rows
        for r in rows:
            free(r)
        for r in range(NR):
            if r not in rows:
                change(r, r % 64)
    elif pattern == "draining":
        rows = sorted({0, NR - 1})
        roles["draining"] = rows
        for r in rows:
            life[r] = WFL_DRAINING
            change(r, 0)
            change(r, 63)
    elif pattern == "random":
        for r in range(NR):
            kind = (r + 2) % 10     # row 0 re-admitted; every kind from 10 rows on
            if kind == 0:
                free(r)
                continue
            if kind == 1:
                life[r] = WFL_DRAINING
            if kind in (2, 3):
                regen(r, [s for s in range(64) if rng.randrange(4) == 0] or [7])
                continue
            for s in range(64):
                if rng.randrange(8) == 0:
                    change(r, s)
        if len(changes) < 2:
            change(NR - 1, 1) if kind not in (0, 2, 3) else None

    state = torch.tensor(state, dtype=torch.uint8)
    shadow = torch.tensor(shadow, dtype=torch.uint8)
    life = torch.tensor(life, dtype=torch.uint8)
    gen = torch.tensor(gen, dtype=torch.int32)
    sgen = torch.tensor(sgen, dtype=torch.int32)
    total = len(changes)
    cap, preload = {
        "ample": (total + 5, 0),
        "ample_preload": (total + 3, 3),
        "exact": (max(1, total), 0),
        "minus1": (max(1, total - 1), 0),
        "one": (1, 0),
        "preload_cap": (max(1, total // 2), max(1, total // 2)),
        "preload_above": (max(1, total // 2), max(1, total // 2) + 3),
    }[cap_mode]
    return {
        "step_state": state.flatten(), "run_life": life, "run_gen": gen,
        "tick": torch.tensor([TICK], dtype=torch.int32), "phase": PHASE,
        "ev_shadow_state": shadow.flatten(), "ev_shadow_gen": sgen,
        "ev_rec": torch.full((cap * 4,), POISON, dtype=torch.int32),
        "ev_count": torch.tensor([preload], dtype=torch.int32),
        "changes": changes, "roles": roles, "cap": cap, "preload": preload,
    }


def expected_emitted(t):
    return min(len(t["changes"]), max(0, t["cap"] - t["preload"]))


def emitted_records(t, out):
    """The records a pass on `t` appended, as [(slot, gen, step, from, to,
    stamp)] in list order: positions preload .. min(count, cap)."""
    lo = min(t["preload"], t["cap"])
    hi = max(lo, min(int(out["ev_count"][0]), t["cap"]))
    rec = out["ev_rec"].view(-1, 4)[lo:hi].tolist()
    return [(a, b, c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFF, d) for a, b, c, d in rec]


def assert_pass_is_sound(t, out, stamp=STAMP):
    """What holds for any correct pass, whichever changes a full list let in:
    the right number of events, each a planted change reported once with its
    generation and stamp; the shadow advanced exactly for those; FREE rows,
    the list outside the appended range and the inputs untouched."""
    NR, cap, preload, changes = int(t["run_life"].shape[0]), t["cap"], t["preload"], t["changes"]
    recs = emitted_records(t, out)
    assert len(recs) == expected_emitted(t)
    count = int(out["ev_count"][0])
    if preload >= cap:
        assert count == preload                       # nothing is ever added
    elif len(changes) <= cap - preload:
        assert count == preload + len(changes)        # no overflow: exact
    else:
        assert cap <= count <= cap - 1 + 64 * NR      # the kernel's bound
    seen = set()
    gens = t["run_gen"].tolist()
    for slot, gen, step, frm, to, st in recs:
        assert (slot, step) in changes and (slot, step) not in seen
        seen.add((slot, step))
        assert (frm, to) == changes[(slot, step)]
        assert gen == gens[slot] and st == stamp
    # the list below the preload and past the appended records is untouched
    rec = out["ev_rec"].view(-1, 4)
    lo = min(preload, cap)
    assert bool((rec[:lo] == POISON).all()) and bool((rec[lo + len(recs):] == POISON).all())
    # shadow: FREE rows untouched; other rows hold the old effective shadow
    # (PENDING after a generation change), advanced for the emitted events
    live = t["run_life"] != WFL_FREE
    regen = live & (t["run_gen"] != t["ev_shadow_gen"])
    want = t["ev_shadow_state"].view(NR, 64).clone()
    want[regen] = WFS_PENDING
    if seen:
        idx = torch.tensor(sorted(seen))
        want[idx[:, 0], idx[:, 1]] = t["step_state"].view(NR, 64)[idx[:, 0], idx[:, 1]]
    assert torch.equal(out["ev_shadow_state"].view(NR, 64), want)
    assert torch.equal(out["ev_shadow_gen"][live], t["run_gen"][live])
    assert torch.equal(out["ev_shadow_gen"][~live], t["ev_shadow_gen"][~live])
    for k in ("step_state", "run_life", "run_gen", "tick"):
        assert torch.equal(out[k], t[k]), k
    return seen


def second_pass_tables(t, out):
    """The tables after the pass `out`, with an emptied list large enough for
    every change that is left."""
    first = {(r[0], r[2]) for r in emitted_records(t, out)}
    left = {k: v for k, v in t["changes"].items() if k not in first}
    u = dict(t)
    u.update(ev_shadow_state=out["ev_shadow_state"], ev_shadow_gen=out["ev_shadow_gen"],
             ev_rec=torch.full((4 * (len(left) + 5),), POISON, dtype=torch.int32),
             ev_count=torch.zeros(1, dtype=torch.int32),
             changes=left, cap=len(left) + 5, preload=0, phase=0)
    return u


def assert_second_pass_completes(ops, t, out, device="cpu"):
    """A second pass with room emits exactly what the first left out, from
    the same `from` state (a delayed event, not a lost one), and leaves the
    shadow equal to the states on every row that is not FREE."""
    u = second_pass_tables(t, out)
    out2 = call(ops, u, device)
    seen2 = assert_pass_is_sound(u, out2, stamp=2 * TICK)
    first = {(r[0], r[2]) for r in emitted_records(t, out)}
    assert first | seen2 == set(t["changes"]) and not first & seen2
    NR = int(t["run_life"].shape[0])
    live = t["run_life"] != WFL_FREE
    assert torch.equal(out2["ev_shadow_state"].view(NR, 64)[live],
                       t["step_state"].view(NR, 64)[live])


@functools.lru_cache(maxsize=None)
def oracle(NR, pattern, cap_mode):
    """(tables, oracle output): computed once, shared, never written."""
    t = build_journal_tables(NR, pattern, cap_mode)
    return t, call(ref_ops(), t)


def assert_case_is_the_case(t, NR, pattern, cap_mode):
    changes, roles, cap, preload = t["changes"], t["roles"], t["cap"], t["preload"]
    total = len(changes)
    state = t["step_state"].view(NR, 64)
    shadow = t["ev_shadow_state"].view(NR, 64)
    if pattern == "none":
        assert total == 0 and torch.equal(state, shadow)
        assert torch.equal(t["run_gen"], t["ev_shadow_gen"])
    if pattern == "last_step":
        assert list(changes) == [(NR - 1, 63)]
    if pattern == "one_row_all":
        assert sorted(changes) == [(roles["row"], s) for s in range(64)]
    if pattern == "all":
        assert total == NR * 64 and bool((state != shadow).all())
    if pattern == "regen":
        for r in roles["regen"]:
            assert int(t["run_gen"][r]) != int(t["ev_shadow_gen"][r])
            assert bool((shadow[r] != 0).all())            # stale and non-zero
            assert 0 < int((state[r] != 0).sum()) < 64     # some steps moved on
            # events of a re-admitted row start from PENDING, not the shadow
            assert all(changes[(r, s)][0] == WFS_PENDING for s in (0, 15, 16, 63))
    if pattern == "free_differs":
        for r in roles["free"]:
            assert int(t["run_life"][r]) == WFL_FREE and bool((state[r] != shadow[r]).all())
            assert not any(k[0] == r for k in changes)
    if pattern == "draining":
        for r in roles["draining"]:
            assert int(t["run_life"][r]) == WFL_DRAINING and (r, 63) in changes
    if pattern == "random" and NR >= 64:
        lives = set(t["run_life"].tolist())
        assert lives == {WFL_FREE, WFL_LIVE, WFL_DRAINING}
        assert bool((t["run_gen"] != t["ev_shadow_gen"]).any())
    if cap_mode != "ample":
        assert total >= 2
    want = {"ample": total, "ample_preload": total, "exact": total,
            "minus1": total - 1, "one": 1, "preload_cap": 0, "preload_above": 0}[cap_mode]
    assert expected_emitted(t) == want
    assert {"exact": cap == total, "minus1": cap == total - 1, "one": cap == 1,
            "preload_cap": preload == cap, "preload_above": preload > cap,
            "ample_preload": 0 < preload and preload + total == cap,
            "ample": cap > total}[cap_mode]


@pytest.mark.parametrize("NR,pattern,cap_mode", CASES)
def test_oracle_pass_on_a_hand_built_table(NR, pattern, cap_mode):
    t, out = oracle(NR, pattern, cap_mode)
    assert_case_is_the_case(t, NR, pattern, cap_mode)
    seen = assert_pass_is_sound(t, out)
    # the oracle visits rows and steps in ascending order: under a full list
    # it keeps the lowest (slot, step) changes, in that order, and its count
    # stops at cap
    recs = emitted_records(t, out)
    assert [(r[0], r[2]) for r in recs] == sorted(t["changes"])[:len(recs)]
    if t["preload"] < t["cap"]:
        assert int(out["ev_count"][0]) == t["preload"] + len(seen)
    if pattern == "none":
        assert torch.equal(out["ev_shadow_state"], t["ev_shadow_state"])
    assert_second_pass_completes(ref_ops(), t, out)


def test_a_record_packs_step_from_and_to_into_word2():
    t, out = oracle(65, "last_step", "ample")
    (frm, to), = t["changes"].values()
    assert out["ev_rec"][:4].tolist() == [64, int(t["run_gen"][64]),
                                          63 | frm << 8 | to << 16, STAMP]
    assert int(out["ev_count"][0]) == 1
