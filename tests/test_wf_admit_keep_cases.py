"""Admission with kept steps (wf_admit_keep): the table builders, the oracle
call and the "the case is the case" assertions, with their CPU checks.

tests/test_gpu_wf_admit_keep.py runs every builder of this module on the
extension and compares with the oracle; here each builder goes through the
oracle alone, and what it returns is checked against statements of the
contract that do not share the oracle's code: validity from the dependency
lists the templates were built from, placement by request index, the step
states from the masks, every other column as a plain admission writes it.
With no step kept the tables must equal wf_admit_ref's on the same input.
"""
import functools

import pytest
import torch

from cordum_amd.ops import reference as ref
from tests import test_gpu_wf_admission as A

SIZES = A.SIZES
POISON, BIG, ROW_TABLES = A.POISON, A.BIG, A.ROW_TABLES
ARGS = A.ARGS["wf_admit"] + ("req_keep", "req_skip")
WORKSPACES = A.WORKSPACES
NOT_TABLES = ("free", "deps")       # builder notes, not kernel arguments
M64 = (1 << 64) - 1

# templates with strictly lower-triangular dependencies, so closed sets exist
TC = 4
NSTEPS = (64, 1, 3, 4)
DEPS = (
    {s: [s - 1] for s in range(1, 64)},     # a 64-deep chain: bit 63 is used
    {},                                     # one step
    {1: [0], 2: [0, 1]},                    # three steps
    {1: [0], 2: [0], 3: [1, 2]},            # a diamond
)
REQ_FANOUT = (7, 0, 4, 0)           # request i uses template i % 4 with this override
N_MODES = A.N_MODES
PATTERNS = ("all", "prefix", "skip", "dep_missing", "at_nsteps", "bit63", "mixed")
CASES = (
    # nothing kept: a plain admission, at every size and request count
    [(NR, "random", nm, "zero") for NR in SIZES for nm in N_MODES]
    + [(NR, "random", "F+1", p) for NR in SIZES for p in PATTERNS]
    # refusals of both kinds in one call, on tables with no or little room
    + [(NR, fm, "over_NR", "mixed") for NR in SIZES for fm in ("random", "none", "last")]
    + [(NR, "all", "F", "mixed") for NR in SIZES]
    + [(513, "third_block_first", "F+1", "mixed")]
)


def _i64(m):
    return m - (1 << 64) if m >= (1 << 63) else m


def _mask(steps):
    return sum(1 << s for s in steps)


def keep_of(pattern, i):
    """(keep, skip) of request i, which uses template i % TC."""
    tid = i % TC
    ns = NSTEPS[tid]
    full = (1 << ns) - 1
    if pattern == "zero":
        return 0, 0
    if pattern == "all":
        return full, 0
    if pattern == "prefix":             # a closed prefix: 32, 0, 1 and 2 steps
        return (1 << (ns // 2)) - 1, 0
    if pattern == "skip":               # every step kept, the odd ones as SKIPPED
        return full, full & 0xAAAAAAAAAAAAAAAA
    if pattern == "dep_missing":        # one dependency of a kept step is not kept
        return (_mask(range(10)) & ~(1 << 4), 1, _mask([1]), _mask([0, 1, 3]))[tid], 0
    if pattern == "at_nsteps":          # a bit exactly at n_steps (none exists at 64)
        return (full | (1 << ns)) & M64, 0
    if pattern == "bit63":              # valid on the 64-step template only
        return full | (1 << 63), 0
    assert pattern == "mixed"
    if i % 3 == 1:                      # refused: past the steps, or not closed
        return ((1 << 63) | (1 << 62), 2, _mask([0, 2]) | (1 << 3), _mask([3]))[tid], 0
    return ((full, _mask([0, 63])), (1, 1), (_mask([0, 1]), _mask([1])),
            (_mask([0, 2]), 0))[tid]


def build_templates(g):
    n = TC * 64
    t = {
        "tmpl_deps": A._rand_i64(n, g),     # garbage at and past n_steps
        "tmpl_kind": A._ri(0, 5, n, g, torch.uint8),
        "tmpl_todo": A._ri(1, 21, n, g),
        "tmpl_maxp": A._ri(0, 6, n, g),
        "tmpl_delay": A._ri(0, 6, n, g),
        "tmpl_nsteps": torch.tensor(NSTEPS, dtype=torch.uint8),
    }
    for tid, deps in enumerate(DEPS):
        for s in range(NSTEPS[tid]):
            t["tmpl_deps"][tid * 64 + s] = _i64(_mask(deps.get(s, [])))
    t["tmpl_kind"][0:64] = (torch.arange(64) % 5).to(torch.uint8)
    t["tmpl_kind"][2 * 64] = ref.WFK_FOR_EACH
    return t


def build_keep_tables(NR, free_mode, n_mode, pattern):
    t = dict(A.build_admit_tables(NR, free_mode, n_mode, seed=17))
    g = torch.Generator().manual_seed(23000 + NR)
    t.update(build_templates(g))
    n = int(t["req_tmpl"].shape[0])
    t["req_tmpl"] = (torch.arange(n) % TC).to(torch.int32)
    t["req_fanout"] = torch.tensor([REQ_FANOUT[i % TC] for i in range(n)],
                                   dtype=torch.int32)
    masks = [keep_of(pattern, i) for i in range(n)]
    t["req_keep"] = torch.tensor([_i64(k) for k, _ in masks], dtype=torch.int64)
    t["req_skip"] = torch.tensor([_i64(s) for _, s in masks], dtype=torch.int64)
    return t


def ref_ops():
    return A.ref_ops()


def call(ops, kernel, t, device="cpu"):
    """Run `kernel` (wf_admit_keep, or wf_admit on the same tables) on clones
    of the tables in `t`; returns every table as a CPU tensor."""
    d = {k: (v.clone().to(device) if torch.is_tensor(v) else v) for k, v in t.items()}
    args = ARGS if kernel == "wf_admit_keep" else A.ARGS["wf_admit"]
    getattr(ops, kernel)(*[d[a] for a in args])
    if str(device) != "cpu":
        torch.cuda.synchronize()
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def oracle(*case):
    """(tables, oracle output): computed once, shared, never written."""
    t = build_keep_tables(*case)
    return t, call(ref_ops(), "wf_admit_keep", t)


def is_closed(tid, keep):
    """The contract, from the dependency lists: every kept step is a step of
    the template and each of its dependencies is kept."""
    steps = [s for s in range(64) if keep >> s & 1]
    return all(s < NSTEPS[tid] and all(keep >> d & 1 for d in DEPS[tid].get(s, []))
               for s in steps)


def expected_slots(t):
    free, n = t["free"], int(t["req_tmpl"].shape[0])
    out = []
    for i in range(n):
        if not is_closed(i % TC, int(t["req_keep"][i]) & M64):
            out.append(-2)              # whatever the table holds
        else:
            out.append(free[i] if i < len(free) else -1)
    return out


def assert_keep_case(t, want):
    """Placement, counters and the row image, stated independently of the
    oracle's code path."""
    n = int(t["req_tmpl"].shape[0])
    slots = expected_slots(t)
    assert want["out_slot"].tolist() == slots
    taken = [(i, s) for i, s in enumerate(slots) if s >= 0]
    assert int(want["admit_count"][0]) == BIG + len(taken)
    for i, s in enumerate(slots):
        assert int(want["out_gen"][i]) == (int(t["run_gen"][s]) + 1 if s >= 0 else 0)
    # rows of slots that were not handed out are untouched: the free slot of
    # a refused request stays FREE, its generation as it was
    keep = torch.ones(t["run_life"].shape[0], dtype=torch.bool)
    keep[[s for _, s in taken]] = False
    for k in ROW_TABLES:
        assert torch.equal(want[k].view(-1, 64)[keep], t[k].view(-1, 64)[keep]), k
    for k in ("n_steps", "cond_bits", "run_state", "run_active", "run_life", "run_gen"):
        assert torch.equal(want[k][keep], t[k][keep]), k
    for i, s in enumerate(slots):
        if s == -2 and i < len(t["free"]):
            assert int(want["run_life"][t["free"][i]]) == ref.WFL_FREE
    for i, slot in taken:
        tid = i % TC
        ns = NSTEPS[tid]
        kmask, smask = int(t["req_keep"][i]) & M64, int(t["req_skip"][i]) & M64
        assert int(want["n_steps"][slot]) == ns
        assert int(want["run_life"][slot]) == ref.WFL_LIVE
        assert int(want["run_active"][slot]) == 1 and int(want["run_state"][slot]) == 0
        assert int(want["cond_bits"][slot]) == int(t["req_cond"][i])
        row = {k: want[k].view(-1, 64)[slot] for k in ROW_TABLES}
        assert row["step_state"].tolist() == [
            ref.WFS_SKIPPED if smask >> s & 1 else ref.WFS_SUCCEEDED if kmask >> s & 1
            else ref.WFS_PENDING for s in range(64)]
        for k in ROW_TABLES:                  # zero at and past n_steps
            assert not bool(row[k][ns:].any()), (k, slot)
        for k in ("step_attempts", "children_out", "children_done", "children_fail",
                  "children_emitted"):
            assert not bool(row[k].any()), (k, slot)
        tr = slice(tid * 64, tid * 64 + ns)
        kind = t["tmpl_kind"][tr]
        assert torch.equal(row["step_kind"][:ns], kind)
        assert torch.equal(row["deps_mask"][:ns], t["tmpl_deps"][tr])
        assert torch.equal(row["max_parallel"][:ns], t["tmpl_maxp"][tr])
        assert torch.equal(row["next_ready"][:ns], A.ADMIT_TICK + 1 + t["tmpl_delay"][tr])
        assert bool((row["dispatch_tick"][:ns] == A.ADMIT_TICK + 1).all())
        todo = t["tmpl_todo"][tr].clone()
        if REQ_FANOUT[tid] > 0:
            todo[kind == ref.WFK_FOR_EACH] = REQ_FANOUT[tid]
        assert torch.equal(row["children_todo"][:ns], todo)
    assert n == len(slots)


@pytest.mark.parametrize("NR,free_mode,n_mode,pattern", CASES)
def test_keep_tables_hold_their_cases(NR, free_mode, n_mode, pattern):
    t, want = oracle(NR, free_mode, n_mode, pattern)
    assert_keep_case(t, want)
    F, n = len(t["free"]), int(t["req_tmpl"].shape[0])
    assert n == {"zero": 0, "one": 1, "F": F, "F+1": F + 1, "over_NR": NR + 3}[n_mode]
    slots = want["out_slot"].tolist()
    # the workspaces are the kernel's own: the oracle leaves them alone
    assert bool((want["free_mask"] == POISON).all())
    if pattern == "zero":
        # nothing kept: every table is what the plain admission writes
        A.assert_tables_equal(want, call(ref_ops(), "wf_admit", t), skip=NOT_TABLES)
        assert -2 not in slots
    if pattern in ("all", "prefix", "skip"):
        assert -2 not in slots and slots[-1] == -1
    if pattern == "mixed" and n >= 2:
        assert slots[1] == -2
        if n_mode == "over_NR":           # both refusals in one call
            assert -1 in slots and -2 in slots[F:]
        if F >= 3:                        # a valid request after a refused one
            assert slots[0] == t["free"][0] and slots[2] == t["free"][2]
            assert int(want["run_life"][t["free"][1]]) == ref.WFL_FREE
            assert int(want["run_gen"][t["free"][1]]) == int(t["run_gen"][t["free"][1]])


def test_patterns_are_what_they_are_called():
    t, want = oracle(65, "all", "F", "mixed")
    slots = want["out_slot"].tolist()
    assert slots[:4] == [0, -2, 2, 3] and slots.count(-2) == 22
    t, want = oracle(257, "random", "F+1", "all")
    st = want["step_state"].view(-1, 64)
    s0 = int(want["out_slot"][0])             # the 64-step template, bit 63 kept
    assert int(t["req_keep"][0]) == -1 and st[s0].tolist() == [ref.WFS_SUCCEEDED] * 64
    t, want = oracle(257, "random", "F+1", "skip")
    st = want["step_state"].view(-1, 64)
    s0 = int(want["out_slot"][0])
    assert st[s0].tolist() == [ref.WFS_SUCCEEDED, ref.WFS_SKIPPED] * 32
    assert int(t["req_skip"][0]) < 0          # bit 63 among the skipped
    t, want = oracle(257, "random", "F+1", "prefix")
    assert int(t["req_keep"][0]) == (1 << 32) - 1 and int(want["out_slot"][0]) >= 0
    # one dependency missing: refused on every template that has a dependency
    t, want = oracle(65, "random", "F+1", "dep_missing")
    assert want["out_slot"][:4].tolist()[0] == -2 and int(want["out_slot"][1]) >= 0
    assert want["out_slot"][2:4].tolist() == [-2, -2]
    # a bit exactly at n_steps: refused, but a 64-step template has none
    t, want = oracle(65, "random", "F+1", "at_nsteps")
    assert int(want["out_slot"][0]) >= 0 and want["out_slot"][1:4].tolist() == [-2] * 3
    assert [int(t["req_keep"][i]) for i in (1, 2, 3)] == [3, 15, 31]
    # bit 63 on the 3-step template
    t, want = oracle(65, "random", "F+1", "bit63")
    assert int(t["req_keep"][2]) == _i64((1 << 63) | 7)
    assert int(want["out_slot"][0]) >= 0 and want["out_slot"][1:4].tolist() == [-2] * 3
    # -2 wins over a full table
    t, want = oracle(65, "none", "over_NR", "mixed")
    assert set(want["out_slot"].tolist()) == {-1, -2}
    assert int(want["admit_count"][0]) == BIG
