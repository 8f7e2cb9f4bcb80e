"""The three kernels of device-decided conditions (wf_cond_eval,
wf_child_payload, wf_apply_out) on hand-built tables, oracle only: no GPU is
needed here.

The table builders and the checks are module-level functions, and
tests/test_gpu_wf_cond.py imports them to run the HIP kernels on the same
cases. A builder plants steps by role and records what a correct pass owes
for each, so the expected tables are known without running the code under
test; every cell nobody owes anything for holds a poison value before and
must hold it afterwards. All outputs are pure functions of the tables, so
every table and both counters are compared exactly.

Layout edges of wf_cond_eval: 4 lanes per row (16 steps each), 16 rows per
wave and 64 rows per block: one row, the wave edge (15, 16, 17), the block
edge (64, 65) and a fifth block with one row (257).
"""
import functools
import itertools
import operator
import random

import pytest
import torch

from cordum_amd.ops.reference import (
    WFK_APPROVAL,
    WFK_CONDITION,
    WFK_DELAY,
    WFK_FOR_EACH,
    WFK_WORKER,
    WFL_DRAINING,
    WFL_FREE,
    WFL_LIVE,
    WFS_PENDING,
    WFS_SKIPPED,
    WFS_SUCCEEDED,
    wf_drop_hash,
    wf_fail_hash,
)

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
POISON = -77
TC = 3                                   # templates; row r runs template r % TC
IW = 4
VALS = (I32_MIN, -1, 0, I32_MAX)         # where signed and unsigned compares disagree
TRUE0, FALSE0 = 1000, 2000               # the counters before the pass
SIZES = (1, 15, 16, 17, 64, 65, 257)

EQ, NE, LT, LE, GT, GE, TRUTHY = 1, 2, 3, 4, 5, 6, 7
K_IMM, K_INPUT, K_OUT = 0, 1, 2
_PY = {EQ: operator.eq, NE: operator.ne, LT: operator.lt, LE: operator.le,
       GT: operator.gt, GE: operator.ge}

COND_ARGS = ("step_state", "deps_mask", "step_kind", "run_life", "run_active",
             "run_tmpl", "tmpl_cond", "tmpl_cond_mask", "run_input", "step_out",
             "cond_bits", "cond_counts", "input_words")
COND_READ_ONLY = ("deps_mask", "step_kind", "run_life", "run_active", "run_tmpl",
                  "tmpl_cond", "tmpl_cond_mask", "run_input")


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


def _i64(m):
    return m - (1 << 64) if m >= (1 << 63) else m


def _code(op, lk, rk=K_IMM, neg=False):
    return op | (16 if neg else 0) | (lk << 8) | (rk << 12)


def _value(op, neg, lhs, rhs):
    v = (lhs != 0) if op == TRUTHY else _PY[op](lhs, rhs)
    return v != neg


# ---- wf_cond_eval -----------------------------------------------------------
# Steps 0..3 are finished steps whose output words are the operands, step 4 is
# a dependency that is not met, step 5 one that is SKIPPED. Steps 8..35 hold
# this template's share of the 84 (op, negate, lhs kind, rhs kind) forms, all
# CONDITION steps without deps. The roles follow from step 36.
COMBOS = list(itertools.product((EQ, NE, LT, LE, GT, GE, TRUTHY), (False, True),
                                (K_INPUT, K_OUT), (K_IMM, K_INPUT, K_OUT)))
assert len(COMBOS) == 84
S_UNMET, S_SKIPDEP = 4, 5
GUARD_KINDS = (WFK_WORKER, WFK_FOR_EACH, WFK_APPROVAL, WFK_DELAY)


def _row_kind(r):
    """What the pass owes row r as a whole."""
    m = r % 16
    if r == 0:
        return "live"
    return {5: "free", 7: "draining", 9: "inactive", 11: "quiet",
            13: "bad_tmpl"}.get(m, "live")


def build_cond_tables(NR):
    rng = random.Random(900 + NR)
    state = [[rng.randrange(1, 7) if s >= 36 else WFS_SUCCEEDED for s in range(64)]
             for _ in range(NR)]
    kind = [[rng.choice(GUARD_KINDS) for _ in range(64)] for _ in range(NR)]
    deps = [[0] * 64 for _ in range(NR)]
    out = [[POISON] * 64 for _ in range(NR)]
    rec = [[(POISON,) * 4 for _ in range(64)] for _ in range(TC)]
    mask = [0] * TC
    life = [WFL_LIVE] * NR
    active = [1] * NR
    tmpl = [r % TC for r in range(NR)]
    inp = [[VALS[(k + r // TC) % 4] for k in range(IW)] for r in range(NR)]
    bits = [rng.getrandbits(64) for _ in range(NR)]

    def setrec(t, s, r4):
        rec[t][s] = tuple(r4)
        mask[t] |= 1 << s

    # the records, per template
    for t in range(TC):
        for n, c in enumerate(c for i, c in enumerate(COMBOS) if i % TC == t):
            op, neg, lk, rk = c
            a, b = (n + t) % 4, (n // 4 + 2 * t) % 4
            setrec(t, 8 + n, (_code(op, lk, rk, neg), a, b, VALS[b]))
        # signed, not unsigned: -1 < 0, INT32_MAX > INT32_MIN as an immediate
        setrec(t, 36, (_code(LT, K_INPUT, K_IMM), 0, 0, 0))      # see "signed"
        # guards: input word IW - 1 against itself, never equal when negated
        for s in (39, 40, 41, 42):                               # false on each kind
            setrec(t, s, (_code(NE, K_INPUT, K_INPUT), 3, 3, 0))
        setrec(t, 43, (_code(EQ, K_INPUT, K_INPUT), 3, 3, 0))    # true guard
        setrec(t, 44, (_code(NE, K_INPUT, K_INPUT), 3, 3, 0))    # unmet deps
        setrec(t, 45, (_code(NE, K_OUT, K_OUT), 1, 1, 0))        # dep SKIPPED
        for s in range(46, 52):                                  # not PENDING
            setrec(t, s, (_code(NE, K_INPUT, K_INPUT), 3, 3, 0))
        setrec(t, 52, (_code(EQ, K_INPUT, K_INPUT, neg=True), 2, 2, 0))  # after 45
        setrec(t, 53, (_code(GE, K_OUT, K_OUT), 2, 2, 0))        # after 52, CONDITION
        # step 63: true on template 0, false on 1, by the row's input on 2
        setrec(t, 63, [(_code(EQ, K_INPUT, K_INPUT), 0, 0, 0),
                       (_code(EQ, K_INPUT, K_INPUT, neg=True), 0, 0, 0),
                       (_code(TRUTHY, K_INPUT), 1, 0, 0)][t])

    want = {"state": {}, "out": {}, "set": [0] * NR, "clr": [0] * NR,
            "true": 0, "false": 0, "roles": {}}

    def seen(role):
        want["roles"][role] = want["roles"].get(role, 0) + 1

    for r in range(NR):
        t = tmpl[r]
        rk_ = _row_kind(r)
        acted = rk_ == "live"
        if rk_ == "free":
            life[r] = WFL_FREE
        elif rk_ == "draining":
            life[r] = WFL_DRAINING
        elif rk_ == "inactive":
            active[r] = 0
        elif rk_ == "bad_tmpl":
            tmpl[r] = TC if (r // 16) % 2 else -1
        seen("row_" + rk_)
        for s in range(4):
            out[r][s] = VALS[(s + r // TC + 1) % 4]
            kind[r][s] = WFK_WORKER
        state[r][S_UNMET], state[r][S_SKIPDEP] = 1 + r % 2, WFS_SKIPPED  # DISPATCHED / WAITING
        out[r][S_SKIPDEP] = 0

        def cond_step(s, dep=()):
            state[r][s], kind[r][s] = WFS_PENDING, WFK_CONDITION
            deps[r][s] = sum(1 << d for d in dep)

        def owe_cond(s, v):
            want["set" if v else "clr"][r] |= 1 << s
            want["out"][(r, s)] = int(v)
            want["true" if v else "false"] += 1

        def operand(k, idx, imm):
            return inp[r][idx] if k == K_INPUT else out[r][idx] if k == K_OUT else imm

        # the 28 forms of this template
        for s in range(8, 36):
            cond_step(s)
            if rk_ == "quiet":
                state[r][s] = WFS_SUCCEEDED
            code, a, b, imm = rec[t][s]
            if acted:
                v = _value(code & 15, bool(code & 16), operand((code >> 8) & 3, a, 0),
                           operand((code >> 12) & 3, b, imm))
                owe_cond(s, v)
                seen(f"form_{'true' if v else 'false'}")
        # signed compare of an input word with 0: true only for negative words
        cond_step(36)
        if acted:
            owe_cond(36, inp[r][0] < 0)
            seen("signed")
        # CONDITION steps without a predicate: the admitted bits survive
        for s, b in ((37, 1), (38, 0)):
            cond_step(s)
            bits[r] = (bits[r] & ~(1 << s)) | (b << s)
            seen("plain_cond")
        # false guards on every other kind -> SKIPPED
        for s, k in zip((39, 40, 41, 42), GUARD_KINDS):
            state[r][s], kind[r][s] = WFS_PENDING, k
            if acted:
                want["state"][(r, s)] = WFS_SKIPPED
                want["false"] += 1
                seen(f"guard_false_kind{k}")
        state[r][43], kind[r][43] = WFS_PENDING, WFK_FOR_EACH         # true: untouched
        if acted:
            want["true"] += 1
            seen("guard_true")
        state[r][44], kind[r][44], deps[r][44] = WFS_PENDING, WFK_WORKER, 1 << S_UNMET
        seen("unmet_deps")
        state[r][45], kind[r][45], deps[r][45] = WFS_PENDING, WFK_WORKER, 1 << S_SKIPDEP
        if acted:
            want["state"][(r, 45)] = WFS_SKIPPED
            want["false"] += 1
            seen("dep_skipped")
        for s in range(46, 52):                                   # states 1 .. 6
            state[r][s], kind[r][s] = s - 45, WFK_WORKER
            seen("not_pending")
        # 45 is skipped in this pass: 52 (false guard on it) follows in the
        # same launch, and so does the CONDITION 53 that waits for 52
        state[r][52], kind[r][52], deps[r][52] = WFS_PENDING, WFK_DELAY, 1 << 45
        cond_step(53, dep=(52, 0))
        cond_step(63)
        if rk_ == "quiet":
            for s in (36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 52, 53, 63):
                state[r][s] = WFS_SUCCEEDED
        if acted:
            want["state"][(r, 52)] = WFS_SKIPPED
            want["false"] += 1
            owe_cond(53, True)
            v63 = [True, False, inp[r][1] != 0][t]
            owe_cond(63, v63)
            seen("cond63_true" if v63 else "cond63_false")
            seen("chain")

    t = {
        "step_state": torch.tensor(state, dtype=torch.uint8).reshape(-1),
        "deps_mask": torch.tensor([[_i64(m) for m in row] for row in deps],
                                  dtype=torch.int64).reshape(-1),
        "step_kind": torch.tensor(kind, dtype=torch.uint8).reshape(-1),
        "run_life": torch.tensor(life, dtype=torch.uint8),
        "run_active": torch.tensor(active, dtype=torch.uint8),
        "run_tmpl": torch.tensor(tmpl, dtype=torch.int32),
        "tmpl_cond": torch.tensor(rec, dtype=torch.int32).reshape(-1),
        "tmpl_cond_mask": torch.tensor([_i64(m) for m in mask], dtype=torch.int64),
        "run_input": torch.tensor(inp, dtype=torch.int32).reshape(-1),
        "step_out": torch.tensor(out, dtype=torch.int32).reshape(-1),
        "cond_bits": torch.tensor([_i64(b) for b in bits], dtype=torch.int64),
        "cond_counts": torch.tensor([TRUE0, FALSE0], dtype=torch.int64),
        "input_words": IW,
        "_want": want,
    }
    return t


def cond_call(ops, t, device="cpu"):
    return _run(ops, "wf_cond_eval", t, COND_ARGS, device)


def cond_expected(t):
    """The tables a correct pass leaves, from what the builder owes."""
    w = t["_want"]
    NR = int(t["run_life"].shape[0])
    st = t["step_state"].clone()
    out = t["step_out"].clone()
    bits = t["cond_bits"].clone()
    for (r, s), v in w["state"].items():
        st[r * 64 + s] = v
    for (r, s), v in w["out"].items():
        out[r * 64 + s] = v
    for r in range(NR):
        b = int(bits[r]) & ((1 << 64) - 1)
        bits[r] = _i64((b & ~w["clr"][r]) | w["set"][r])
    counts = torch.tensor([TRUE0 + w["true"], FALSE0 + w["false"]], dtype=torch.int64)
    return {"step_state": st, "step_out": out, "cond_bits": bits, "cond_counts": counts}


def assert_cond_exact(t, got):
    for k, v in cond_expected(t).items():
        bad = torch.nonzero(got[k] != v).flatten().tolist()[:8]
        assert not bad, (k, bad, [int(got[k][i]) for i in bad], [int(v[i]) for i in bad])
    for k in COND_READ_ONLY:
        assert torch.equal(got[k], t[k]), k


@functools.lru_cache(maxsize=None)
def cond_tables(NR):
    return build_cond_tables(NR)


@pytest.mark.parametrize("NR", SIZES)
def test_wf_cond_eval_oracle_gives_what_the_builder_owes(NR):
    t = cond_tables(NR)
    assert_cond_exact(t, cond_call(ref_ops(), t))


def test_wf_cond_eval_cases_plant_every_role():
    roles = {}
    for NR in SIZES:
        for k, v in cond_tables(NR)["_want"]["roles"].items():
            roles[k] = roles.get(k, 0) + v
    for k in ("row_live", "row_free", "row_draining", "row_inactive", "row_quiet",
              "row_bad_tmpl", "form_true", "form_false", "signed", "plain_cond",
              "guard_true", "unmet_deps", "dep_skipped", "not_pending", "chain",
              "cond63_true", "cond63_false") + tuple(
                  f"guard_false_kind{k}" for k in GUARD_KINDS):
        assert roles.get(k, 0) > 0, k
    # all 84 forms are held by the three templates together, in three lanes
    t = cond_tables(65)
    codes = t["tmpl_cond"].view(TC, 64, 4)[:, 8:36, 0].reshape(-1).tolist()
    assert len(set(codes)) == 84
    # one row's predicates write cond_bits from lanes 0, 1, 2 and 3
    w = t["_want"]
    m = w["set"][1] | w["clr"][1]
    assert all(m >> (16 * q) & 0xFFFF for q in range(4))
    # operands where a signed and an unsigned compare disagree
    signed = [int(t["run_input"][r * IW]) for r in range(65)]
    assert I32_MIN in signed and -1 in signed and I32_MAX in signed and 0 in signed


def test_wf_cond_eval_quiet_table_writes_nothing():
    """Nothing PENDING carries a predicate: not one word changes, the
    counters included."""
    t = dict(cond_tables(65))
    t["step_state"] = torch.where(t["step_state"] == WFS_PENDING,
                                  torch.tensor(WFS_SUCCEEDED, dtype=torch.uint8),
                                  t["step_state"])
    got = cond_call(ref_ops(), t)
    for k in COND_ARGS[:-1]:
        assert torch.equal(got[k], t[k]), k


# ---- wf_child_payload -------------------------------------------------------
PAYLOAD_ARGS = ("child_tag", "child_seq", "child_count", "run_input", "child_payload",
                "input_words", "payload_words")
PAYLOAD_CB, PAYLOAD_NR = 80, 5
# (count, CB, IW, W); the last one has more rows than one pass of the grid
# (one wave per row, 2048 blocks of 4 waves)
PAYLOAD_CASES = [(c, PAYLOAD_CB, iw, w) for c in (0, 1, 63, 64, 65, 100)
                 for iw, w in ((1, 3), (8, 10), (8, 64))] + [(8200, 8200, 8, 10)]


@functools.lru_cache(maxsize=None)
def build_payload_tables(count, CB, iw, w):
    rng = random.Random(count * 131 + iw * 7 + w)
    NR = PAYLOAD_NR
    tag = [rng.randrange(NR) * 64 + rng.randrange(64) for _ in range(CB)]
    seq = [rng.choice((0, 1, 7, I32_MAX, rng.randrange(1 << 20))) for _ in range(CB)]
    inp = [[rng.choice(VALS + (rng.randrange(-(1 << 31), 1 << 31),)) for _ in range(iw)]
           for _ in range(NR)]
    want = [[POISON] * w for _ in range(CB)]
    for c in range(min(count, CB)):
        want[c] = inp[tag[c] // 64] + [seq[c], tag[c] % 64] + [0] * (w - iw - 2)
    return {
        "child_tag": torch.tensor(tag, dtype=torch.int32),
        "child_seq": torch.tensor(seq, dtype=torch.int32),
        "child_count": torch.tensor([count], dtype=torch.int32),
        "run_input": torch.tensor(inp, dtype=torch.int32).reshape(-1),
        "child_payload": torch.full((CB * w,), POISON, dtype=torch.int32),
        "input_words": iw, "payload_words": w,
        "_want": torch.tensor(want, dtype=torch.int32).reshape(-1),
    }


def payload_call(ops, t, device="cpu"):
    return _run(ops, "wf_child_payload", t, PAYLOAD_ARGS, device)


def assert_payload_exact(t, got):
    assert torch.equal(got["child_payload"], t["_want"])
    for k in ("child_tag", "child_seq", "child_count", "run_input"):
        assert torch.equal(got[k], t[k]), k


@pytest.mark.parametrize("count,CB,iw,w", PAYLOAD_CASES)
def test_wf_child_payload_oracle_gives_what_the_builder_owes(count, CB, iw, w):
    t = build_payload_tables(count, CB, iw, w)
    assert_payload_exact(t, payload_call(ref_ops(), t))


# ---- wf_apply_out -----------------------------------------------------------
APPLY_ARGS = ("send_slots", "send_cnt", "child_tag", "child_seq", "rq_prev_tag",
              "rq_prev_seq", "children_done", "children_fail", "children_out",
              "fail_ppt", "drop_ppt", "cap", "world")
APPLY_OUT_ARGS = APPLY_ARGS[:9] + ("sums_back", "step_out") + APPLY_ARGS[9:]
APPLY_CASES = [(cap, world, f, d) for cap in (1, 64, 65) for world in (1, 2)
               for f in (0, 500, 1000) for d in (0, 500, 1000)]
APPLY_NR, APPLY_CB, APPLY_RQ = 3, 32, 8


@functools.lru_cache(maxsize=None)
def build_apply_tables(cap, world, fail_ppt, drop_ppt):
    rng = random.Random(cap * 1009 + world * 101 + fail_ppt + 3 * drop_ppt)
    NS = APPLY_NR * 64
    # few distinct steps, so that several children add into one output word
    tags = [rng.randrange(NS) for _ in range(5)]
    child_tag = [rng.choice(tags) for _ in range(APPLY_CB)]
    child_seq = [rng.randrange(1 << 16) for _ in range(APPLY_CB)]
    rq_tag = [rng.choice(tags) for _ in range(APPLY_RQ)]
    rq_seq = [rng.randrange(1 << 16) for _ in range(APPLY_RQ)]
    # region 0 is full and says more than cap (it clamps); region 1 is short
    cnt = [cap + 5, max(0, cap - 3)][:world]
    slots = [POISON * 1000] * (world * cap)
    sums = [POISON] * (world * cap)
    done, fail, outc = [[rng.randrange(0, 9) for _ in range(NS)] for _ in range(3)]
    step_out = [rng.choice((0, I32_MAX, I32_MIN, -1, 12345)) for _ in range(NS)]
    want = {"done": list(done), "fail": list(fail), "out": list(outc),
            "step_out": list(step_out), "n_done": 0, "n_wrapped": 0, "n_redelivered": 0}
    for r in range(world):
        for e in range(min(cnt[r], cap)):
            i = r * cap + e
            if rng.random() < 0.3:
                j = rng.randrange(APPLY_RQ)
                slots[i], tag, seq = -1 - j, rq_tag[j], rq_seq[j]
                want["n_redelivered"] += 1
            else:
                s = rng.randrange(APPLY_CB)
                slots[i], tag, seq = s, child_tag[s], child_seq[s]
            sums[i] = rng.choice((I32_MAX, I32_MIN, -1, 1, rng.randrange(-(1 << 31), 1 << 31)))
            if wf_drop_hash(tag, seq) % 1000 < drop_ppt:
                continue
            if wf_fail_hash(tag, seq) % 1000 < fail_ppt:
                want["fail"][tag] += 1
            else:
                want["done"][tag] += 1
                full = want["step_out"][tag] + sums[i]
                v = (full + (1 << 31)) % (1 << 32) - (1 << 31)
                want["n_wrapped"] += int(v != full)
                want["step_out"][tag] = v
                want["n_done"] += 1
            want["out"][tag] -= 1

    def ti(x):
        return torch.tensor(x, dtype=torch.int32)

    return {
        "send_slots": ti(slots), "send_cnt": ti(cnt), "child_tag": ti(child_tag),
        "child_seq": ti(child_seq), "rq_prev_tag": ti(rq_tag), "rq_prev_seq": ti(rq_seq),
        "children_done": ti(done), "children_fail": ti(fail), "children_out": ti(outc),
        "sums_back": ti(sums), "step_out": ti(step_out),
        "fail_ppt": fail_ppt, "drop_ppt": drop_ppt, "cap": cap, "world": world,
        "_want": want,
    }


def apply_out_call(ops, t, device="cpu"):
    return _run(ops, "wf_apply_out", t, APPLY_OUT_ARGS, device)


def apply_call(ops, t, device="cpu"):
    return _run(ops, "wf_apply", t, APPLY_ARGS, device)


def assert_apply_out_exact(t, got):
    w = t["_want"]
    for k, col in (("children_done", "done"), ("children_fail", "fail"),
                   ("children_out", "out"), ("step_out", "step_out")):
        assert got[k].tolist() == w[col], k
    for k in ("send_slots", "send_cnt", "child_tag", "child_seq", "rq_prev_tag",
              "rq_prev_seq", "sums_back"):
        assert torch.equal(got[k], t[k]), k


def assert_apply_counters_equal(got, plain):
    for k in ("children_done", "children_fail", "children_out"):
        assert torch.equal(got[k], plain[k]), k


@pytest.mark.parametrize("cap,world,fail_ppt,drop_ppt", APPLY_CASES)
def test_wf_apply_out_oracle_gives_what_the_builder_owes(cap, world, fail_ppt, drop_ppt):
    t = build_apply_tables(cap, world, fail_ppt, drop_ppt)
    got = apply_out_call(ref_ops(), t)
    assert_apply_out_exact(t, got)
    assert_apply_counters_equal(got, apply_call(ref_ops(), t))


def test_wf_apply_out_cases_wrap_and_redeliver():
    w = [build_apply_tables(*c)["_want"] for c in APPLY_CASES]
    assert sum(x["n_wrapped"] for x in w) > 0
    assert sum(x["n_redelivered"] for x in w) > 0
    assert sum(x["n_done"] for x in w) > 0
    # at 1000 per mille everything fails or is dropped: no output moves
    for c in APPLY_CASES:
        if c[2] == 1000 or c[3] == 1000:
            t = build_apply_tables(*c)
            assert t["_want"]["step_out"] == t["step_out"].tolist()
