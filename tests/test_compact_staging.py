"""Compact descriptor staging, host side: which set dimensions a compiled
policy reads (policy_mfma.live_dims), the layout of the buffer that carries
one column per such dimension (pipeline.alloc_compact_staging), and the native
encoder's compact mode (ext.synthetic_fresh_compact) against the full-layout
encoder it must agree with word for word (ext.synthetic_fresh_stamped).

The bundle builders here are shared with the GPU tests of the same feature.
"""
import pytest
import torch

from cordum_amd.ops import get_ext
from cordum_amd.ops.pipeline import alloc_compact_staging, make_synthetic_policy
from cordum_amd.ops.policy_compile import compile_policy
from cordum_amd.ops.policy_mfma import (COL_ABSENT, col_map, col_of, gather_live_cols,
                                        live_dims, pack_policy_mfma)
from cordum_amd.safety import policy as pol

# dimension numbers: the 7 any-of in JobBatch order, then the 2 all-of
TENANT, TOPIC, CAP, PACK, ACTOR, ATYPE, RISK, REQUIRES, LABELS = range(9)


def _rule(i, decision="allow", **match):
    return pol.PolicyRule(id=f"r{i}", match=pol.PolicyMatch(**match), decision=decision)


def tenants_only_policy(n_rules=5, vocab=48):
    return pol.SafetyPolicy(version="tenants", rules=[
        _rule(i, "deny" if i % 3 == 0 else "allow", tenants=[f"t{(7 * i + 1) % vocab}"])
        for i in range(n_rules)])


def all_dims_policy(n_rules=9, vocab=48):
    """Rule i constrains dimension i % 9 alone, over the synthetic job
    vocabulary where the synthetic jobs carry that dimension."""
    rules = []
    for i in range(n_rules):
        v = (5 * i + 2) % vocab
        match = [
            dict(tenants=[f"t{v}"]),
            dict(topics=[f"job.a{v}"]),
            dict(capabilities=[f"cap{v}"]),
            dict(pack_ids=[f"pack{v}"]),
            dict(actor_ids=[f"actor{v}"]),
            dict(actor_types=[f"atype{v}"]),
            dict(risk_tags=[f"tag{v}"]),
            dict(requires=[f"req{v}"]),
            dict(labels={"k": f"v{v}"}),
        ][i % 9]
        rules.append(_rule(i, "deny" if i % 2 else "allow", **match))
    return pol.SafetyPolicy(version="alldims", rules=rules)


def catch_all_policy(n_rules=3, secrets=False):
    """No rule constrains a set dimension. secrets=True makes rule 0 apply to
    jobs carrying secrets only (still no set dimension), so that first-match
    results differ from job to job."""
    rules = [_rule(i, "deny" if i == 0 else "allow") for i in range(n_rules)]
    if secrets:
        rules[0].match.secrets_present = True
    return pol.SafetyPolicy(version="catchall", rules=rules)


BIT63_VOCAB = 64  # the largest vocabulary a 1-word policy holds: ids 0..63


def bit63_policy(n_rules=4):
    """Rule 0 names all 64 tenants and requires all 64 requirements, so both
    interners run up to id 63 whatever n_rules is (a job with every
    requirement matches it: card 64 == dot 64). The next rules, cyclically:
    tenant t63 alone, requirement req63 alone, risk tag among tag0..tag63
    with tag63 interned last."""
    V = BIT63_VOCAB
    rules = [_rule(0, "deny", tenants=[f"t{v}" for v in range(V)],
                   requires=[f"req{v}" for v in range(V)])]
    for i in range(1, n_rules):
        kind = i % 3
        if kind == 1:
            rules.append(_rule(i, "deny", tenants=["t63"]))
        elif kind == 2:
            rules.append(_rule(i, "allow", requires=["req63"]))
        else:
            rules.append(_rule(i, "deny", risk_tags=[f"tag{v}" for v in range(V)][-(i % 7 + 1):]
                               if i > 3 else [f"tag{v}" for v in range(V)]))
    return pol.SafetyPolicy(version="bit63", rules=rules)


def packed(policy):
    compiled = compile_policy(policy, words=1)
    assert compiled.exact
    return compiled, pack_policy_mfma(compiled)


# ---- live dimensions ----------------------------------------------------------

def test_live_dims_tenants_only():
    _, mp = packed(tenants_only_policy())
    assert live_dims(mp) == [TENANT]


def test_live_dims_synthetic_bundle():
    _, mp = packed(make_synthetic_policy(256, seed=7))
    live = live_dims(mp)
    assert live == [TENANT, TOPIC, RISK, REQUIRES]
    assert live == sorted(live)


def test_live_dims_every_dimension():
    _, mp = packed(all_dims_policy())
    assert live_dims(mp) == list(range(9))


def test_live_dims_catch_all():
    _, mp = packed(catch_all_policy())
    assert live_dims(mp) == []


def test_live_dims_ignore_padding_rules():
    """Padding rules carry an impossible card on dim 7 so they never match;
    that must not make `requires` live (17 rules pad the second tile)."""
    _, mp = packed(tenants_only_policy(17))
    assert live_dims(mp) == [TENANT]


def test_col_map_nibbles():
    live = [TENANT, TOPIC, RISK, REQUIRES]
    m = col_map(live)
    nib = [(m >> (4 * d)) & 0xF for d in range(9)]
    assert nib == [0, 1, COL_ABSENT, COL_ABSENT, COL_ABSENT, COL_ABSENT, 2, 3, COL_ABSENT]
    assert m >> 36 == 0
    assert col_map([]) == int("F" * 9, 16)
    assert col_map(list(range(9))) == sum(d << (4 * d) for d in range(9))
    assert [col_of(live, d) for d in (TENANT, CAP, REQUIRES, LABELS)] == [0, -1, 3, -1]


# ---- allocator layout ---------------------------------------------------------

@pytest.mark.parametrize("B,L", [(1, 0), (1, 1), (17, 4), (64, 9)])
def test_alloc_compact_staging_layout(B, L):
    cols, sec, buf = alloc_compact_staging(B, L)
    assert buf.dtype == torch.uint8 and buf.dim() == 1 and buf.is_contiguous()
    assert buf.numel() == ((B * L * 8 + B + 7) // 8) * 8
    assert buf.numel() % 8 == 0 and buf.numel() >= B * L * 8 + B
    assert bool((buf == 0).all())
    assert cols.dtype == torch.int64 and tuple(cols.shape) == (B, L)
    assert sec.dtype == torch.uint8 and tuple(sec.shape) == (B,)
    base = buf.data_ptr()
    assert base % 8 == 0
    if L:
        assert cols.data_ptr() == base and cols.data_ptr() % 8 == 0
        assert cols.is_contiguous()
    assert sec.data_ptr() == base + B * L * 8
    # views, not copies: writes land in the flat buffer at those offsets
    sec.fill_(3)
    if L:
        cols.fill_(-1)
    assert bool((buf[:B * L * 8] == 255).all())
    assert bool((buf[B * L * 8:B * L * 8 + B] == 3).all())
    assert bool((buf[B * L * 8 + B:] == 0).all())


# ---- encoder equivalence --------------------------------------------------------

BS = (1, 63, 64, 65, 1000)
STEPS = (0, 9, 2 ** 32 + 5)
V = 48
PW = 5
DIMS = (0, 1, 6, 0)  # tenant, topic, risk of any_bits; requires of all_bits
SENTINEL = 0x5A5A5A5A5A


def _ext():
    ext = get_ext(required=False)
    if ext is None or not hasattr(ext, "synthetic_fresh_compact"):
        pytest.skip("HIP extension with synthetic_fresh_compact not built")
    return ext


def _luts(seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(-(1 << 62), 1 << 62, (V, 1), dtype=torch.int64, generator=g)
            for _ in range(4)]


def _full_reference(ext, B, luts, step, payload0):
    any_b = torch.zeros((B, 7, 1), dtype=torch.int64)
    all_b = torch.zeros((B, 2, 1), dtype=torch.int64)
    payload = payload0.clone()
    ext.synthetic_fresh_stamped(any_b, all_b, *luts, 11, step, *DIMS, payload, PW, 1, -1)
    from cordum_amd.ops.policy_compile import JobBatch

    jb = JobBatch(any_b, all_b, torch.zeros(B, dtype=torch.uint8),
                  torch.zeros((B, 4, 1), dtype=torch.int64), torch.zeros(B, dtype=torch.uint8))
    return jb, payload


# live sets: the synthetic four; the four among others (columns 0,1,3,5 of 6);
# one synthetic dim (risk) not live, with a neighbouring dim's column in its
# place (pack, which the encoder never writes: the sentinel there must stay)
LIVE_SETS = [
    [TENANT, TOPIC, RISK, REQUIRES],
    [TENANT, TOPIC, CAP, RISK, ATYPE, REQUIRES, LABELS],
    [TENANT, TOPIC, PACK, REQUIRES],
    [TOPIC],
]


@pytest.mark.parametrize("B", BS)
def test_fresh_compact_equals_gathered_fresh_stamped(B):
    ext = _ext()
    luts = _luts()
    g = torch.Generator().manual_seed(B)
    payload0 = torch.randint(-(1 << 31), (1 << 31) - 1, (B * PW,), dtype=torch.int32,
                             generator=g)
    levels = sorted(set(range(ext.encoder_isa_level() + 1)))
    for step in STEPS:
        ref, ref_payload = _full_reference(ext, B, luts, step, payload0)
        for live in LIVE_SETS:
            live = sorted(live)
            want = gather_live_cols(ref, live)
            columns = (col_of(live, TENANT), col_of(live, TOPIC), col_of(live, RISK),
                       col_of(live, REQUIRES))
            written = [c for c in columns if c >= 0]
            for threads in (1, 2):
                for isa in levels:
                    tag = f"B={B} step={step} live={live} threads={threads} isa={isa}"
                    cols = torch.full((B, len(live)), SENTINEL, dtype=torch.int64)
                    payload = payload0.clone()
                    ext.synthetic_fresh_compact(cols, *luts, 11, step, *columns,
                                                payload, PW, threads, isa)
                    assert torch.equal(cols[:, written], want[:, written]), tag
                    others = [c for c in range(len(live)) if c not in written]
                    # a column of a dim the encoder does not draw, and the
                    # column next to a skipped dim, keep the sentinel
                    assert bool((cols[:, others] == SENTINEL).all()), tag
                    assert torch.equal(payload, ref_payload), tag


def test_fresh_compact_no_live_dims_only_stamps():
    ext = _ext()
    luts = _luts()
    B = 65
    cols = torch.zeros((B, 0), dtype=torch.int64)
    payload = torch.arange(B * PW, dtype=torch.int32)
    ext.synthetic_fresh_compact(cols, *luts, 11, 9, -1, -1, -1, -1, payload, PW, 2, -1)
    rows = payload.view(B, PW)
    assert bool((rows[:, 0] == 9).all())
    assert torch.equal(rows[:, 1:], torch.arange(B * PW, dtype=torch.int32).view(B, PW)[:, 1:])


def test_fresh_compact_rejects_bad_columns():
    ext = _ext()
    luts = _luts()
    cols = torch.zeros((4, 2), dtype=torch.int64)
    with pytest.raises(RuntimeError):
        ext.synthetic_fresh_compact(cols, *luts, 1, 0, 0, 1, 2, -1, None, 0, 1, -1)
    with pytest.raises(RuntimeError):
        ext.synthetic_fresh_compact(cols, *luts, 1, 0, 0, 0, -1, -1, None, 0, 1, -1)


def test_standalone_sanitized_compact_program(tmp_path):
    """tests/native/encode_compact_check.cpp: the header's compact mode under
    ASan+UBSan as a program of its own, built and run the way
    test_native_encoder_fast.py builds and runs encode_check.cpp."""
    import shutil
    import subprocess
    from pathlib import Path

    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    root = Path(__file__).resolve().parent.parent
    src = root / "tests" / "native" / "encode_compact_check.cpp"
    exe = tmp_path / "encode_compact_check"
    cc = subprocess.run(
        [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-pthread",
         f"-I{root / 'cordum_amd' / 'ops' / 'hip'}", str(src), "-o", str(exe)],
        capture_output=True, text=True)
    if cc.returncode != 0 and "asan" in cc.stderr.lower() and "cannot find" in cc.stderr.lower():
        pytest.skip("sanitizer runtime libraries not installed")
    assert cc.returncode == 0, cc.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "encode_compact_check ok" in run.stdout


def test_pipeline_encoder_wrapper_compact_matches_fresh_stamped():
    """SyntheticEncoder.fresh_compact on a real policy's LUTs and live map."""
    ext = _ext()
    from cordum_amd.ops.pipeline import SyntheticEncoder, alloc_batch_staging

    compiled, mp = packed(make_synthetic_policy(64, seed=7))
    live = live_dims(mp)
    enc = SyntheticEncoder(compiled, seed=101)
    B = 257
    full, _ = alloc_batch_staging(B, 1)
    cols, sec, _ = alloc_compact_staging(B, len(live))
    pa = torch.arange(B * 64, dtype=torch.int32)
    pb = pa.clone()
    enc.fresh_stamped(full, 12, ext, pa, 64)
    enc.fresh_compact(cols, 12, ext, enc.compact_columns(live), pb, 64)
    assert torch.equal(cols, gather_live_cols(full, live))
    assert torch.equal(pa, pb)
    assert bool((sec == 0).all())
