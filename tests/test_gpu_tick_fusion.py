"""The fused 5-launch tick (prologue | K2 pick | K1 from bit words | gate+route
| finish) against the one-kernel-per-stage sequence it replaced, on identical
inputs, run both on the GPU (same stage bodies, other kernels) and on the CPU
reference backend (no shared code); and K1-from-bits against the bitset K1
and the pack-then-MFMA path.

Everything here is an integer path, so per-slot outputs must be EQUAL. The
order of entries inside the compacted slot lists is unspecified (wave-level
atomics), so those are compared as sorted sets.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (B, rules, workers, payload words): every value the fusion can trip on —
# B around the 16-job MFMA tile, the 64-lane wave and the 256-thread block;
# R around the 16-rule tile and one multi-tile size; a single worker, a
# sub-block table and one past the pick kernel's 1024-entry LDS chunk (also
# past the K=1024 spread clamp); payload rows shorter than, equal to and one
# past a wave's 64 lanes
SHAPES = [
    (1, 1, 1, 1),
    (15, 16, 64, 64),
    (17, 17, 1025, 65),
    (255, 300, 64, 1),
    (257, 16, 1025, 64),
    (1000, 300, 1025, 65),
    (1000, 17, 1, 64),
]
CASES = ["default", "deny_all", "deny_none", "overloaded", "labels", "same_worker"]


def _policy(case, R):
    from cordum_amd.ops.pipeline import make_synthetic_policy
    from cordum_amd.safety import policy as pol

    # deny_frac high enough that small bundles hold deny rules too
    p = make_synthetic_policy(R, deny_frac=0.3, seed=3)
    if case == "deny_all":
        # rule 0 becomes a catch-all deny: first match for every job
        p.rules[0] = pol.PolicyRule(id="r0", match=pol.PolicyMatch(), decision="deny")
    elif case == "deny_none":
        for r in p.rules:
            r.decision = "allow"
    return p


def _mutate(pipe, case):
    """Case set-up applied identically to both pipelines (deterministic)."""
    B, NW = pipe.B, pipe.NWL
    d = pipe.device
    if case == "overloaded":
        # every worker over the cpu cut-off: valid_count = 0, nothing routable
        pipe.w_cpu_local.fill_(95.0)
        pipe.valid_buf.zero_()
    elif case == "labels":
        # distinct label needs: the exact pick runs and spreads over workers
        pipe.w_labels.copy_((torch.arange(NW, device=d) % 4) + 1)   # 1..4
        jl = torch.arange(B, device=d) % 5                          # 0 = unconstrained
        pipe.j_labels.copy_(torch.where(jl == 3, torch.ones_like(jl), jl).to(torch.int64))
    elif case == "same_worker":
        # every job constrained, every worker eligible: all pick the one
        # least-loaded worker (same-address histogram adds)
        pipe.w_labels.fill_(1)
        pipe.j_labels.fill_(1)
    # a non-trivial spread order (the eager refresh is not part of the body)
    pipe.order_buf.copy_(torch.arange(NW - 1, -1, -1, dtype=torch.int32, device=d))


def _run(case, shape, unfused, ticks=2, device=DEV, backend="ext", **extra):
    from cordum_amd.ops.pipeline import DevicePipeline

    B, R, NW, PW = shape
    pipe = DevicePipeline(device=torch.device(device), batch_size=B, n_local_workers=NW,
                          n_rules=R, n_batches=1, payload_words=PW, seed=3,
                          policy=_policy(case, R), mfma_pack_on_device=True,
                          unfused_tick=unfused, backend=backend, **extra)
    _mutate(pipe, case)
    sync = torch.cuda.synchronize if pipe.device.type == "cuda" else (lambda: None)
    mid = None
    for t in range(ticks):
        pipe._fused_body(0)
        if t == 0:
            sync()
            mid = pipe.w_active_local.cpu().clone()
    sync()
    return pipe, mid


EXACT = ["states", "attempts", "deadlines", "out_decision", "_counts", "res_sums",
         "res_arena", "w_active_local", "w_keys", "acc_counts", "dlq_head"]


def _compare(new, old, mid_new, mid_old):
    for name in EXACT:
        a, b = getattr(new, name).cpu(), getattr(old, name).cpu()
        assert torch.equal(a, b), f"{name} differs"
    assert torch.equal(mid_new, mid_old), "w_active_local after tick 1 differs"
    c = new._counts.cpu().tolist()
    n_den, n_all, n_rt = c[0], c[1], c[2]
    assert n_den + n_all == new.B

    def sset(p, name, n):
        return torch.sort(getattr(p, name)[:n].cpu()).values

    assert torch.equal(sset(new, "allowed_slots", n_all), sset(old, "allowed_slots", n_all))
    assert torch.equal(sset(new, "denied_slots", n_den), sset(old, "denied_slots", n_den))

    def pairs(p):
        s = p.routable_slots[:n_rt].cpu().to(torch.int64)
        w = p.routable_widx[:n_rt].cpu().to(torch.int64)
        return torch.sort(s * (1 << 32) + w).values

    assert torch.equal(pairs(new), pairs(old))
    # DLQ: two ticks appended 2 * n_den entries (ring is 65536 deep here)
    head = int(new.dlq_head.cpu()[0])
    assert torch.equal(torch.sort(new.dlq_ring[:head].cpu()).values,
                       torch.sort(old.dlq_ring[:head].cpu()).values)
    assert torch.equal(new.dlq_ring[head:].cpu(), old.dlq_ring[head:].cpu())
    return n_den, n_all, n_rt


def _check_case(case, shape, counts, mid_new):
    """The case must actually be the case."""
    n_den, n_all, n_rt = counts
    B = shape[0]
    if case == "deny_all":
        assert n_den == B and n_rt == 0
    elif case == "deny_none":
        assert n_den == 0 and n_rt == B
    elif case == "overloaded":
        assert n_rt == 0
    elif case == "same_worker":
        # tick 1: every allowed job landed on one worker
        assert int(mid_new.max()) == int(mid_new.sum()) == n_all
    elif case == "labels" and shape[2] >= 4 and B >= 5:
        assert n_rt > 0 and int((mid_new > 0).sum()) > 1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-R%d-W%d-P%d" % s)
@pytest.mark.parametrize("case", CASES)
def test_fused_tick_equals_unfused(case, shape):
    new, mid_new = _run(case, shape, unfused=False)
    assert new._use_mfma, "shape must exercise the MFMA K1-from-bits path"
    old, mid_old = _run(case, shape, unfused=True)
    _check_case(case, shape, _compare(new, old, mid_new, mid_old), mid_new)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-R%d-W%d-P%d" % s)
@pytest.mark.parametrize("case", CASES)
def test_fused_tick_equals_cpu_reference(case, shape):
    """The fused and staged GPU kernels share their stage bodies, so a fault
    in a body shows identically on both sides of the test above. The staged
    tick on the CPU reference backend shares no code with them: same
    arguments, same set-up, same comparison. Every compared field is an
    integer path except w_keys, whose score goes through float; it is
    compared with the worker loads as they are."""
    new, mid_new = _run(case, shape, unfused=False)
    assert new._use_mfma, "shape must exercise the MFMA K1-from-bits path"
    ref, mid_ref = _run(case, shape, unfused=True, device="cpu", backend="ref")
    _check_case(case, shape, _compare(new, ref, mid_new, mid_ref), mid_new)


@pytest.mark.parametrize("shape", [(257, 17, 64, 65), (1000, 300, 1025, 1)],
                         ids=lambda s: "B%d-R%d-W%d-P%d" % s)
def test_fused_tick_equals_unfused_bitset_k1(shape):
    """Outside the MFMA envelope the fused sequence keeps the bitset K1."""
    new, mid_new = _run("labels", shape, unfused=False, use_mfma=False)
    assert not new._use_mfma
    old, mid_old = _run("labels", shape, unfused=True, use_mfma=False)
    _compare(new, old, mid_new, mid_old)


def test_captured_fused_tick_matches_unfused_stats():
    """Through the real entry point (graph capture + replay), two ring slots."""
    from cordum_amd.ops.pipeline import DevicePipeline

    kw = dict(device=torch.device(DEV), batch_size=1000, n_local_workers=64, n_rules=300,
              n_batches=2, payload_words=17, seed=5, mfma_pack_on_device=True)
    new = DevicePipeline(**kw)
    old = DevicePipeline(unfused_tick=True, **kw)
    for _ in range(3):
        a, b = new.tick(), old.tick()
        assert (a.completed, a.denied, a.unrouted) == (b.completed, b.denied, b.unrouted)
    for name in ("states", "attempts", "res_sums", "out_decision", "w_active_local", "acc_counts"):
        assert torch.equal(getattr(new, name).cpu(), getattr(old, name).cpu()), name


# ---- K1 from bits -----------------------------------------------------------

K1_JS = (1, 15, 16, 17, 1000)
K1_RS = (1, 16, 17, 300)
# register-blocked K1 (2 job tiles per wave): J giving 1, 3 and 5 job tiles
# leaves the last block partially filled
K1_TILED_JS = (16, 33, 80)


def _k1_inputs(J, R, seed=9):
    from cordum_amd.ops.pipeline import encode_synthetic_jobs, make_synthetic_policy
    from cordum_amd.ops.policy_compile import compile_policy
    from cordum_amd.ops.policy_mfma import pack_jobs_mfma, pack_policy_mfma

    compiled = compile_policy(make_synthetic_policy(R, deny_frac=0.3, seed=seed), words=1)
    assert compiled.exact
    jobs = encode_synthetic_jobs(compiled, J, seed=seed + 1)
    # some jobs carry secrets so the per-rule secrets test is live
    jobs.secrets[::3] = 1
    return compiled, jobs, pack_policy_mfma(compiled), pack_jobs_mfma(jobs)[0]


def _k1_three_ways(ext, compiled, jobs, mp, a_pack, job_tiles=1):
    d = torch.device(DEV)
    J, R = jobs.n_jobs, compiled.n_rules
    cp = compiled.to(d)
    bitset = ext.policy_first_match(
        cp.any_masks, cp.all_masks, cp.secrets, cp.mcp_masks, cp.mcp_any,
        jobs.any_bits.to(d), jobs.all_bits.to(d), jobs.secrets.to(d),
        jobs.mcp_bits.to(d), jobs.mcp_used.to(d), 0).cpu()
    mpd = mp.to(d)
    packed = ext.policy_first_match_mfma(
        a_pack.to(d), mpd.b_pack, mpd.cards, mpd.secrets, jobs.secrets.to(d),
        mpd.tile_dims, J, R).cpu()
    out = torch.full((J,), 2 ** 31 - 1, dtype=torch.int32, device=d)
    ext.policy_first_match_mfma_bits_into(
        jobs.any_bits.to(d).contiguous(), jobs.all_bits.to(d).contiguous(),
        mpd.b_pack, mpd.cards, mpd.secrets, jobs.secrets.to(d), mpd.tile_dims, R, out,
        job_tiles)
    torch.cuda.synchronize()
    bits = out.cpu()
    bits = torch.where(bits == 2 ** 31 - 1, torch.full_like(bits, -1), bits)
    return bitset.to(torch.int32), packed.to(torch.int32), bits


@pytest.mark.parametrize("R", K1_RS)
@pytest.mark.parametrize("J", K1_JS)
def test_k1_from_bits_matches_bitset_and_packed(J, R):
    from cordum_amd.ops import get_ext
    from cordum_amd.ops.policy_compile import first_match_reference

    ext = get_ext(required=True)
    compiled, jobs, mp, a_pack = _k1_inputs(J, R)
    bitset, packed, bits = _k1_three_ways(ext, compiled, jobs, mp, a_pack)
    assert torch.equal(bits, bitset)
    assert torch.equal(bits, packed)
    assert torch.equal(bits, first_match_reference(compiled, jobs).to(torch.int32))


@pytest.mark.parametrize("job_tiles", (2,))
@pytest.mark.parametrize("R", (17, 300))
@pytest.mark.parametrize("J", K1_TILED_JS + (1000,))
def test_k1_from_bits_register_blocked(J, R, job_tiles):
    from cordum_amd.ops import get_ext

    ext = get_ext(required=True)
    compiled, jobs, mp, a_pack = _k1_inputs(J, R, seed=13)
    bitset, packed, bits = _k1_three_ways(ext, compiled, jobs, mp, a_pack, job_tiles)
    assert torch.equal(bits, bitset)
    assert torch.equal(bits, packed)


def test_k1_from_bits_rule_chunked():
    """R large enough that the launch splits the rule tiles over nchunks > 1
    blocks per job tile and the atomicMin epilogue merges them: J=17 gives 2
    job tiles, R=300 gives 19 rule tiles -> min(ceil(19/4), 2048/2) = 5."""
    from cordum_amd.ops import get_ext

    ext = get_ext(required=True)
    J, R = 17, 300
    Jt, Rt = (J + 15) // 16, (R + 15) // 16
    assert max(1, min((Rt + 3) // 4, max(1, 2048 // Jt))) > 1
    compiled, jobs, mp, a_pack = _k1_inputs(J, R, seed=21)
    bitset, packed, bits = _k1_three_ways(ext, compiled, jobs, mp, a_pack)
    assert torch.equal(bits, bitset) and torch.equal(bits, packed)
    assert int((bits >= 0).sum()) > 0
