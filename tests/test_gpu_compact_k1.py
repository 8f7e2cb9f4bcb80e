"""K1 from compact rows (ext.policy_first_match_mfma_cols_into: one int64
column per set dimension the compiled policy reads) against K1 from the full
bit-word layout, whose MFMA rule scan it shares, and against
first_match_reference on the CPU, which shares no code with either.

Integer paths: results must be EQUAL.
"""
import functools
import random

import pytest
import torch

from tests.test_compact_staging import (BIT63_VOCAB, all_dims_policy, bit63_policy,
                                        catch_all_policy, tenants_only_policy)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INT_MAX = 2 ** 31 - 1

# (J, R): around the 16-job tile, the 2-tile pair a wave holds, the 64-lane
# wave and the 256-thread block; R around the 16-rule tile and one size that
# spreads the rule tiles over several blocks per job tile
SHAPES = [(1, 1), (15, 16), (16, 17), (17, 300), (31, 16), (32, 17), (33, 300),
          (255, 300), (257, 16), (1000, 300)]

# bundle -> (policy builder over R rules, job vocabulary, expected L or None)
BUNDLES = {
    "synthetic": (None, 48, None),
    "all_dims": (all_dims_policy, 48, None),
    "tenants_only": (tenants_only_policy, 48, 1),
    "catch_all": (lambda R: catch_all_policy(R, secrets=True), 48, 0),
    # 64 tenants / requirements / risk tags: ids up to 63, bit 63 of a column
    "bit63": (bit63_policy, BIT63_VOCAB, None),
}


def _inputs(J, vocab, seed):
    """Jobs over every dimension; every 5th job has no field set at all, so
    all of its columns are zero, whatever the live set."""
    from cordum_amd.safety import policy as pol

    rng = random.Random(seed)
    out = []
    for j in range(J):
        if j % 5 == 4:
            out.append(pol.PolicyInput())
            continue
        v = lambda: rng.randrange(vocab)  # noqa: E731
        n_req = rng.choice((0, 0, 1, 2, vocab))  # vocab: every requirement
        out.append(pol.PolicyInput(
            tenant=f"t{v()}" if rng.random() < 0.9 else f"t{vocab - 1}",
            topic=f"job.a{v()}",
            capability=f"cap{v()}", pack_id=f"pack{v()}", actor_id=f"actor{v()}",
            actor_type=f"atype{v()}",
            risk_tags=[f"tag{v()}" for _ in range(rng.choice((0, 1, 2)))],
            requires=([f"req{k}" for k in range(vocab)] if n_req == vocab
                      else [f"req{v()}" for _ in range(n_req)] + [f"req{vocab - 1}"][:n_req]),
            labels={"k": f"v{v()}"} if rng.random() < 0.5 else {},
            secrets_present=(j % 3 == 0)))
    return out


@functools.lru_cache(maxsize=None)
def _case(bundle, J, R):
    """Compiled bundle, jobs, packed policy, live set and the CPU reference:
    computed once per (bundle, shape), shared by both job_tiles, not written."""
    from cordum_amd.ops.pipeline import make_synthetic_policy
    from cordum_amd.ops.policy_compile import JobEncoder, compile_policy, first_match_reference
    from cordum_amd.ops.policy_mfma import gather_live_cols, live_dims, pack_policy_mfma

    build, vocab, want_L = BUNDLES[bundle]
    policy = (make_synthetic_policy(R, deny_frac=0.3, seed=9) if build is None
              else build(R))
    compiled = compile_policy(policy, words=1)
    assert compiled.exact and compiled.n_rules == R
    jobs = JobEncoder(compiled).encode(_inputs(J, vocab, seed=J * 31 + R))
    mp = pack_policy_mfma(compiled)
    live = live_dims(mp)
    if want_L is not None:
        assert len(live) == want_L
    if bundle == "all_dims" and R >= 9:
        assert len(live) == 9
    cols = gather_live_cols(jobs, live)
    ref = first_match_reference(compiled, jobs).to(torch.int32)
    return compiled, jobs, mp, live, cols, ref


def _run_cols(ext, mp_dev, cols, cmap, secrets, J, R, job_tiles):
    out = torch.full((J,), INT_MAX, dtype=torch.int32, device=DEV)
    ext.policy_first_match_mfma_cols_into(
        cols, cmap, mp_dev.b_pack, mp_dev.cards, mp_dev.secrets, secrets,
        mp_dev.tile_dims, R, out, job_tiles)
    torch.cuda.synchronize()
    out = out.cpu()
    return torch.where(out == INT_MAX, torch.full_like(out, -1), out)


@pytest.mark.parametrize("job_tiles", (1, 2))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "J%d-R%d" % s)
@pytest.mark.parametrize("bundle", list(BUNDLES))
def test_k1_from_cols_matches_bits_and_reference(bundle, shape, job_tiles):
    from cordum_amd.ops import get_ext
    from cordum_amd.ops.policy_mfma import col_map

    ext = get_ext(required=True)
    J, R = shape
    compiled, jobs, mp, live, cols, ref = _case(bundle, J, R)
    d = torch.device(DEV)
    mpd = mp.to(d)
    sec = jobs.secrets.to(d)
    got = _run_cols(ext, mpd, cols.to(d), col_map(live), sec, J, R, job_tiles)

    bits = torch.full((J,), INT_MAX, dtype=torch.int32, device=d)
    ext.policy_first_match_mfma_bits_into(
        jobs.any_bits.to(d).contiguous(), jobs.all_bits.to(d).contiguous(),
        mpd.b_pack, mpd.cards, mpd.secrets, sec, mpd.tile_dims, R, bits, job_tiles)
    torch.cuda.synchronize()
    bits = bits.cpu()
    bits = torch.where(bits == INT_MAX, torch.full_like(bits, -1), bits)

    assert torch.equal(got, bits)
    assert torch.equal(got, ref)
    # the all-zero jobs are there, and (J permitting) so are both outcomes
    if live and J >= 5:
        assert bool((cols[4::5] == 0).all())
    if bundle == "bit63":
        assert bool((cols < 0).any()) or J < 15, "no column with bit 63 set"
    if bundle == "catch_all" and J >= 3 and R >= 2:
        assert set(got.tolist()) == {0, 1}


def test_bit63_bundle_uses_bit_63():
    """The vocabulary of 64 fills the word: rule masks and job columns with
    the top bit set, and a job that holds every requirement matches rule 0."""
    compiled, jobs, mp, live, cols, ref = _case("bit63", 257, 16)
    assert int(compiled.any_masks[0, 0, 0]) == -1 and int(compiled.all_masks[0, 0, 0]) == -1
    assert bool((cols < 0).any())
    assert bool((ref == 0).any())


def test_stale_map_raises():
    """A map that lacks a dimension the packed policy scans, one whose column
    count is not the buffer's, and one that is not ascending."""
    from cordum_amd.ops import get_ext
    from cordum_amd.ops.policy_mfma import col_map

    ext = get_ext(required=True)
    J, R = 33, 300
    compiled, jobs, mp, live, cols, ref = _case("synthetic", J, R)
    assert live == [0, 1, 6, 7]
    d = torch.device(DEV)
    mpd = mp.to(d)
    sec = jobs.secrets.to(d)
    with pytest.raises(RuntimeError, match="lacks a dimension"):
        _run_cols(ext, mpd, cols[:, :3].contiguous().to(d), col_map([0, 1, 6]), sec, J, R, 2)
    with pytest.raises(RuntimeError, match="columns"):
        _run_cols(ext, mpd, cols.to(d), col_map([0, 1, 6]), sec, J, R, 2)
    swapped = col_map(live) ^ (0x1 << 0) ^ (0x1 << 4)  # tenant <-> topic columns
    with pytest.raises(RuntimeError, match="ascending"):
        _run_cols(ext, mpd, cols.to(d), swapped, sec, J, R, 2)
    # a superset map is fine: an extra column is staged and never scanned
    wide = sorted(set(live) | {3})
    from cordum_amd.ops.policy_mfma import gather_live_cols

    got = _run_cols(ext, mpd, gather_live_cols(jobs, wide).to(d), col_map(wide), sec, J, R, 2)
    assert torch.equal(got, ref)
