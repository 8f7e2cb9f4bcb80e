"""The staged (one op per stage) tick on the CPU reference backend.

tests/test_gpu_tick_fusion.py holds the fused GPU tick to this pipeline, so
this pipeline is held here to the properties of a tick, on its own and
without a GPU.
"""
import pytest
import torch

from cordum_amd.ops.pipeline import (ALLOW_CODES, DENIED, SUCCEEDED, DevicePipeline,
                                     make_synthetic_policy)
from cordum_amd.ops.policy_compile import first_match_reference

NO_DEADLINE = torch.iinfo(torch.int64).max
SOME_DEADLINE = 123456789

# (B, rules, workers, payload words): the smallest tick, odd sizes on every
# axis with more workers than jobs, and more jobs than one block's threads
SHAPES = [(1, 1, 1, 1), (17, 17, 1025, 65), (257, 16, 1025, 64)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-R%d-W%d-P%d" % s)
def test_reference_staged_tick(shape):
    B, R, NW, PW = shape
    pipe = DevicePipeline(device="cpu", backend="ref", unfused_tick=True, batch_size=B,
                          n_local_workers=NW, n_rules=R, n_batches=1, payload_words=PW,
                          seed=3, policy=make_synthetic_policy(R, deny_frac=0.3, seed=3))
    pipe.deadlines.fill_(SOME_DEADLINE)
    pipe._fused_body(0)

    # decisions: first matching rule's, default allow
    first = first_match_reference(pipe.compiled, pipe.batches[0]).long()
    want = torch.where(first >= 0, pipe.compiled.decisions.long()[first.clamp(min=0)],
                       torch.ones_like(first))
    assert torch.equal(pipe.out_decision.long(), want)
    allowed = (want == ALLOW_CODES[0]) | (want == ALLOW_CODES[1])

    n_den, n_all, n_rt = pipe._counts[:3].tolist()
    assert n_den + n_all == B
    assert n_all == int(allowed.sum())
    assert n_rt <= n_all
    assert torch.equal(torch.sort(pipe.allowed_slots[:n_all]).values.long(),
                       torch.nonzero(allowed).flatten())
    denied = torch.nonzero(~allowed).flatten()
    assert torch.equal(torch.sort(pipe.denied_slots[:n_den]).values.long(), denied)

    # routed slots: SUCCEEDED through the whole chain, scheduled exactly once
    routed = pipe.routable_slots[:n_rt].long()
    assert routed.unique().numel() == n_rt and bool(allowed[routed].all())
    assert bool((pipe.states[routed] == SUCCEEDED).all())
    assert bool((pipe.attempts[routed] == 1).all())
    assert bool((pipe.deadlines[routed] == NO_DEADLINE).all())
    payload = pipe.payloads[0].view(B, PW)
    assert torch.equal(pipe.res_arena[: B * PW].view(B, PW)[routed], payload[routed])

    # denied slots: DENIED, deadline cleared, in the DLQ ring
    assert bool((pipe.states[denied] == DENIED).all())
    assert bool((pipe.deadlines[denied] == NO_DEADLINE).all())
    assert bool((pipe.attempts[denied] == 0).all())
    assert int(pipe.dlq_head[0]) == n_den
    assert torch.equal(torch.sort(pipe.dlq_ring[:n_den]).values.long(), denied)

    # everything else was left alone; the load histogram counts the routed
    rest = torch.ones(B, dtype=torch.bool)
    rest[routed] = False
    rest[denied] = False
    assert bool((pipe.deadlines[rest] == SOME_DEADLINE).all())
    assert int(pipe.w_active_local.sum()) == n_rt
    assert bool((pipe.w_active_local >= 0).all())
