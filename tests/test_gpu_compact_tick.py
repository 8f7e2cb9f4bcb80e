"""Compact descriptor staging through the pipeline: the fused tick with K1
reading the slot's compact buffer against the full-layout fused tick (GPU)
and the staged tick on the CPU reference backend (no shared code); e2e_run
with compact staging against e2e_run without; and the paths that keep
reading the full-layout tensors after a compact e2e_run.

Shapes, cases, set-up and comparison are those of test_gpu_tick_fusion.py
(imported, not copied). Integer paths: outputs must be EQUAL.
"""
import pytest
import torch

from tests.test_gpu_tick_fusion import DEV, _check_case, _compare, _mutate, _policy, _run

pytestmark = pytest.mark.gpu

SHAPES = [(17, 17, 1025, 65), (257, 16, 1025, 64), (1000, 300, 1025, 65)]
CASES = ["default", "deny_all", "labels"]


def _run_compact(case, shape, ticks=2):
    """_run of test_gpu_tick_fusion.py with the body's compact variant."""
    from cordum_amd.ops.pipeline import DevicePipeline

    B, R, NW, PW = shape
    pipe = DevicePipeline(device=torch.device(DEV), batch_size=B, n_local_workers=NW,
                          n_rules=R, n_batches=1, payload_words=PW, seed=3,
                          policy=_policy(case, R), mfma_pack_on_device=True,
                          compact_staging=True)
    _mutate(pipe, case)
    # K1 must not be able to lean on the full-layout words
    pipe.batches[0].any_bits.fill_(-1)
    pipe.batches[0].all_bits.fill_(-1)
    pipe.batches[0].secrets.fill_(1)
    mid = None
    for t in range(ticks):
        pipe._fused_body(0, compact=True)
        if t == 0:
            torch.cuda.synchronize()
            mid = pipe.w_active_local.cpu().clone()
    torch.cuda.synchronize()
    return pipe, mid


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-R%d-W%d-P%d" % s)
@pytest.mark.parametrize("case", CASES)
def test_compact_tick_equals_full_layout_and_cpu_reference(case, shape):
    new, mid_new = _run_compact(case, shape)
    assert new._compact and new._use_mfma
    full, mid_full = _run(case, shape, unfused=False, compact_staging=False)
    assert full._use_mfma and not full._compact
    _check_case(case, shape, _compare(new, full, mid_new, mid_full), mid_new)
    ref, mid_ref = _run(case, shape, unfused=True, device="cpu", backend="ref")
    _check_case(case, shape, _compare(new, ref, mid_new, mid_ref), mid_new)


def _pipe(B, compact):
    from cordum_amd.ops.pipeline import DevicePipeline

    return DevicePipeline(device=torch.device(DEV), batch_size=B, n_local_workers=64,
                          n_rules=300, n_batches=2, payload_words=17, seed=5,
                          mfma_pack_on_device=True, compact_staging=compact)


@pytest.mark.parametrize("B", (257, 1000))
def test_e2e_run_compact_equals_full_layout(B):
    new, old = _pipe(B, True), _pipe(B, False)
    assert new._compact and not old._compact
    assert len(new._live) == 4
    for call in range(2):  # the second call reuses the host buffers
        a = new.e2e_run(6)
        b = old.e2e_run(6)
        assert a[:2] == b[:2], f"call {call}: (completed, denied)"
        assert a[0] > 0 and a[0] + a[1] <= 6 * B
        assert torch.equal(new._e2e_sums, old._e2e_sums), f"call {call}"
        assert torch.equal(new._e2e_decisions, old._e2e_decisions), f"call {call}"
    # the compact run staged nothing into the full-layout slots
    assert new.compact_bufs[0].numel() < new.batch_bufs[0].numel()


def test_full_layout_paths_intact_after_compact_e2e_run():
    B = 1000
    new = _pipe(B, True)
    new.e2e_run(6)
    # tick(): the full-layout slots still hold the pre-staged batches, which a
    # pipeline that never staged anything decides the same way (the payload
    # slots were restaged, so checksums are not compared here)
    fresh = _pipe(B, False)
    new._tick = 0
    for slot in range(2):
        a, b = new.tick(), fresh.tick()
        assert (a.completed, a.denied, a.unrouted) == (b.completed, b.denied, b.unrouted)
        assert torch.equal(new.out_decision.cpu(), fresh.out_decision.cpu()), slot
    # tick_e2e(): fresh encode into full-layout slot 0, against a pipeline
    # with the same history on the full-layout path
    old = _pipe(B, False)
    old.e2e_run(6)
    for _ in range(2):
        a, b = new.tick_e2e(), old.tick_e2e()
        assert (a.completed, a.denied, a.unrouted) == (b.completed, b.denied, b.unrouted)
        assert torch.equal(new._e2e_sums, old._e2e_sums)
        assert torch.equal(new._e2e_decisions, old._e2e_decisions)
    # and tick() on what tick_e2e just staged, same slot on both
    new._tick = old._tick = 0
    a, b = new.tick(), old.tick()
    assert (a.completed, a.denied, a.unrouted) == (b.completed, b.denied, b.unrouted)
    for name in ("res_sums", "out_decision", "states"):
        assert torch.equal(getattr(new, name).cpu(), getattr(old, name).cpu()), name
