"""ext.synthetic_fresh_stamped (one-call host batch preparation: blocked,
ISA-dispatched, optionally split over two threads) against its oracle
ext.synthetic_fresh: the four synthetic dims must be bit-identical, payload
word 0 of every row must carry the step, and nothing else may change.

The stand-alone program tests/native/encode_check.cpp covers the same header
under AddressSanitizer/UBSan; it is compiled and run here when g++ is there.
"""
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from cordum_amd.ops import get_ext

BS = (1, 63, 64, 65, 1000, 4113)
WS = (1, 2)
STEPS = (0, 7, 2 ** 32 + 3)
V = 48
PW = 5  # payload words per row (odd, > 1 so "no other word changes" bites)
DIMS = (0, 1, 3, 0)  # tenant, topic, risk dims of any_bits; requires dim of all_bits


def _ext():
    ext = get_ext(required=False)
    if ext is None or not hasattr(ext, "synthetic_fresh_stamped"):
        pytest.skip("HIP extension with synthetic_fresh_stamped not built")
    return ext


def _luts(W, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(-(1 << 62), 1 << 62, (V, W), dtype=torch.int64, generator=g)
            for _ in range(4)]


def _batch(B, W, fill):
    return (torch.full((B, 7, W), fill, dtype=torch.int64),
            torch.full((B, 2, W), fill, dtype=torch.int64))


def _low32(step):
    v = step & 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("B", BS)
def test_stamped_matches_synthetic_fresh(B, W):
    ext = _ext()
    luts = _luts(W)
    g = torch.Generator().manual_seed(B * 7 + W)
    payload0 = torch.randint(-(1 << 31), (1 << 31) - 1, (B * PW,), dtype=torch.int32,
                             generator=g)
    levels = sorted({0, ext.encoder_isa_level()})
    for step in STEPS:
        # untouched dims keep a sentinel in both paths
        ref_any, ref_all = _batch(B, W, 0x5A5A)
        ext.synthetic_fresh(ref_any, ref_all, *luts, 11, step, *DIMS)
        for threads in (1, 2):
            for isa in levels:
                any_b, all_b = _batch(B, W, 0x5A5A)
                payload = payload0.clone()
                ext.synthetic_fresh_stamped(any_b, all_b, *luts, 11, step, *DIMS,
                                            payload, PW, threads, isa)
                tag = f"B={B} W={W} step={step} threads={threads} isa={isa}"
                assert torch.equal(any_b, ref_any), tag
                assert torch.equal(all_b, ref_all), tag
                rows = payload.view(B, PW)
                assert bool((rows[:, 0] == _low32(step)).all()), tag
                assert torch.equal(rows[:, 1:], payload0.view(B, PW)[:, 1:]), tag


def test_stamp_is_optional_and_single_word_rows():
    ext = _ext()
    luts = _luts(1)
    ref_any, ref_all = _batch(65, 1, 0)
    ext.synthetic_fresh(ref_any, ref_all, *luts, 5, 9, *DIMS)
    any_b, all_b = _batch(65, 1, 0)
    ext.synthetic_fresh_stamped(any_b, all_b, *luts, 5, 9, *DIMS, None, 0, 2, -1)
    assert torch.equal(any_b, ref_any) and torch.equal(all_b, ref_all)
    payload = torch.full((65,), -1, dtype=torch.int32)  # rows of one word
    ext.synthetic_fresh_stamped(any_b, all_b, *luts, 5, 9, *DIMS, payload, 1, 2, -1)
    assert bool((payload == 9).all())


def test_pipeline_encoder_wrapper_matches_fresh_fast():
    """SyntheticEncoder.fresh_stamped on real LUTs == fresh_fast + torch stamp."""
    ext = _ext()
    from cordum_amd.ops.pipeline import (SyntheticEncoder, alloc_batch_staging,
                                         make_synthetic_policy)
    from cordum_amd.ops.policy_compile import compile_policy

    compiled = compile_policy(make_synthetic_policy(64, seed=7), words=1)
    enc = SyntheticEncoder(compiled, seed=101)
    B = 257
    a, _ = alloc_batch_staging(B, compiled.words)
    b, _ = alloc_batch_staging(B, compiled.words)
    pa = torch.arange(B * 64, dtype=torch.int32)
    pb = pa.clone()
    enc.fresh_fast(a, 12, ext)
    pa.view(B, 64)[:, 0] = 12
    enc.fresh_stamped(b, 12, ext, pb, 64)
    assert torch.equal(a.any_bits, b.any_bits) and torch.equal(a.all_bits, b.all_bits)
    assert torch.equal(pa, pb)


def test_standalone_sanitized_program(tmp_path):
    """The torch-free header under ASan+UBSan, as a program of its own."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    root = Path(__file__).resolve().parent.parent
    src = root / "tests" / "native" / "encode_check.cpp"
    exe = tmp_path / "encode_check"
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
    assert "encode_check ok" in run.stdout
