"""CPU check of the inputs of tests/test_gpu_wf_kernels.py.

Each table builder of the GPU module is run through its oracle here and the
"the case is the case" assertions are made on the oracle's output: every
step kind fires, step 63 is ready, the overflow cases overflow, all three
wf_apply outcomes occur, every wf_commit branch is taken. The inputs of the
GPU tests are thereby verified on a machine without a GPU, and an edit to a
builder cannot quietly empty a GPU test.
"""
import pytest
import torch

from cordum_amd.ops import reference as ref
from tests import test_gpu_wf_kernels as K


@pytest.mark.parametrize("NR", K.SIZES)
def test_sweep_tables_hold_their_cases(NR):
    t, out, out2 = K.sweep_oracle(NR)
    K.assert_sweep_case(t, out, out2)
    # step 63 is dispatched, held for approval and resolved somewhere
    disp, appr = K.sweep_lists(out)
    if NR >= 63:
        assert any(s == 63 for _, s in disp) and any(s == 63 for _, s in appr)
        assert bool((t["run_active"] == 0).any())
        assert {0, 1, 2} <= set((t["next_ready"] - t["tick"] + 1).tolist())
    # ample caps: nothing was cut, nothing written past the counters
    assert len(disp) == int(out["disp_count"][0]) and len(appr) == int(out["appr_count"][0])
    assert bool((out["disp_runs"][len(disp):] == K.POISON).all())


@pytest.mark.parametrize("NR", K.SIZES)
def test_readiness_tables_hold_their_cases(NR):
    t, ready, pairs = K.readiness_oracle(NR)
    K.assert_readiness_case(t, ready, pairs)
    assert len(pairs) == len(set(pairs))
    if NR >= 63:  # a dependency mask that uses bit 62
        assert bool(((t["deps_mask"] >> 62) & 1).bool().any())


@pytest.mark.parametrize("NR,cap,acap", [(65, 1, 1), (257, 63, 7), (513, 300, 65)])
def test_sweep_overflow_overflows(NR, cap, acap):
    t, out, _ = K.sweep_oracle(NR, cap, acap)
    _, full, _ = K.sweep_oracle(NR)
    full_disp, full_appr = K.sweep_lists(full)
    disp, appr = K.sweep_lists(out)
    K.assert_capped_prefix(disp, int(out["disp_count"][0]), cap, full_disp)
    K.assert_capped_prefix(appr, int(out["appr_count"][0]), acap, full_appr)
    assert torch.equal(out["step_state"], full["step_state"])


@pytest.mark.parametrize("NR,cap", [(65, 1), (257, 64), (513, 1000)])
def test_readiness_overflow_overflows(NR, cap):
    _, _, pairs = K.readiness_oracle(NR)
    assert len(pairs) > cap


@pytest.mark.parametrize("N,cap", [(257, 1), (257, 64), (1000, 65)])
def test_deadline_overflow_overflows(N, cap):
    t = K.build_deadline_tables(N)
    assert t["want"].numel() > cap + 1 and 0 not in t["want"].tolist()


@pytest.mark.parametrize("valid_count", [0, 1, 7, 1024, 1500])
@pytest.mark.parametrize("n_entries", [1, 3, 4, 5, 9])
def test_expand_tables_fit_and_spread(n_entries, valid_count):
    t = K.build_expand_tables(K.std_entries(n_entries), valid_count=valid_count)
    want = K.call(K.ref_ops(), "wf_expand", t)
    seen = K.assert_expand_matches(t, want, want)
    assert len(seen) == n_entries
    assert K.ORDER_LEN == 1500 and t["order"].unique().numel() > 1024
    # cell 0 is no entry: the unused list slots may name it
    assert all(e[0] * 64 + e[1] != 0 for e in t["entries"])


def test_expand_window_cases():
    t = K.build_expand_tables(list(K.MAXP_ENTRIES))
    want = K.call(K.ref_ops(), "wf_expand", t)
    seen = K.assert_expand_matches(t, want, want)
    got = [seen.get(e[0] * 64 + e[1], 0) for e in K.MAXP_ENTRIES]
    assert got == [15, 0, 10, 0, 0, 4]
    assert got == [K.expand_window(e[2], e[3], e[4]) for e in K.MAXP_ENTRIES]
    # smaller than todo, equal to children_out, and maxp == 0
    assert any(0 < e[4] - e[3] < e[2] for e in K.MAXP_ENTRIES)
    assert any(e[4] > 0 and e[4] == e[3] for e in K.MAXP_ENTRIES)
    assert any(e[4] == 0 and e[2] > 0 for e in K.MAXP_ENTRIES)


@pytest.mark.parametrize("name", list(K.ARENA_SINGLE))
def test_expand_arena_single_cases(name):
    t = K.build_arena_single(name)
    todo, c0, fits = K.ARENA_SINGLE[name]
    want = K.call(K.ref_ops(), "wf_expand", t)
    seen = K.assert_expand_all_or_nothing(t, want)
    assert (list(seen.values()) == [todo]) if fits else (not seen)
    assert (c0 + todo == K.ARENA_CB) if fits else (c0 + todo == K.ARENA_CB + 1)
    if not fits:
        K.assert_tables_equal(want, t, skip=("entries",))


@pytest.mark.parametrize("name", list(K.ARENA_MANY))
def test_expand_arena_many_cases(name):
    t = K.build_arena_many(name)
    CB, todos = K.ARENA_MANY[name]
    want = K.call(K.ref_ops(), "wf_expand", t)
    seen = K.assert_expand_all_or_nothing(t, want)
    assert sum(todos) > CB and 1 <= len(seen) < len(todos)
    if name.startswith("oversized"):
        assert todos[0] > CB and max(todos[1:]) <= CB
        assert t["entries"][0][0] * 64 + t["entries"][0][1] not in seen


@pytest.mark.parametrize("ppt_idx", range(4))
@pytest.mark.parametrize("one_tag", [True, False])
@pytest.mark.parametrize("cap", [1, 63, 65, 300])
@pytest.mark.parametrize("world", [1, 4])
def test_apply_tables_hold_their_cases(world, cap, one_tag, ppt_idx):
    t, want = K.oracle("wf_apply", K.build_apply_tables, world, cap, one_tag, ppt_idx)
    K.assert_apply_case(t)
    drop, fail, done, _ = K.apply_outcomes(t)
    assert int((want["children_fail"] - t["children_fail"]).sum()) == fail
    assert int((want["children_done"] - t["children_done"]).sum()) == done
    assert int((t["children_out"] - want["children_out"]).sum()) == fail + done
    if one_tag:
        assert int((want["children_out"] != t["children_out"]).sum()) <= 1
    if world == 4 and cap >= 63 and K.APPLY_PPT[ppt_idx] == (150, 100):
        assert drop and fail and done  # all three outcomes occur


def test_apply_send_counts_cover_every_mode():
    for cap in (1, 63, 65, 300):
        modes = {0, cap // 2, cap, cap + 7}
        assert {K.apply_send_counts(1, cap, i)[0] for i in range(4)} == modes
        for i in range(4):
            assert set(K.apply_send_counts(4, cap, i)) == modes


@pytest.mark.parametrize("count_mode", K.DEAD_COUNTS)
@pytest.mark.parametrize("dcap", [1, 63, 65, 300])
def test_apply_dead_tables_hold_their_cases(dcap, count_mode):
    t, want = K.oracle("wf_apply_dead", K.build_apply_dead_tables, dcap, False, count_mode)
    n = min(int(t["dead_count"][0]), dcap)
    assert (int(t["dead_count"][0]) > dcap) == (count_mode == "above")
    assert (n == 0) == (count_mode == "zero")
    assert int((want["children_fail"] - t["children_fail"]).sum()) == n
    if dcap >= 63 and n:
        assert bool((t["dead_src"][:n] < 0).any()) and bool((t["dead_src"][:n] >= 0).any())


@pytest.mark.parametrize("NR", [1, 63, 65, 257])
def test_timeout_tables_hold_their_cases(NR):
    t, want = K.oracle("wf_timeout_scan", K.build_timeout_tables, NR)
    K.assert_timeout_case(t, want)


@pytest.mark.parametrize("NR", [1, 65, 257])
def test_commit_tables_take_every_branch(NR):
    t, want = K.oracle("wf_commit", K.build_commit_tables, NR)
    K.assert_commit_case(t, want)
    for a in K.BACKOFF_ATTEMPTS:
        assert f"retry_{a}" in K.COMMIT_BRANCHES and a < K.COMMIT_MAX_RETRIES
    # the backoff on both sides of its cap of 16
    backoff = set((want["next_ready"] - K.COMMIT_TICK).tolist())
    assert {2, 16} <= backoff and max(backoff) == 16


@pytest.mark.parametrize("NR", K.SIZES)
def test_status_tables_hold_their_cases(NR):
    t, want = K.oracle("wf_status", K.build_status_tables, NR)
    K.assert_status_case(t, want)


@pytest.mark.parametrize("n_grants", K.GRANT_NS)
def test_grant_tables_hold_their_cases(n_grants):
    t, want = K.oracle("wf_grant", K.build_grant_tables, n_grants)
    K.assert_grant_case(t, want)


@pytest.mark.parametrize("filter_state", [ref.WFS_SUCCEEDED, ref.WFS_FAILED])
@pytest.mark.parametrize("NR", K.SIZES)
def test_readmit_tables_hold_their_cases(NR, filter_state):
    t, want = K.oracle("wf_readmit", K.build_readmit_tables, NR, filter_state)
    K.assert_readmit_case(t, want)
    if NR > 1:  # runs of 1 and of 64 steps are re-admitted
        for r, ns in ((NR - 1, 1), (NR - 2, 64)):
            assert int(t["n_steps"][r]) == ns and int(want["run_active"][r]) == 1
