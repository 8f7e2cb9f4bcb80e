"""GPU tests of the approval-hold kernels (wf_hold_scan, wf_hold_list,
wf_decide): the HIP kernels are called directly on the hand-built tables of
tests/test_wf_hold_cases.py and compared with their oracles.

Every output is a pure function of the tables, so every table, counter and
list is compared exactly; the list's records are compared in list order, with
no sorting.
"""
import pytest
import torch

from tests import test_wf_hold_cases as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from cordum_amd.ops import get_ext

    return get_ext(required=True)


@pytest.mark.parametrize("NR,pattern", H.SCAN_CASES)
def test_wf_hold_scan_matches_oracle(ext, NR, pattern):
    t, want = H.scan_oracle(NR, pattern)
    got = H.scan_call(ext, t, "cuda")
    H.assert_scan_is_exact(t, got)
    for k in H.SCAN_TABLES:
        assert torch.equal(got[k], want[k]), k
    H.assert_second_scan_only_expires(ext, t, got, "cuda")


@pytest.mark.parametrize("NR,cap_mode,cursor_mode", H.LIST_CASES)
def test_wf_hold_list_matches_oracle(ext, NR, cap_mode, cursor_mode):
    t, want = H.list_oracle(NR, cap_mode, cursor_mode)
    got = H.list_call(ext, t, "cuda")
    H.assert_list_is_exact(t, got)
    assert torch.equal(got["list"], want["list"])      # bit for bit


@pytest.mark.parametrize("NR", H.LIST_SIZES)
def test_wf_hold_list_pages_reassemble_to_the_planted_set(ext, NR):
    t = H.build_list_tables(NR)
    for cap in (1, 7) if NR <= 65 else (64,):
        got, pages = H.page_all(ext, t, cap, "cuda")
        assert got == t["planted"]
        assert pages == max(1, -(-len(got) // cap))


def test_wf_hold_list_rejects_a_misaligned_list(ext):
    """The records are written as 16-byte vector stores: a list that does not
    start on a 16-byte boundary is refused by the host binding, not run."""
    t = H.build_list_tables(65)
    d = {k: (v.clone().cuda() if torch.is_tensor(v) else v) for k, v in t.items()}
    buf = torch.zeros(d["list"].numel() + 1, dtype=torch.int32, device="cuda")
    d["list"] = buf[1:]
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ext.wf_hold_list(*[d[a] for a in H.LIST_ARGS])


@pytest.mark.parametrize("n", H.DECIDE_COUNTS)
def test_wf_decide_matches_oracle(ext, n):
    t, want = H.decide_oracle(n)
    got = H.decide_call(ext, t, "cuda")
    H.assert_decide_is_exact(t, got)
    for k in ("out_code", "step_state", "hold_counts"):
        assert torch.equal(got[k], want[k]), k


def test_wf_decide_every_role_and_two_steps_of_one_run(ext):
    t, want = H.decide_oracle(len(H.ROLES), True)
    got = H.decide_call(ext, t, "cuda")
    H.assert_decide_is_exact(t, got)
    assert torch.equal(got["out_code"], want["out_code"])
