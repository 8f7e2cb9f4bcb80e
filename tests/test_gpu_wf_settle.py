"""GPU tests of the per-step-policy pass (wf_settle): the HIP kernel is called
directly on the hand-built tables of tests/test_wf_settle_cases.py and
compared with what the builder owes and with the oracle, and, at stock
policies, with the HIP kernels of the pair it replaces.

Every output is a pure function of the tables, so every table and both
counters are compared exactly.
"""
import pytest
import torch

from tests import test_wf_settle_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from cordum_amd.ops import get_ext

    return get_ext(required=True)


@pytest.mark.parametrize("NR,pattern", S.CASES)
def test_wf_settle_matches_oracle(ext, NR, pattern):
    t, want = S.settle_oracle(NR, pattern)
    got = S.settle_call(ext, t, "cuda")
    S.assert_exact(t, got)
    for k in S.ARGS:
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("NR,R", S.EQUIV_CASES)
def test_wf_settle_equals_the_stock_pair_at_stock_policies(ext, NR, R):
    t = S.build_equiv_tables(NR, R)
    pair = S.pair_call(ext, t, R, "cuda")
    S.assert_equiv_case_is_the_case(t, pair, NR, R)
    got = S.settle_call(ext, t, "cuda")
    S.assert_settle_equals_pair(got, pair)
    S.assert_settle_equals_pair(got, S.settle_call(S.ref_ops(), t))


def test_wf_settle_rejects_a_misaligned_policy_table(ext):
    """The policy records are read as 16-byte vector loads: a table that does
    not start on a 16-byte boundary is refused by the host binding, not run."""
    t = S.build_tables(65, "edge")
    d = {k: (v.clone().cuda() if torch.is_tensor(v) else v) for k, v in t.items()}
    buf = torch.zeros(d["tmpl_policy"].numel() + 1, dtype=torch.int32, device="cuda")
    d["tmpl_policy"] = buf[1:]
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ext.wf_settle(*[d[a] for a in S.ARGS])
