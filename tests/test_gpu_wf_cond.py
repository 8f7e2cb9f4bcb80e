"""GPU tests of the kernels of device-decided conditions: the HIP kernels
wf_cond_eval, wf_child_payload and wf_apply_out are called directly on the
hand-built tables of tests/test_wf_cond_cases.py and compared with what the
builder owes and with the oracle.

Every output is a pure function of the tables, so every table and both
counters are compared exactly.
"""
import pytest
import torch

from tests import test_wf_cond_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from cordum_amd.ops import get_ext

    return get_ext(required=True)


@pytest.mark.parametrize("NR", C.SIZES)
def test_wf_cond_eval_matches_oracle(ext, NR):
    t = C.cond_tables(NR)
    got = C.cond_call(ext, t, "cuda")
    C.assert_cond_exact(t, got)
    want = C.cond_call(C.ref_ops(), t)
    for k in C.COND_ARGS[:-1]:
        assert torch.equal(got[k], want[k]), k


def test_wf_cond_eval_quiet_table_writes_nothing(ext):
    t = dict(C.cond_tables(65))
    t["step_state"] = torch.where(t["step_state"] == C.WFS_PENDING,
                                  torch.tensor(C.WFS_SUCCEEDED, dtype=torch.uint8),
                                  t["step_state"])
    got = C.cond_call(ext, t, "cuda")
    for k in C.COND_ARGS[:-1]:
        assert torch.equal(got[k], t[k]), k


def test_wf_cond_eval_rejects_a_misaligned_predicate_table(ext):
    """The predicate records are read as 16-byte vector loads: a table that
    does not start on a 16-byte boundary is refused by the host binding, not
    run."""
    t = C.cond_tables(65)
    d = {k: (v.clone().cuda() if torch.is_tensor(v) else v) for k, v in t.items()}
    buf = torch.zeros(d["tmpl_cond"].numel() + 1, dtype=torch.int32, device="cuda")
    d["tmpl_cond"] = buf[1:]
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ext.wf_cond_eval(*[d[a] for a in C.COND_ARGS])


@pytest.mark.parametrize("count,CB,iw,w", C.PAYLOAD_CASES)
def test_wf_child_payload_matches_oracle(ext, count, CB, iw, w):
    t = C.build_payload_tables(count, CB, iw, w)
    got = C.payload_call(ext, t, "cuda")
    C.assert_payload_exact(t, got)
    assert torch.equal(got["child_payload"],
                       C.payload_call(C.ref_ops(), t)["child_payload"])


@pytest.mark.parametrize("cap,world,fail_ppt,drop_ppt", C.APPLY_CASES)
def test_wf_apply_out_matches_oracle_and_wf_apply(ext, cap, world, fail_ppt, drop_ppt):
    t = C.build_apply_tables(cap, world, fail_ppt, drop_ppt)
    got = C.apply_out_call(ext, t, "cuda")
    C.assert_apply_out_exact(t, got)
    want = C.apply_out_call(C.ref_ops(), t)
    for k in ("children_done", "children_fail", "children_out", "step_out"):
        assert torch.equal(got[k], want[k]), k
    # the counters it shares with wf_apply: the HIP wf_apply on the same input
    C.assert_apply_counters_equal(got, C.apply_call(ext, t, "cuda"))
