"""CPU check of the inputs of tests/test_gpu_wf_admission.py.

Each table builder of the GPU module is run through its oracle here and the
"the case is the case" assertions are made on the oracle's output: the
overflow cases overflow, the quiescent-by-staleness row really has children
out, the stale-generation cancel really names a LIVE slot. The inputs of the
GPU tests are thereby verified on a machine without a GPU, and the oracles
of the three lifecycle kernels are checked against statements of the
contract that do not share their code.
"""
import pytest
import torch

from cordum_amd.ops import reference as ref
from tests import test_gpu_wf_admission as A


@pytest.mark.parametrize("NR,free_mode,n_mode", A.ADMIT_CASES)
def test_admit_tables_hold_their_cases(NR, free_mode, n_mode):
    t, want = A.oracle("wf_admit", A.build_admit_tables, NR, free_mode, n_mode)
    A.assert_admit_case(t, want)
    F, n = len(t["free"]), int(t["req_tmpl"].shape[0])
    assert F == int((t["run_life"] == ref.WFL_FREE).sum())
    assert n == {"zero": 0, "one": 1, "F": F, "F+1": F + 1, "over_NR": NR + 3}[n_mode]
    if n_mode in ("F+1", "over_NR"):          # the overflow case overflows
        assert n > F and int(want["out_slot"][-1]) == -1
    if n_mode == "over_NR":
        assert n > NR
    if free_mode == "none":
        assert F == 0 and want["out_slot"].tolist() == [-1]
    if free_mode == "all":
        assert F == NR and want["out_slot"][:NR].tolist() == list(range(NR))
    if free_mode == "last":
        assert want["out_slot"].tolist() == [NR - 1, -1]
    if free_mode == "third_block_first":
        assert t["free"] == [512] and int(want["out_slot"][0]) == 512
    if free_mode == "alternating":
        assert t["free"] == list(range(0, NR, 2))
    if n:                                      # bit 63 of cond_bits survives
        assert int(t["req_cond"][0]) < 0
        if F:
            assert int(want["cond_bits"][t["free"][0]]) == int(t["req_cond"][0])
    # the workspaces are the kernel's own: the oracle leaves them alone
    assert bool((want["free_mask"] == A.POISON).all())


def test_admit_requests_cover_the_template_cases():
    t, want = A.oracle("wf_admit", A.build_admit_tables, 65, "all", "F+1")
    ns = t["tmpl_nsteps"].tolist()
    assert ns[0] == 64 and ns[1] == 1
    kind0 = t["tmpl_kind"][:64]
    assert A.REQ_FANOUT[0] > 0                 # override on a 64-step template
    assert bool((kind0 == ref.WFK_FOR_EACH).any()) and bool((kind0 == ref.WFK_WORKER).any())
    # ... taken on its FOR_EACH steps, ignored on the others
    row = want["children_todo"].view(-1, 64)[0]
    assert bool((row[kind0 == ref.WFK_FOR_EACH] == A.REQ_FANOUT[0]).all())
    assert torch.equal(row[kind0 != ref.WFK_FOR_EACH],
                       t["tmpl_todo"][:64][kind0 != ref.WFK_FOR_EACH])
    # the one-step WORKER template ignores its override
    assert A.REQ_FANOUT[1] > 0 and int(t["tmpl_kind"][64]) == ref.WFK_WORKER
    assert want["children_todo"].view(-1, 64)[1].tolist() == [1] + [0] * 63
    # no override: the template's own fan-out
    assert A.REQ_FANOUT[3] == 0 and int(t["tmpl_kind"][3 * 64]) == ref.WFK_FOR_EACH
    assert int(want["children_todo"][3 * 64]) == int(t["tmpl_todo"][3 * 64])
    # template entries past n_steps are garbage the kernel must not copy
    assert bool(t["tmpl_todo"][64 + 1:128].all())
    assert int(want["admit_count"][0]) == A.BIG + 65


@pytest.mark.parametrize("NR", A.SIZES)
def test_cancel_tables_hold_their_cases(NR):
    t, want = A.oracle("wf_cancel", A.build_cancel_tables, NR)
    A.assert_cancel_case(t, want)
    assert len(t["roles"]) == min(NR, len(A.CANCEL_ROLES))
    if NR >= 63:   # effective and ineffective requests among the random rows too
        ok = want["out_ok"].tolist()
        assert ok.count(1) > 2 and ok.count(0) > 4
        assert -1 in t["req_slot"].tolist()


@pytest.mark.parametrize("NR", A.SIZES)
def test_retire_tables_hold_their_cases(NR):
    t, want = A.oracle("wf_retire", A.build_retire_tables, NR)
    A.assert_retire_case(t, want)
    assert len(t["roles"]) == min(NR, len(A.RETIRE_ROLES))
    if NR >= 63:
        r = t["roles"]["draining_step63_blocks"]
        assert int(t["n_steps"][r]) == 64 and int(t["children_out"][r * 64 + 63]) > 0
        assert not bool(t["children_out"].view(-1, 64)[r, :63].any())
        r = t["roles"]["terminal_block_past_n_steps"]
        ns = int(t["n_steps"][r])
        assert int(t["children_out"][r * 64 + ns]) > 0
        assert int(t["dispatch_tick"][r * 64 + ns]) > A.RETIRE_TICK - A.RETIRE_CUTOFF
        # the random rows: DRAINING ones both freed and kept
        dr = t["run_life"] == ref.WFL_DRAINING
        assert bool((want["run_life"][dr] == ref.WFL_FREE).any())
        assert bool((want["run_life"][dr] == ref.WFL_DRAINING).any())


@pytest.mark.parametrize("NR", (1, 65, 257))
def test_tick_oracles_leave_cancelled_steps_alone(NR):
    from tests import test_gpu_wf_kernels as K

    A.assert_tick_kernels_write_nothing(A.ref_ops(), NR)
    # the case is the case: with the cancelled steps open again, each of
    # the four kernels does act on this table
    t = A.build_cancelled_tables(NR)
    for kernel, state in (("wf_sweep", ref.WFS_PENDING), ("wf_commit", ref.WFS_DISPATCHED),
                          ("wf_timeout_scan", ref.WFS_DISPATCHED),
                          ("wf_status", ref.WFS_FAILED)):
        u = dict(t)
        u["step_state"] = torch.where(t["step_state"] == ref.WFS_CANCELLED,
                                      torch.tensor(state, dtype=torch.uint8), t["step_state"])
        out = K.call(A.ref_ops(), kernel, u)
        assert any(torch.is_tensor(v) and not torch.equal(out[k], v) for k, v in u.items()), kernel
