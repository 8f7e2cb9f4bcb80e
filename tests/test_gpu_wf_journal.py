"""GPU tests of the step-transition journal kernel (wf_journal): the HIP
kernel is called directly on the hand-built tables of
tests/test_wf_journal_cases.py and compared with its oracle.

Without overflow the event list is compared as a sorted set (the kernel
appends per wave, in no defined order) and the shadows and the count exactly.
Under a full list, which changes fit is undefined on the GPU: the emitted set
must be a subset of the planted changes of the oracle's size, the shadow
advanced exactly for that set, and a second pass must complete it.
"""
import pytest
import torch

from tests import test_wf_journal_cases as J

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from cordum_amd.ops import get_ext

    return get_ext(required=True)


@pytest.mark.parametrize("NR,pattern,cap_mode", J.CASES)
def test_wf_journal_matches_oracle(ext, NR, pattern, cap_mode):
    t, want = J.oracle(NR, pattern, cap_mode)
    got = J.call(ext, t, "cuda")
    seen = J.assert_pass_is_sound(t, got)
    overflow = len(t["changes"]) > max(0, t["cap"] - t["preload"])
    if not overflow:
        assert sorted(J.emitted_records(t, got)) == sorted(J.emitted_records(t, want))
        for k in ("ev_shadow_state", "ev_shadow_gen", "ev_count"):
            assert torch.equal(got[k], want[k]), k
    else:
        assert len(seen) == len(J.emitted_records(t, want))
        assert seen <= set(t["changes"])
    J.assert_second_pass_completes(ext, t, got, "cuda")


def test_wf_journal_rejects_a_misaligned_record_list(ext):
    """The records are written as 16-byte vector stores: a list that does not
    start on a 16-byte boundary is refused by the host binding, not run."""
    t = dict(J.build_journal_tables(17, "all", "ample"))
    d = {k: (v.clone().cuda() if torch.is_tensor(v) else v) for k, v in t.items()}
    buf = torch.zeros(d["ev_rec"].numel() + 1, dtype=torch.int32, device="cuda")
    d["ev_rec"] = buf[1:]
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ext.wf_journal(*[d[a] for a in J.ARGS])
