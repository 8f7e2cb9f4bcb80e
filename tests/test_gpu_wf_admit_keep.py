"""GPU tests of wf_admit_keep, the admission with kept steps: the extension
is called directly on every table set of tests/test_wf_admit_keep_cases.py
and compared with the oracle (reference.wf_admit_keep_ref) by exact equality
on all tables, the kernel's workspaces excluded.

The binding's argument checks follow: the valid 17-row tables with one thing
broken must be refused with the matching message before anything is launched.
"""
import pytest
import torch

from tests import test_wf_admit_keep_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from cordum_amd.ops import get_ext

    return get_ext(required=True)


@pytest.mark.parametrize("NR,free_mode,n_mode,pattern", K.CASES)
def test_wf_admit_keep_matches_oracle(ext, NR, free_mode, n_mode, pattern):
    t, want = K.oracle(NR, free_mode, n_mode, pattern)
    got = K.call(ext, "wf_admit_keep", t, "cuda")
    K.A.assert_tables_equal(got, want, skip=K.WORKSPACES + K.NOT_TABLES)


@pytest.mark.parametrize("NR", (65, 513))
def test_nothing_kept_is_wf_admit(ext, NR):
    """The two kernels share the row writer: with no step kept the extension's
    two bindings write the same tables."""
    t, _ = K.oracle(NR, "random", "F+1", "zero")
    got = K.call(ext, "wf_admit_keep", t, "cuda")
    plain = K.call(ext, "wf_admit", t, "cuda")
    K.A.assert_tables_equal(got, plain, skip=K.WORKSPACES + K.NOT_TABLES)


# ---------------------------------------------------------------------------
# the binding's argument checks
# ---------------------------------------------------------------------------
NR = 17
# how -> (the tables it is applied to, the message)
BREAKS = {
    "step_short": (("step_state",), "table sizes disagree"),
    "run_short": (("run_life", "run_gen"), "table sizes disagree"),
    "req_short": (("req_cond", "req_fanout", "out_slot", "out_gen", "req_keep",
                   "req_skip"), "shorter than the request count"),
    "strided": (("req_keep", "req_skip"), "must be contiguous"),
    "int32": (("req_keep", "req_skip"), "must be int64"),
    "workspace": (("free_mask", "blk_scan"), "workspace too small"),
    "tmpl_short": (("tmpl_deps",), "template sizes disagree"),
}


def _device_tables():
    t = K.build_keep_tables(NR, "random", "F", "mixed")
    assert int(t["req_tmpl"].shape[0]) >= 3
    return {k: (t[k].clone().cuda() if torch.is_tensor(t[k]) else t[k]) for k in K.ARGS}


def _strided(v):
    buf = torch.zeros(2 * v.numel(), dtype=v.dtype, device=v.device)
    view = buf[::2]
    view.copy_(v)
    assert view.numel() == v.numel() and not view.is_contiguous()
    return view


def test_binding_accepts_the_valid_tables(ext):
    d = _device_tables()
    ext.wf_admit_keep(*[d[a] for a in K.ARGS])
    torch.cuda.synchronize()
    assert -2 in d["out_slot"].tolist()


@pytest.mark.parametrize("how,table", [(h, k) for h, (ks, _) in BREAKS.items() for k in ks])
def test_binding_rejects_one_broken_table(ext, how, table):
    d = _device_tables()
    v = d[table]
    if how == "step_short":
        d[table] = v[:-64]
    elif how in ("run_short", "req_short", "workspace", "tmpl_short"):
        d[table] = v[:-1]
    elif how == "int32":
        d[table] = v.to(torch.int32)
    else:
        d[table] = _strided(v)
    before = {k: x.clone() for k, x in d.items() if torch.is_tensor(x)}
    with pytest.raises(RuntimeError, match=BREAKS[how][1]) as err:
        ext.wf_admit_keep(*[d[a] for a in K.ARGS])
    assert str(err.value).startswith("wf_admit_keep:")
    torch.cuda.synchronize()
    for k, x in before.items():         # refused before any launch
        assert torch.equal(d[k], x), k
