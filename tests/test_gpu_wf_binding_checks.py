"""GPU tests of the argument checks in the host bindings of the row-scan
workflow kernels: wf_journal, wf_hold_scan, wf_settle, wf_cond_eval and
wf_hold_list.

Each binding is given the valid 17-row tables of its case builder
(tests/test_wf_*_cases.py) with one thing broken, and must refuse the call
with the matching message before anything is launched:
  a per-step table one row (64 entries) short   "table sizes disagree"
  a per-run table one entry short               "table sizes disagree"
  a table passed as a strided view of the       "must be contiguous"
  right length
Every table that a binding checks in one of these ways is broken once, so a
table dropped from a check fails here. The unbroken call must not raise.
The 16-byte alignment checks have their tests next to the kernels'.
"""
import pytest
import torch

from tests import test_wf_cond_cases as C
from tests import test_wf_hold_cases as H
from tests import test_wf_journal_cases as J
from tests import test_wf_settle_cases as S

pytestmark = pytest.mark.gpu

NR = 17

# binding -> (tables, argument names, per-step tables whose size is checked,
#             per-run tables whose size is checked, tables that must be
#             contiguous). NR is taken from run_life, which is never broken.
BINDINGS = {
    "wf_journal": (
        lambda: J.build_journal_tables(NR, "all", "ample"), J.ARGS,
        ("step_state", "ev_shadow_state"),
        ("run_gen", "ev_shadow_gen"),
        ("step_state", "ev_shadow_state", "ev_rec")),
    "wf_hold_scan": (
        lambda: H.build_scan_tables(NR, "fresh"), H.SCAN_ARGS,
        ("step_state", "hold_ttl", "hold_tick"),
        ("n_steps", "run_active", "run_gen", "hold_mask", "hold_gen"),
        ("step_state", "hold_ttl", "hold_tick", "hold_mask")),
    "wf_settle": (
        lambda: S.build_tables(NR, "edge"), S.ARGS,
        ("step_state",) + S.STEP_COLS,
        ("run_tmpl",),
        ("step_state",) + S.STEP_COLS + ("run_tmpl", "tmpl_policy", "tmpl_timeout")),
    "wf_cond_eval": (
        lambda: C.build_cond_tables(NR), C.COND_ARGS,
        ("step_state", "deps_mask", "step_kind", "step_out"),
        ("run_active", "run_tmpl", "cond_bits"),
        ("step_state", "deps_mask", "step_kind", "run_life", "run_active", "run_tmpl",
         "tmpl_cond", "tmpl_cond_mask", "run_input", "step_out", "cond_bits")),
    "wf_hold_list": (
        lambda: H.build_list_tables(NR), H.LIST_ARGS,
        ("step_state", "hold_tick"),
        ("run_active", "run_gen", "hold_mask", "hold_gen"),
        ("step_state", "hold_tick", "list")),
}

BREAKS = [(name, "step_short", k) for name, b in BINDINGS.items() for k in b[2]] \
    + [(name, "run_short", k) for name, b in BINDINGS.items() for k in b[3]] \
    + [(name, "strided", k) for name, b in BINDINGS.items() for k in b[4]]
PHRASE = {"step_short": "table sizes disagree", "run_short": "table sizes disagree",
          "strided": "must be contiguous"}


@pytest.fixture(scope="module")
def ext():
    from cordum_amd.ops import get_ext

    return get_ext(required=True)


def _device_tables(name):
    build, args = BINDINGS[name][:2]
    t = build()
    return {k: (t[k].clone().cuda() if torch.is_tensor(t[k]) else t[k]) for k in args}, args


def _strided(v):
    """The same values and length, every second element of a buffer twice as
    long; it starts where the buffer starts, so it is as aligned as `v`."""
    buf = torch.zeros(2 * v.numel(), dtype=v.dtype, device=v.device)
    view = buf[::2]
    view.copy_(v)
    assert view.numel() == v.numel() and not view.is_contiguous()
    return view


@pytest.mark.parametrize("name", list(BINDINGS))
def test_binding_accepts_the_valid_tables(ext, name):
    d, args = _device_tables(name)
    getattr(ext, name)(*[d[a] for a in args])
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,how,table", BREAKS)
def test_binding_rejects_one_broken_table(ext, name, how, table):
    d, args = _device_tables(name)
    v = d[table]
    if how == "step_short":
        assert v.numel() % (NR * 64) == 0
        d[table] = v[:-64]
    elif how == "run_short":
        assert v.numel() == NR
        d[table] = v[:-1]
    else:
        d[table] = _strided(v)
    before = {k: x.clone() for k, x in d.items() if torch.is_tensor(x)}
    with pytest.raises(RuntimeError, match=PHRASE[how]) as err:
        getattr(ext, name)(*[d[a] for a in args])
    assert str(err.value).startswith(name + ":")
    torch.cuda.synchronize()
    for k, x in before.items():         # refused before any launch
        assert torch.equal(d[k], x), k
