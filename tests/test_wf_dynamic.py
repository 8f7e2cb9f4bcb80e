"""Dynamic mode of the device workflow engine (run lifecycle: admit, cancel,
drain) on the CPU reference backend."""
import functools
import random

import pytest
import torch

from cordum_amd.ops.wf_pipeline import (
    DagSpec,
    StepSpec,
    WFK_APPROVAL,
    WFK_DELAY,
    WFK_FOR_EACH,
    WFK_WORKER,
    WFL_DRAINING,
    WFL_FREE,
    WFL_LIVE,
    WFS_CANCELLED,
    WFS_FAILED,
    WFS_SUCCEEDED,
    WorkflowPipeline,
)

pytestmark = pytest.mark.timeout(300)


def mk_pipe(dags, **kw):
    kw.setdefault("device", "cpu")
    kw.setdefault("backend", "ref")
    kw.setdefault("n_local_workers", 16)
    kw.setdefault("payload_words", 4)
    return WorkflowPipeline(dags=dags, **kw)


def random_dags():
    """The DAGs of test_device_tick_matches_host_engine_on_random_dags."""
    rng = random.Random(42)
    dags = []
    for _ in range(12):
        n = rng.randint(1, 6)
        steps = []
        for s in range(n):
            deps = [d for d in range(s) if rng.random() < 0.5]
            kind = rng.choice([WFK_WORKER, WFK_FOR_EACH, WFK_APPROVAL, WFK_DELAY])
            steps.append(StepSpec(kind, deps=deps,
                                  fanout=rng.randint(1, 9) if kind == WFK_FOR_EACH else 1,
                                  max_parallel=rng.choice([0, 0, 2, 3])
                                  if kind == WFK_FOR_EACH else 0,
                                  delay_ticks=rng.randint(0, 3)))
        dags.append(DagSpec(steps=steps))
    return dags


AMPLE = dict(child_cap=4096, pad_cap=4096, fail_ppt=0)
ROWS = ("step_state", "children_done", "step_attempts")
T_SHIFT = 48


def snapshot(pipe, slots):
    return {k: getattr(pipe, k).view(-1, 64)[slots].clone() for k in ROWS}


@functools.lru_cache(maxsize=None)
def static_history():
    """Per-tick rows of the random DAGs as one static wave: computed once."""
    dags = random_dags()
    pipe = mk_pipe(dags, **AMPLE)
    pipe.reset_runs()
    hist = []
    for _ in range(T_SHIFT):
        pipe.tick()
        hist.append(snapshot(pipe, list(range(len(dags)))))
    assert pipe.active() == 0, "T_SHIFT ticks must finish the wave"
    return dags, hist, pipe.run_state.clone()


@pytest.mark.parametrize("k", [0, 1, 7])
def test_admitted_run_is_the_static_run_shifted_by_k_ticks(k):
    dags, hist, static_state = static_history()
    filler = DagSpec.fanout_approval(6)
    pipe = mk_pipe(dags + [filler], dynamic_capacity=24, **AMPLE)
    # other runs already in the table, at slots the new runs do not get
    other, _ = pipe.admit([len(dags)] * 5 + [3, 4])
    assert other == list(range(7))
    for _ in range(k):
        pipe.tick()
    assert int(pipe.tick_buf[0]) == k - 1
    slots, gens = pipe.admit(list(range(len(dags))))
    assert slots == list(range(7, 7 + len(dags))) and gens == [1] * len(dags)
    plain = [i for i, d in enumerate(dags)
             if all(s.kind != WFK_APPROVAL for s in d.steps)]
    assert 3 <= len(plain) < len(dags)
    for j in range(T_SHIFT):
        pipe.tick()
        got = snapshot(pipe, slots)
        for key in ROWS:
            assert torch.equal(got[key][plain], hist[j][key][plain]), (key, j)
    # approval holds take the host grant hop, whose latency depends on the
    # other holds in the table: terminal state only
    assert torch.equal(pipe.run_state[slots], static_state)
    assert not bool(pipe.run_active[slots].any())


def test_lowest_free_slot_across_admit_drain_admit():
    pipe = mk_pipe([DagSpec(steps=[StepSpec(WFK_WORKER)])], dynamic_capacity=6)
    assert pipe.admit([0] * 4) == ([0, 1, 2, 3], [1, 1, 1, 1])
    assert pipe.cancel([2, 1], [1, 1]) == [1, 1]
    assert pipe.drain_completed() == ([1, 2], [1, 1], [WFS_CANCELLED] * 2)
    assert pipe.run_life.tolist() == [WFL_LIVE, WFL_FREE, WFL_FREE, WFL_LIVE,
                                      WFL_FREE, WFL_FREE]
    # the lowest free slots in request order, generations bumped on reuse
    assert pipe.admit([0] * 3) == ([1, 2, 4], [2, 2, 1])
    for _ in range(3):
        pipe.tick()
    assert pipe.drain_completed() == ([0, 1, 2, 3, 4], [1, 2, 2, 1, 1],
                                      [WFS_SUCCEEDED] * 5)
    assert pipe.drain_completed() == ([], [], [])
    assert pipe.admit([0]) == ([0], [2])
    assert int(pipe.admit_count[0]) == 8 and int(pipe.cancel_count[0]) == 2


def test_table_full_rejects_the_excess_until_a_drain():
    pipe = mk_pipe([DagSpec(steps=[StepSpec(WFK_WORKER)])], dynamic_capacity=3)
    slots, gens = pipe.admit([0] * 5)
    assert slots == [0, 1, 2, -1, -1]
    assert pipe.admit([0]) == ([-1], [0])
    assert int(pipe.admit_count[0]) == 3
    for _ in range(3):
        pipe.tick()
    # terminal but not drained: the slots are still taken
    assert pipe.active() == 0 and pipe.admit([0]) == ([-1], [0])
    assert pipe.drain_completed()[0] == [0, 1, 2]
    assert pipe.admit([0] * 2) == ([0, 1], [2, 2])


def test_admit_rejects_bad_requests_on_the_host():
    pipe = mk_pipe([DagSpec(steps=[StepSpec(WFK_FOR_EACH, fanout=3)])],
                   dynamic_capacity=3, child_cap=64)
    with pytest.raises(ValueError):
        pipe.admit([1])
    with pytest.raises(ValueError):
        pipe.admit([-1])
    with pytest.raises(ValueError):
        pipe.admit([0], fanout=[65])   # larger than the child arena
    with pytest.raises(ValueError):   # the same limit on a template's own fan-out
        pipe.add_template(DagSpec(steps=[StepSpec(WFK_FOR_EACH, fanout=65)]))
    with pytest.raises(ValueError):
        pipe.add_template(DagSpec(steps=[StepSpec(WFK_WORKER)] * 65))
    assert pipe.n_templates == 1
    assert pipe.admit([]) == ([], [])
    assert pipe.run_life.tolist() == [WFL_FREE] * 3
    t = pipe.add_template(DagSpec(steps=[StepSpec(WFK_WORKER)]))
    assert t == 1 and pipe.admit([1, 0], fanout=[0, 64])[0] == [0, 1]
    assert int(pipe.children_todo[64]) == 64


def test_cancel_midflight_quarantines_the_row_until_quiescent():
    """pad_cap far below the fan-out: children park in the requeue ring. The
    cancelled run is reported once, its slot is not reused while a parked
    child can still apply, and the next occupant's accounting is exact."""
    FAN = 40
    pipe = mk_pipe([DagSpec(steps=[StepSpec(WFK_FOR_EACH, fanout=FAN)])],
                   dynamic_capacity=1, pad_cap=8, max_retries=10)
    assert pipe.admit([0]) == ([0], [1])
    pipe.tick()
    assert int(pipe.rq_count[0]) > 0               # children really are parked
    assert 0 < int(pipe.children_out[0]) < FAN
    assert pipe.cancel([0], [1]) == [1]
    assert pipe.cancel([0], [1]) == [0]            # already cancelled
    assert pipe.drain_completed() == ([0], [1], [WFS_CANCELLED])
    reports, waited = 0, 0
    while int(pipe.run_life[0]) != WFL_FREE:
        assert int(pipe.run_life[0]) == WFL_DRAINING
        assert int(pipe.children_out[0]) > 0       # not quiescent, and young
        assert int(pipe.dispatch_tick[0]) > int(pipe.tick_buf[0]) - pipe.timeout_cutoff
        assert pipe.admit([0]) == ([-1], [0])      # the slot is not reused
        pipe.tick()
        reports += len(pipe.drain_completed()[0])
        waited += 1
        assert waited < 30
    assert reports == 0 and waited >= 2            # reported once, above
    assert int(pipe.children_out[0]) == 0
    assert pipe.admit([0]) == ([0], [2])
    for _ in range(40):
        pipe.tick()
        done = pipe.drain_completed()
        if done[0]:
            break
    assert done == ([0], [2], [WFS_SUCCEEDED])
    assert int(pipe.children_done[0]) == FAN       # no child of the old run
    assert int(pipe.children_fail[0]) == 0


def test_lost_results_free_a_cancelled_slot_by_staleness():
    """drop_ppt = 1000: no child result ever comes home, children_out never
    drains. The cancelled row is freed once its last expansion is
    timeout_cutoff ticks old, not never."""
    CUT = 8
    pipe = mk_pipe([DagSpec(steps=[StepSpec(WFK_FOR_EACH, fanout=5)])],
                   dynamic_capacity=2, drop_ppt=1000, timeout_cutoff=CUT)
    assert pipe.admit([0]) == ([0], [1])
    pipe.tick()                                    # expansion at tick 0
    assert int(pipe.dispatch_tick[0]) == 0 and int(pipe.children_out[0]) == 5
    assert pipe.cancel([0], [1]) == [1]
    assert pipe.drain_completed() == ([0], [1], [WFS_CANCELLED])
    for _ in range(CUT - 1):
        pipe.tick()
        assert pipe.drain_completed() == ([], [], [])
        assert int(pipe.run_life[0]) == WFL_DRAINING
    pipe.tick()                                    # tick CUT: 0 <= CUT - CUT
    assert int(pipe.tick_buf[0]) == CUT
    assert pipe.drain_completed() == ([], [], [])
    assert int(pipe.run_life[0]) == WFL_FREE
    assert int(pipe.children_out[0]) == 5          # freed by age, not by count
    assert pipe.admit([0]) == ([0], [2])


def test_stale_handle_cancel_after_reuse_is_a_noop():
    pipe = mk_pipe([DagSpec(steps=[StepSpec(WFK_DELAY, delay_ticks=3),
                                   StepSpec(WFK_WORKER, deps=[0])])],
                   dynamic_capacity=2)
    assert pipe.admit([0]) == ([0], [1])
    assert pipe.cancel([0], [1]) == [1]
    assert pipe.drain_completed()[0] == [0]
    assert pipe.admit([0]) == ([0], [2])
    pipe.tick()
    before = pipe.step_state.clone()
    assert pipe.cancel([0, 0, 1], [1, 2, 1]) == [0, 0, 0]   # stale, repeated, free
    assert torch.equal(pipe.step_state, before) and int(pipe.run_active[0]) == 1
    assert int(pipe.cancel_count[0]) == 1
    for _ in range(6):
        pipe.tick()
    assert pipe.drain_completed() == ([0], [2], [WFS_SUCCEEDED])


def test_conservation_over_a_200_tick_churn():
    rng = random.Random(11)
    dags = [d for d in random_dags()]
    pipe = mk_pipe(dags, dynamic_capacity=7, fail_ppt=120, max_retries=1,
                   child_cap=512)
    live, reported = {}, []
    admitted = rejected = cancelled_ok = 0
    for tick in range(200):
        slots, gens, states = pipe.drain_completed()
        for h in zip(slots, gens, states):
            reported.append(h)
            assert live.pop(h[:2]) is True
        want = [rng.randrange(len(dags)) for _ in range(rng.randint(0, 3))]
        for s, g in zip(*pipe.admit(want)):
            if s < 0:
                rejected += 1
                continue
            assert (s, g) not in live
            live[(s, g)] = True
            admitted += 1
        if live and rng.random() < 0.3:
            h = rng.choice(sorted(live))
            cancelled_ok += pipe.cancel([h[0]], [h[1]])[0]
        pipe.tick()
    slots, gens, states = pipe.drain_completed()
    for h in zip(slots, gens, states):
        reported.append(h)
        assert live.pop(h[:2]) is True
    by = {s: sum(1 for r in reported if r[2] == s)
          for s in (WFS_SUCCEEDED, WFS_FAILED, WFS_CANCELLED)}
    assert sum(by.values()) == len(reported)
    assert admitted == sum(by.values()) + len(live)
    assert len(set(r[:2] for r in reported)) == len(reported)   # each once
    assert admitted == int(pipe.admit_count[0])
    assert by[WFS_CANCELLED] == cancelled_ok == int(pipe.cancel_count[0])
    assert (by[WFS_SUCCEEDED], by[WFS_FAILED]) == pipe.counts()
    # the churn was a churn: every outcome, rejections and slot reuse occur
    assert min(by.values()) > 0 and rejected > 0 and len(live) > 0
    assert int(pipe.run_gen.max()) > 3
    # what is still live is LIVE and active on the device
    for s, g in live:
        assert int(pipe.run_life[s]) == WFL_LIVE and int(pipe.run_gen[s]) == g


def test_static_entry_points_raise_in_dynamic_mode():
    pipe = mk_pipe([DagSpec.fanout_approval(4)], dynamic_capacity=4)
    for call in (pipe.reset_runs, pipe.run_wave, pipe.readmit_succeeded,
                 pipe.drain_failed_to_dlq):
        with pytest.raises(RuntimeError):
            call()


def test_lifecycle_entry_points_raise_in_static_mode():
    pipe = mk_pipe([DagSpec.fanout_approval(4)])
    assert not pipe.dynamic and not hasattr(pipe, "run_life")
    with pytest.raises(RuntimeError):
        pipe.admit([0])
    with pytest.raises(RuntimeError):
        pipe.cancel([0], [1])
    with pytest.raises(RuntimeError):
        pipe.drain_completed()
    with pytest.raises(RuntimeError):
        pipe.add_template(DagSpec.fanout_approval(4))


def test_dynamic_table_starts_free_and_zero():
    pipe = mk_pipe(random_dags(), dynamic_capacity=9, template_cap=16)
    for k in ("step_state", "deps_mask", "step_kind", "children_todo",
              "max_parallel", "next_ready", "n_steps", "cond_bits", "run_active",
              "run_state", "run_life", "run_gen"):
        assert not bool(getattr(pipe, k).any()), k
    assert pipe.NR == 9 and pipe.n_templates == 12
    assert pipe.tmpl_deps.numel() == 16 * 64 and pipe.tmpl_nsteps.numel() == 16
    assert pipe.done_slot.numel() == 9 and pipe.done_count.numel() == 1
    assert pipe.run_life.dtype == torch.uint8 and pipe.run_gen.dtype == torch.int32
    assert pipe.cancel_count.dtype == torch.int64
    for _ in range(3):      # ticking an empty table changes only the counter
        pipe.tick()
    assert int(pipe.tick_buf[0]) == 2 and pipe.counts() == (0, 0)
