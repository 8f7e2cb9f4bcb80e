#!/usr/bin/env python3
"""Sustained run churn on the device workflow engine: dynamic admission
against the readmit continuous mode.

Holds --runs live runs of the config #3 DAG (seed -> 1->N fan-out ->
approval -> final). Dynamic mode: every tick it drains the completion
records, then admits as many runs as the table has room for
(`drain_completed` + `admit`). Baseline, in the same process and at the same
sizes: the static pipeline's `readmit_succeeded()` after every tick, which
recreates each finished run in its own slot on the device with no host
round trip.

Each repeat is one window of --ticks ticks per mode, the modes alternating;
the rate of a window is runs completed over host wall time (the window ends
in a device synchronise). `admit` and `drain_completed` are timed per call
with device events (the drain's time includes its D2H copy). Prints one JSON
line with the median and the min..max spread over the repeats.

With --events [CAP] a third mode joins the alternation: the same churn on a
pipeline with the step-transition journal on (event_cap CAP, default
2 * runs * 64, which cannot overflow), driven through `DeviceRunTable`, whose
poll() drains the journal every tick. It reports runs/s, events/s, the
`event_overflows` count and the bytes one journal pass has to move at this
table size (life bytes, plus generations, states and shadow of the rows that
are not FREE, plus the records written).

With --approvals a further mode joins the alternation: the same churn as the
dynamic window on a pipeline with approvals="external", where every tick
`open_holds()` lists the waiting approvals and `decide()` approves all of
them. It reports runs/s, holds/s, `open_holds` and `decide` per call by device
events, and the bytes one hold scan moves at this table size (a life byte per
slot; active byte, two generations, the mask and 64 state bytes per row that
is not FREE; tick and ttl of each continuing hold). It also times the hold
scan and the journal pass alone, alternating, on tables of --runs rows and of
--pass-rows rows (quiet: nothing to report; held: one continuing hold / one
changed step in every row).

With --step-policy a further mode joins the alternation: the same churn as the
dynamic window on a pipeline with step_policy=True and no annotated step, so
every step runs on the default policy and the two windows compute the same
thing, one through wf_settle, the other through wf_timeout_scan + wf_commit.
It reports runs/s and the ratio, and times the settle pass and the pair alone,
alternating on the same tables, at --runs and --pass-rows rows (quiet: no
DISPATCHED step; busy: one DISPATCHED step with a child in flight in every
row, which neither changes). --skip-readmit leaves the static baseline out, so
that a kernel trace of the run holds the pair's kernels from the dynamic
window only; --settle-pass ROWS runs nothing but the quiet pass timings at
that size, for a kernel trace of one table size.

With --conditions nothing but this runs: the churn of a branching template,
`a: worker -> c: condition(a's output > K) -> w: worker if true, f: for_each
if false`, on a pipeline with device_conditions=True, where wf_cond_eval
decides c and the two guards from the output word of a; against the same work
with the predicate evaluated before admission and the option off: one
template per outcome (`a -> c -> w` with c's bit set, `a -> c -> f` with it
clear), the host choosing by the same rule. Inputs alternate between 2K and 0,
so half of the runs take each branch. The two windows alternate; it reports
runs/s of both, the ratio, and the predicate counters. --cond-pass ROWS runs
nothing but the quiet passes of wf_cond_eval (nothing PENDING) and wf_settle
(nothing DISPATCHED) alone, alternating, at that size.

With --rerun nothing but this runs: `admit(keep=...)` (wf_admit_keep, every
request keeping the three steps before `final`) against plain `admit()`, per
call by device events, with n = 1, 256 and 4096 requests on a table of --runs
slots that is half full. The two calls alternate, 8 pairs per n after a
warm-up pair, and so does their order within a pair; what a call admitted is
cancelled and drained before the next one, so every call sees the same table.
The time of a call is the host's packing of the request, the H2D copy, the
launches and the D2H copy that ends it; the three launches of the two
bindings are timed alone as well, on requests that are on the device already
(`wf_admit_keep_launches_us`, `wf_admit_launches_us`). With --other-ext PATH (a build of the
extension from another commit) plain `admit()` on this build is timed against
plain `admit()` on that one in the same way, on one pipeline whose tables
both use. For illustration it also counts the child jobs emitted and the
ticks to completion of one full run and of a rerun of it from `final`.

    python tools/wf_churn_bench.py --runs 2048 --fanout 256 --repeats 5
    python tools/wf_churn_bench.py --runs 2048 --fanout 256 --repeats 5 --events
    python tools/wf_churn_bench.py --runs 2048 --fanout 256 --repeats 5 --approvals
    python tools/wf_churn_bench.py --runs 2048 --fanout 256 --repeats 5 --step-policy
    python tools/wf_churn_bench.py --runs 2048 --fanout 256 --repeats 5 --conditions
    python tools/wf_churn_bench.py --runs 8192 --fanout 256 --rerun
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3),
            "max": round(max(xs), 3), "n": len(xs)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=2048, help="live runs held")
    ap.add_argument("--fanout", type=int, default=256)
    ap.add_argument("--workers", type=int, default=1000)
    ap.add_argument("--payload-bytes", type=int, default=256)
    ap.add_argument("--ticks", type=int, default=200, help="ticks per window")
    ap.add_argument("--warmup", type=int, default=40, help="ticks before the first window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--events", type=int, nargs="?", const=0, default=None, metavar="CAP",
                    help="also run the churn with the step journal on "
                         "(CAP records; default 2 * runs * 64)")
    ap.add_argument("--approvals", action="store_true",
                    help="also run the churn with externally decided approvals "
                         "(open_holds + approve everything, every tick)")
    ap.add_argument("--pass-rows", type=int, default=1 << 20,
                    help="second table size for the scan / journal pass timings "
                         "(0: no pass timings, for a kernel trace of the churn alone)")
    ap.add_argument("--step-policy", action="store_true",
                    help="also run the churn with step_policy=True and default "
                         "policies (wf_settle in place of the scan / commit pair)")
    ap.add_argument("--skip-readmit", action="store_true",
                    help="leave the static readmit baseline out (kernel traces)")
    ap.add_argument("--settle-pass", type=int, default=0, metavar="ROWS",
                    help="only time the quiet settle pass and the pair at ROWS rows")
    ap.add_argument("--conditions", action="store_true",
                    help="only the branching churn: conditions decided on the device "
                         "against the predicate evaluated before admission")
    ap.add_argument("--cond-pass", type=int, default=0, metavar="ROWS",
                    help="only time the quiet wf_cond_eval and wf_settle passes at ROWS rows")
    ap.add_argument("--rerun", action="store_true",
                    help="only time admit(keep=...) against admit(), per call")
    ap.add_argument("--other-ext", metavar="PATH", default=None,
                    help="with --rerun: a second build of the extension (.so) to time "
                         "plain admit() against")
    ap.add_argument("--allow-cpu", action="store_true",
                    help="rehearse the host logic on the reference backend (no timings)")
    args = ap.parse_args()

    import torch

    from cordum_amd.ops.wf_pipeline import DagSpec, WFS_SUCCEEDED, WorkflowPipeline

    use_gpu = torch.cuda.is_available()
    if not use_gpu and not args.allow_cpu:
        print("wf_churn_bench needs a GPU (--allow-cpu rehearses without timings)",
              file=sys.stderr)
        return 2
    device = torch.device("cuda:0" if use_gpu else "cpu")
    dag = DagSpec.fanout_approval(args.fanout)
    common = dict(device=device, n_local_workers=args.workers,
                  payload_words=max(1, args.payload_bytes // 4),
                  backend="ext" if use_gpu else "ref",
                  child_cap=args.runs * (args.fanout + 2))

    def sync():
        if use_gpu:
            torch.cuda.synchronize(device)

    class Timer:
        """Device-event pairs around calls; read after the window's sync."""

        def __init__(self):
            self.pairs = []

        def __call__(self, fn, *a):
            if not use_gpu:
                return fn(*a)
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a)
            e1.record()
            self.pairs.append((e0, e1))
            return out

        def take_ms(self):
            ms = [a.elapsed_time(b) for a, b in self.pairs]
            self.pairs = []
            return ms

    def settle_pass_times(ext, NR, busy, reps=15):
        """The settle pass and the pair it replaces (timeout scan + commit)
        alone on one all-LIVE table of NR rows at stock policies, alternating,
        one device-event pair per side and round; µs, median (min..max).
        Quiet: no step is DISPATCHED. Busy: every row has one DISPATCHED step
        with a child in flight and nothing left to emit, which both sides
        read and leave as it is, so every round sees the same table."""
        d = device
        st = torch.full((NR * 64,), WFS_SUCCEEDED, dtype=torch.uint8, device=d)

        def zi():
            return torch.zeros(NR * 64, dtype=torch.int32, device=d)

        att, todo, out, done, fail, maxp, nready, dtick = (zi() for _ in range(8))
        tickb = torch.tensor([5], dtype=torch.int32, device=d)
        if busy:
            st.view(NR, 64)[:, 1] = 1              # WFS_DISPATCHED
            out.view(NR, 64)[:, 1] = 1
            dtick.view(NR, 64)[:, 1] = 5
        life = torch.ones(NR, dtype=torch.uint8, device=d)
        rtmpl = torch.zeros(NR, dtype=torch.int32, device=d)
        policy = torch.tensor([2, 2, 16, 512], dtype=torch.int32).repeat(64).to(d)
        timeout = torch.full((64,), 8, dtype=torch.int32, device=d)
        tcount = torch.zeros(1, dtype=torch.int64, device=d)
        rcount = torch.zeros(1, dtype=torch.int64, device=d)

        def pair():
            ext.wf_timeout_scan(st, out, fail, dtick, tickb, 8, tcount)
            ext.wf_commit(st, att, todo, out, done, fail, maxp, nready, tickb, 2, rcount)

        def settle():
            ext.wf_settle(st, att, todo, out, fail, maxp, nready, dtick, life, rtmpl,
                          policy, timeout, tickb, tcount, rcount)

        pair_t, settle_t = Timer(), Timer()
        for i in range(reps + 3):
            pair_t(pair)
            settle_t(settle)
            sync()
            if i < 3:                              # warm-up launches
                pair_t.take_ms(), settle_t.take_ms()
        assert int(tcount.cpu()[0]) == 0 and int(rcount.cpu()[0]) == 0
        if not use_gpu:
            return None
        return {"rows": NR, "case": "busy" if busy else "quiet",
                "pair_us": spread([1000 * x for x in pair_t.take_ms()]),
                "settle_us": spread([1000 * x for x in settle_t.take_ms()])}

    if args.settle_pass:
        from cordum_amd.ops import get_ext
        from cordum_amd.ops.pipeline import _RefOps

        ext = get_ext(required=True) if use_gpu else _RefOps()
        print(json.dumps({"metric": "settle pass vs timeout scan + commit, alone",
                          "unit": "us", "timed": bool(use_gpu),
                          "pass_times": [settle_pass_times(ext, args.settle_pass, False)]}))
        return 0

    def cond_pass_times(ext, NR, reps=15):
        """The quiet passes of wf_cond_eval and wf_settle alone on one all-LIVE
        table of NR rows, alternating, one device-event pair per side and
        round; µs, median (min..max). Every step of the one template carries
        a predicate, and no step is PENDING (or DISPATCHED): both passes read
        their columns and write nothing."""
        d = device
        st = torch.full((NR * 64,), WFS_SUCCEEDED, dtype=torch.uint8, device=d)

        def zi(n=NR * 64):
            return torch.zeros(n, dtype=torch.int32, device=d)

        att, todo, out, fail, maxp, nready, dtick, sout = (zi() for _ in range(8))
        tickb = torch.tensor([5], dtype=torch.int32, device=d)
        ones8 = torch.ones(NR, dtype=torch.uint8, device=d)
        rtmpl = zi(NR)
        policy = torch.tensor([2, 2, 16, 512], dtype=torch.int32).repeat(64).to(d)
        timeout = torch.full((64,), 8, dtype=torch.int32, device=d)
        tcount = torch.zeros(1, dtype=torch.int64, device=d)
        rcount = torch.zeros(1, dtype=torch.int64, device=d)
        deps = torch.zeros(NR * 64, dtype=torch.int64, device=d)
        kind = torch.zeros(NR * 64, dtype=torch.uint8, device=d)
        crec = torch.tensor([7 | 1 << 8, 0, 0, 0], dtype=torch.int32).repeat(64).to(d)
        cmask = torch.full((1,), -1, dtype=torch.int64, device=d)
        rin = zi(NR * 8)
        cbits = torch.zeros(NR, dtype=torch.int64, device=d)
        ccount = torch.zeros(2, dtype=torch.int64, device=d)

        def settle():
            ext.wf_settle(st, att, todo, out, fail, maxp, nready, dtick, ones8, rtmpl,
                          policy, timeout, tickb, tcount, rcount)

        def cond():
            ext.wf_cond_eval(st, deps, kind, ones8, ones8, rtmpl, crec, cmask, rin,
                             sout, cbits, ccount, 8)

        settle_t, cond_t = Timer(), Timer()
        for i in range(reps + 3):
            settle_t(settle)
            cond_t(cond)
            sync()
            if i < 3:                              # warm-up launches
                settle_t.take_ms(), cond_t.take_ms()
        assert int(ccount.cpu().sum()) == 0 and int(tcount.cpu()[0]) == 0
        if not use_gpu:
            return None
        return {"rows": NR, "case": "quiet",
                "settle_us": spread([1000 * x for x in settle_t.take_ms()]),
                "cond_eval_us": spread([1000 * x for x in cond_t.take_ms()])}

    if args.cond_pass:
        from cordum_amd.ops import get_ext
        from cordum_amd.ops.pipeline import _RefOps

        ext = get_ext(required=True) if use_gpu else _RefOps()
        print(json.dumps({"metric": "quiet wf_cond_eval pass vs quiet wf_settle pass, alone",
                          "unit": "us", "timed": bool(use_gpu),
                          "pass_times": [cond_pass_times(ext, args.cond_pass)]}))
        return 0

    if args.rerun:
        pipe = WorkflowPipeline(dags=[dag], dynamic_capacity=args.runs, **common)
        this_ext, other_ext = pipe.ext, None
        if args.other_ext:
            import importlib.util

            spec = importlib.util.spec_from_file_location("cordum_hip_ops", args.other_ext)
            other_ext = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(other_ext)
        held, _ = pipe.admit([0] * (args.runs // 2))
        assert min(held) >= 0
        KEEP = 0b0111                              # seed, fan-out and approval done

        def release(got):
            """Cancel and drain what a timed call admitted: the same table again."""
            if torch.is_tensor(got):               # a binding's [slots | gens]
                h = got.cpu().tolist()
                got = h[:len(h) // 2], h[len(h) // 2:]
            slots, gens = got
            live = [(s, g) for s, g in zip(slots, gens) if s >= 0]
            assert all(pipe.cancel([s for s, _ in live], [g for _, g in live]))
            done, _, _ = pipe.drain_completed()
            assert sorted(done) == sorted(s for s, _ in live)
            return len(live)

        def plain_on(ext):
            def call(n):
                pipe.ext = ext
                try:
                    return pipe.admit([0] * n)
                finally:
                    pipe.ext = this_ext
            return call

        def binding(name):
            """The three launches alone, on a request that is on the device."""
            def call(n):
                req = torch.zeros(4 * n, dtype=torch.int32, device=device)
                masks = torch.full((2 * n,), KEEP, dtype=torch.int64, device=device)
                masks[n:] = 0
                out = torch.empty(2 * n, dtype=torch.int32, device=device)
                tail = (masks[:n], masks[n:]) if name == "wf_admit_keep" else ()
                sync()
                return lambda _n: launch(name, req, out, n, tail)
            return call

        def launch(name, req, out, n, tail):
            getattr(this_ext, name)(
                req[2 * n:3 * n], req[:2 * n].view(torch.int64), req[3 * n:],
                pipe.tmpl_deps, pipe.tmpl_kind, pipe.tmpl_todo, pipe.tmpl_maxp,
                pipe.tmpl_delay, pipe.tmpl_nsteps,
                pipe.step_state, pipe.step_attempts, pipe.deps_mask, pipe.step_kind,
                pipe.children_todo, pipe.max_parallel, pipe.children_out,
                pipe.children_done, pipe.children_fail, pipe.children_emitted,
                pipe.next_ready, pipe.dispatch_tick, pipe.n_steps, pipe.cond_bits,
                pipe.run_state, pipe.run_active, pipe.run_life, pipe.run_gen,
                pipe.tick_buf, pipe._free_mask, pipe._blk_scan,
                out[:n], out[n:], pipe.admit_count, *tail)
            return out

        def alternate(a, b, n, pairs=8):
            ta, tb = Timer(), Timer()
            admitted = set()
            for i in range(pairs + 1):
                # the order within a pair alternates too: whichever call
                # comes first in a pair starts on an idle device
                for timer, fn in ((ta, a), (tb, b))[::1 if i % 2 else -1]:
                    admitted.add(release(timer(fn, n)))
                sync()
                if i == 0:                         # warm-up pair
                    ta.take_ms(), tb.take_ms()
            assert len(admitted) == 1              # every call found the same room
            if not use_gpu:
                return admitted.pop(), None, None
            return (admitted.pop(), spread([1000 * x for x in ta.take_ms()]),
                    spread([1000 * x for x in tb.take_ms()]))

        rows = []
        for n in (1, 256, 4096):
            k, keep_us, plain_us = alternate(
                lambda m: pipe.admit([0] * m, keep=[KEEP] * m), plain_on(this_ext), n)
            row = {"n": n, "admitted": k, "admit_keep_us": keep_us, "admit_us": plain_us}
            _, keep_us, plain_us = alternate(
                binding("wf_admit_keep")(n), binding("wf_admit")(n), n)
            row.update(wf_admit_keep_launches_us=keep_us, wf_admit_launches_us=plain_us)
            if other_ext is not None:
                _, here_us, there_us = alternate(plain_on(this_ext), plain_on(other_ext), n)
                row.update(admit_this_build_us=here_us, admit_other_build_us=there_us)
            rows.append(row)

        def to_the_end(keep):
            (slot,), _ = pipe.admit([0], keep=None if keep is None else [keep])
            for t in range(1, 200):
                pipe.tick()
                done, _, states = pipe.drain_completed()
                if slot in done:
                    assert states[done.index(slot)] == WFS_SUCCEEDED
                    return {"ticks": t,
                            "children": int(pipe.children_emitted[slot * 64:slot * 64 + 64].sum())}
            raise AssertionError("the run did not end")

        release(([s for s in held], [1] * len(held)))
        print(json.dumps({
            "metric": "admit(keep=...) vs admit() per call, alternating, device events "
                      "(config #3: 1->%d fan-out + approval; table half full)" % args.fanout,
            "unit": "us", "timed": bool(use_gpu), "runs": args.runs, "pairs": 8,
            "calls": rows,
            "full_run": to_the_end(None), "rerun_from_final": to_the_end(KEEP),
        }))
        return 0

    if args.conditions:
        from cordum_amd.ops.wf_pipeline import (
            CondSpec, StepSpec, WFK_CONDITION, WFK_FOR_EACH, WFK_WORKER)

        K = 1000
        branching = DagSpec(steps=[
            StepSpec(WFK_WORKER),
            StepSpec(WFK_CONDITION, deps=[0], when=CondSpec(">", ("out", 0), K)),
            StepSpec(WFK_WORKER, deps=[1], when=CondSpec("truthy", ("out", 1))),
            StepSpec(WFK_FOR_EACH, deps=[1], fanout=args.fanout,
                     when=CondSpec("==", ("out", 1), 0)),
        ])
        decided = [
            DagSpec(steps=[StepSpec(WFK_WORKER), StepSpec(WFK_CONDITION, deps=[0], cond=True),
                           StepSpec(WFK_WORKER, deps=[1])]),
            DagSpec(steps=[StepSpec(WFK_WORKER), StepSpec(WFK_CONDITION, deps=[0], cond=False),
                           StepSpec(WFK_FOR_EACH, deps=[1], fanout=args.fanout)]),
        ]
        words = max(10, args.payload_bytes // 4)
        kw = dict(common, payload_words=words)
        on = WorkflowPipeline(dags=[branching], dynamic_capacity=args.runs,
                              device_conditions=True, **kw)
        off = WorkflowPipeline(dags=decided, dynamic_capacity=args.runs, **kw)

        def window_of(pipe, admit):
            state = {"live": 0, "n": 0}

            def fill():
                want = args.runs - state["live"]
                if want:
                    # request i of the pipeline's life: input 2K (true) or 0 (false)
                    big = [(state["n"] + i) % 2 == 0 for i in range(want)]
                    got = admit(pipe, big)
                    k = sum(1 for s in got if s >= 0)
                    state["live"] += k
                    state["n"] += k
            fill()
            assert state["live"] == args.runs

            def window(n_ticks):
                ok = 0
                sync()
                t0 = time.perf_counter()
                for _ in range(n_ticks):
                    pipe.tick()
                    _, _, states = pipe.drain_completed()
                    ok += sum(1 for s in states if s == WFS_SUCCEEDED)
                    state["live"] -= len(states)
                    fill()
                sync()
                return ok, time.perf_counter() - t0
            return window

        modes = [
            ("conditions", window_of(on, lambda p, big: p.admit(
                [0] * len(big), inputs=[[2 * K if b else 0] for b in big])[0])),
            ("preevaluated", window_of(off, lambda p, big: p.admit(
                [0 if b else 1 for b in big])[0])),
        ]
        for _, window in modes:
            window(args.warmup)
        rate = {name: [] for name, _ in modes}
        tick_ms = {name: [] for name, _ in modes}
        for _ in range(args.repeats):
            for name, window in modes:
                ok, dt = window(args.ticks)
                rate[name].append(ok / dt)
                tick_ms[name].append(dt / args.ticks * 1000.0)
        print(json.dumps({
            "metric": "sustained workflow runs/s, conditions decided on the device vs "
                      "evaluated before admission (worker -> condition -> worker | "
                      "1->%d for_each)" % args.fanout,
            "unit": "runs/s", "timed": bool(use_gpu),
            "runs": args.runs, "fanout": args.fanout, "workers": args.workers,
            "payload_words": words, "ticks_per_window": args.ticks, "repeats": args.repeats,
            "conditions_runs_per_s": spread(rate["conditions"]),
            "preevaluated_runs_per_s": spread(rate["preevaluated"]),
            "conditions_over_preevaluated": round(
                statistics.median(rate["conditions"])
                / max(1e-9, statistics.median(rate["preevaluated"])), 3),
            "ratio_per_repeat": [round(a / max(1e-9, b), 3) for a, b in
                                 zip(rate["conditions"], rate["preevaluated"])],
            "ms_per_tick": {k: spread(v) for k, v in tick_ms.items()},
            "cond_stats": on.cond_stats(),
            "graph": {"conditions": bool(on._wf_graph), "preevaluated": bool(off._wf_graph)},
        }))
        return 0

    # ---- dynamic mode ------------------------------------------------------
    dyn = WorkflowPipeline(dags=[dag], dynamic_capacity=args.runs, **common)
    t_admit, t_drain = Timer(), Timer()
    live = [0]
    slots, _ = dyn.admit([0] * args.runs)
    live[0] = sum(1 for s in slots if s >= 0)
    assert live[0] == args.runs

    def dyn_window(n_ticks):
        ok = 0
        sync()
        t0 = time.perf_counter()
        for _ in range(n_ticks):
            dyn.tick()
            _, _, states = t_drain(dyn.drain_completed)
            ok += sum(1 for s in states if s == WFS_SUCCEEDED)
            live[0] -= len(states)
            want = args.runs - live[0]
            if want:
                got, _ = t_admit(dyn.admit, [0] * want)
                live[0] += sum(1 for s in got if s >= 0)
        sync()
        return ok, time.perf_counter() - t0

    # ---- dynamic mode with per-step policies (all of them the default) -----
    sp_window = None
    if args.step_policy:
        spp = WorkflowPipeline(dags=[dag], dynamic_capacity=args.runs,
                               step_policy=True, **common)
        sp_live = [0]
        got, _ = spp.admit([0] * args.runs)
        sp_live[0] = sum(1 for s in got if s >= 0)
        assert sp_live[0] == args.runs

        def sp_window(n_ticks):
            ok = 0
            sync()
            t0 = time.perf_counter()
            for _ in range(n_ticks):
                spp.tick()
                _, _, states = spp.drain_completed()
                ok += sum(1 for s in states if s == WFS_SUCCEEDED)
                sp_live[0] -= len(states)
                want = args.runs - sp_live[0]
                if want:
                    got, _ = spp.admit([0] * want)
                    sp_live[0] += sum(1 for s in got if s >= 0)
            sync()
            return ok, time.perf_counter() - t0

    # ---- dynamic mode with the step journal, through DeviceRunTable --------
    ev_window = None
    if args.events is not None:
        from cordum_amd.workflow.device_runs import DeviceRunTable

        ev_cap = args.events or 2 * args.runs * 64
        evp = WorkflowPipeline(dags=[dag], dynamic_capacity=args.runs,
                               event_cap=ev_cap, **common)
        table = DeviceRunTable(evp)
        next_id = [0]
        n_events = [0]

        def submit(n):
            for _ in range(n):
                table.submit(f"run-{next_id[0]}", 0)
                next_id[0] += 1

        # twice what the table holds: with submissions always waiting, every
        # later one queues too and poll() admits them in one batch per tick,
        # as the plain dynamic window does. The table itself stays full.
        submit(2 * args.runs)
        assert table.queued() == args.runs

        def ev_window(n_ticks):
            ok = 0
            sync()
            t0 = time.perf_counter()
            for _ in range(n_ticks):
                table.tick()
                done = table.poll()
                ok += sum(1 for _, st in done if st == "succeeded")
                n_events[0] += len(table.take_events())
                submit(len(done))
            sync()
            return ok, time.perf_counter() - t0

    # ---- dynamic mode with externally decided approvals --------------------
    ap_window = None
    if args.approvals:
        exp = WorkflowPipeline(dags=[dag], dynamic_capacity=args.runs,
                               approvals="external", **common)
        t_holds, t_decide = Timer(), Timer()
        ap_live = [0]
        n_holds = [0]
        got, _ = exp.admit([0] * args.runs)
        ap_live[0] = sum(1 for s in got if s >= 0)
        assert ap_live[0] == args.runs

        def ap_window(n_ticks):
            ok = 0
            sync()
            t0 = time.perf_counter()
            for _ in range(n_ticks):
                exp.tick()
                slots, gens, steps, _ = t_holds(exp.open_holds)
                if slots:
                    codes = t_decide(exp.decide, slots, gens, steps, [1] * len(slots))
                    assert not any(codes)
                    n_holds[0] += len(slots)
                _, _, states = exp.drain_completed()
                ok += sum(1 for s in states if s == WFS_SUCCEEDED)
                ap_live[0] -= len(states)
                want = args.runs - ap_live[0]
                if want:
                    got, _ = exp.admit([0] * want)
                    ap_live[0] += sum(1 for s in got if s >= 0)
            sync()
            return ok, time.perf_counter() - t0

    def pass_times(NR, held, reps=15):
        """Hold scan and journal pass alone on an all-LIVE table of NR rows,
        alternating, one device-event pair per launch; µs, median (min..max).
        Quiet: nothing waits and nothing changed. Held: every row has one
        continuing hold (scan), one changed step (journal)."""
        ext, d = dyn.ext, device
        st = torch.full((NR * 64,), WFS_SUCCEEDED, dtype=torch.uint8, device=d)
        ones8 = torch.ones(NR, dtype=torch.uint8, device=d)
        gen = torch.ones(NR, dtype=torch.int32, device=d)
        hgen, sgen = gen.clone(), gen.clone()      # hold / shadow generations
        ns =torch.full((NR,), 4, dtype=torch.uint8, device=d)
        tickb = torch.tensor([5], dtype=torch.int32, device=d)
        ttl = torch.zeros(NR * 64, dtype=torch.int32, device=d)
        htick = torch.zeros(NR * 64, dtype=torch.int32, device=d)
        mask = torch.zeros(NR, dtype=torch.int64, device=d)
        counts = torch.zeros(4, dtype=torch.int64, device=d)
        hopen = torch.zeros(1, dtype=torch.int32, device=d)
        if held:
            st.view(NR, 64)[:, 1] = 2              # WFS_WAITING
            ttl.view(NR, 64)[:, 1] = 1 << 30
            mask.fill_(2)
        shadow = st.clone()
        rec = torch.zeros(4 * (NR + 1024), dtype=torch.int32, device=d)
        cnt = torch.zeros(1, dtype=torch.int32, device=d)
        scan_t, jour_t = Timer(), Timer()
        for i in range(reps + 3):
            if held:
                shadow.view(NR, 64)[:, 1] = 0      # one change per row, again
                cnt.zero_()
            hopen.zero_()
            scan_t(ext.wf_hold_scan, st, ns, ones8, ones8, gen, tickb, ttl, mask,
                   htick, hgen, counts, hopen)
            jour_t(ext.wf_journal, st, ones8, gen, tickb, 0, shadow, sgen, rec, cnt)
            sync()
            if i < 3:                              # warm-up launches
                scan_t.take_ms(), jour_t.take_ms()
        if not use_gpu:
            return None
        return {"rows": NR, "case": "held" if held else "quiet",
                "scan_us": spread([1000 * x for x in scan_t.take_ms()]),
                "journal_us": spread([1000 * x for x in jour_t.take_ms()])}

    # ---- baseline: readmit continuous mode ---------------------------------
    sta = WorkflowPipeline(dags=[dag], replicate=args.runs, **common)
    sta.reset_runs()
    t_readmit = Timer()

    def sta_window(n_ticks):
        sync()
        ok0 = sta.counts()[0]
        t0 = time.perf_counter()
        for _ in range(n_ticks):
            sta.tick()
            t_readmit(sta.readmit_succeeded)
        ok1 = sta.counts()[0]          # D2H: ends the window in a synchronise
        return ok1 - ok0, time.perf_counter() - t0

    modes = [("dynamic", dyn_window), ("readmit", sta_window)]
    if args.skip_readmit:
        modes.pop()
    if sp_window is not None:
        modes.insert(1, ("step_policy", sp_window))
    if ev_window is not None:
        modes.insert(1, ("events", ev_window))
    if ap_window is not None:
        modes.insert(1, ("approvals", ap_window))
    for _, window in modes:
        window(args.warmup)
    t_admit.take_ms(), t_drain.take_ms(), t_readmit.take_ms()
    if ap_window is not None:
        t_holds.take_ms(), t_decide.take_ms()

    rate = {name: [] for name, _ in modes}
    tick_ms = {name: [] for name, _ in modes}
    ev_rate = []
    hold_rate = []
    call_ms = {"admit": [], "drain_completed": [], "readmit_succeeded": []}
    timers = [("admit", t_admit), ("drain_completed", t_drain),
              ("readmit_succeeded", t_readmit)]
    if ap_window is not None:
        call_ms.update(open_holds=[], decide=[])
        timers += [("open_holds", t_holds), ("decide", t_decide)]
    for _ in range(args.repeats):
        for name, window in modes:
            if name == "events":
                n_events[0] = 0
            if name == "approvals":
                n_holds[0] = 0
            ok, dt = window(args.ticks)
            rate[name].append(ok / dt)
            tick_ms[name].append(dt / args.ticks * 1000.0)
            if name == "events":
                ev_rate.append(n_events[0] / dt)
            if name == "approvals":
                hold_rate.append(n_holds[0] / dt)
        # per-call medians of this repeat
        for key, timer in timers:
            ms = timer.take_ms()
            if ms:
                call_ms[key].append(statistics.median(ms))

    out = {
        "metric": "sustained workflow runs/s, dynamic admit+drain vs readmit "
                  "(config #3: 1->%d fan-out + approval)" % args.fanout,
        "unit": "runs/s",
        "timed": bool(use_gpu),
        "runs": args.runs, "fanout": args.fanout, "workers": args.workers,
        "ticks_per_window": args.ticks, "repeats": args.repeats,
        "dynamic_runs_per_s": spread(rate["dynamic"]),
        "ms_per_tick": {k: spread(v) for k, v in tick_ms.items()},
        "ms_per_call_device_events": {k: spread(v) for k, v in call_ms.items() if v},
        "graph": {"dynamic": bool(dyn._wf_graph), "readmit": bool(sta._wf_graph)},
        "live_at_end": live[0],
    }
    if not args.skip_readmit:
        out["readmit_runs_per_s"] = spread(rate["readmit"])
        out["dynamic_over_readmit"] = round(
            statistics.median(rate["dynamic"]) / max(1e-9, statistics.median(rate["readmit"])), 3)
    if sp_window is not None:
        out["step_policy"] = {
            "runs_per_s": spread(rate["step_policy"]),
            "step_policy_over_dynamic": round(
                statistics.median(rate["step_policy"])
                / max(1e-9, statistics.median(rate["dynamic"])), 3),
            # per repeat, the two windows back to back
            "ratio_per_repeat": [round(a / max(1e-9, b), 3) for a, b in
                                 zip(rate["step_policy"], rate["dynamic"])],
            "graph": bool(spp._wf_graph),
            "pass_times": [settle_pass_times(dyn.ext, n, busy) for n in
                           ((args.runs, args.pass_rows) if use_gpu else (64,))
                           for busy in (False, True)] if args.pass_rows else [],
        }
    if ev_window is not None:
        per_tick = statistics.median(ev_rate) * statistics.median(tick_ms["events"]) / 1000.0
        # one pass: a life byte per slot; generation + shadow generation,
        # 64 state and 64 shadow bytes per row that is not FREE (the table is
        # held full); 16 bytes per record written
        pass_bytes = args.runs * (1 + 4 + 4 + 64 + 64) + 16 * per_tick
        out["events"] = {
            "event_cap": ev_cap,
            "runs_per_s": spread(rate["events"]),
            "events_per_s": spread(ev_rate),
            "events_over_dynamic": round(
                statistics.median(rate["events"]) / max(1e-9, statistics.median(rate["dynamic"])), 3),
            "event_overflows": evp.event_overflows,
            "events_per_tick": round(per_tick, 1),
            "journal_bytes_per_pass": int(pass_bytes),
            "graph": bool(evp._wf_graph),
        }
    if ap_window is not None:
        per_tick = statistics.median(hold_rate) * statistics.median(tick_ms["approvals"]) / 1000.0
        # one scan: a life byte per slot; active byte, generation + hold
        # generation, the mask word and 64 state bytes per row that is not
        # FREE (the table is held full); a fresh hold writes its tick and the
        # mask, a continuing one reads its ttl (and its tick when ttl > 0)
        scan_bytes = args.runs * (1 + 1 + 4 + 4 + 8 + 64) + (4 + 8) * per_tick
        out["approvals"] = {
            "hold_cap": exp.hold_cap,
            "runs_per_s": spread(rate["approvals"]),
            "holds_per_s": spread(hold_rate),
            "approvals_over_dynamic": round(
                statistics.median(rate["approvals"]) / max(1e-9, statistics.median(rate["dynamic"])), 3),
            "holds_per_tick": round(per_tick, 1),
            "scan_bytes_per_pass": int(scan_bytes),
            "hold_stats": exp.hold_stats(),
            "graph": bool(exp._wf_graph),
            "pass_times": [pass_times(n, held) for n in
                           ((args.runs, args.pass_rows) if use_gpu else (64,))
                           for held in (False, True)] if args.pass_rows else [],
        }
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
