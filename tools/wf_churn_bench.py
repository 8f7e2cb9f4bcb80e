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

    python tools/wf_churn_bench.py --runs 2048 --fanout 256 --repeats 5
    python tools/wf_churn_bench.py --runs 2048 --fanout 256 --repeats 5 --events
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
    if ev_window is not None:
        modes.insert(1, ("events", ev_window))
    for _, window in modes:
        window(args.warmup)
    t_admit.take_ms(), t_drain.take_ms(), t_readmit.take_ms()

    rate = {name: [] for name, _ in modes}
    tick_ms = {name: [] for name, _ in modes}
    ev_rate = []
    call_ms = {"admit": [], "drain_completed": [], "readmit_succeeded": []}
    for _ in range(args.repeats):
        for name, window in modes:
            if name == "events":
                n_events[0] = 0
            ok, dt = window(args.ticks)
            rate[name].append(ok / dt)
            tick_ms[name].append(dt / args.ticks * 1000.0)
            if name == "events":
                ev_rate.append(n_events[0] / dt)
        # per-call medians of this repeat
        for key, timer in (("admit", t_admit), ("drain_completed", t_drain),
                           ("readmit_succeeded", t_readmit)):
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
        "readmit_runs_per_s": spread(rate["readmit"]),
        "dynamic_over_readmit": round(
            statistics.median(rate["dynamic"]) / max(1e-9, statistics.median(rate["readmit"])), 3),
        "ms_per_tick": {k: spread(v) for k, v in tick_ms.items()},
        "ms_per_call_device_events": {k: spread(v) for k, v in call_ms.items() if v},
        "graph": {"dynamic": bool(dyn._wf_graph), "readmit": bool(sta._wf_graph)},
        "live_at_end": live[0],
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
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
