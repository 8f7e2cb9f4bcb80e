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

    python tools/wf_churn_bench.py --runs 2048 --fanout 256 --repeats 5
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

    dyn_window(args.warmup)
    sta_window(args.warmup)
    t_admit.take_ms(), t_drain.take_ms(), t_readmit.take_ms()

    rate = {"dynamic": [], "readmit": []}
    tick_ms = {"dynamic": [], "readmit": []}
    call_ms = {"admit": [], "drain_completed": [], "readmit_succeeded": []}
    for _ in range(args.repeats):
        for name, window in (("dynamic", dyn_window), ("readmit", sta_window)):
            ok, dt = window(args.ticks)
            rate[name].append(ok / dt)
            tick_ms[name].append(dt / args.ticks * 1000.0)
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
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
