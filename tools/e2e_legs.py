#!/usr/bin/env python3
"""Host-side legs of the pipelined e2e ingest step (bench window 1), profiler
off: (a) host encode per batch, serial, payload stamp included; (b) the main
thread's busy time per step in the submit loop (staging copies, event ops,
graph replay, result copy enqueue) with no encode and no harvest wait in the
way. The device legs (kernels, H2D/D2H copies) come from rocprofv3 traces.

Run on a GPU box; prints one JSON line. Works on trees with or without the
one-call stamped encoder, the fused result block and compact descriptor
staging. Where the pipeline has compact staging it measures the path e2e_run
takes (compact by default); `--full-layout` builds the pipeline with
compact_staging=False and measures the full-layout path instead.

  python tools/e2e_legs.py [reps] [--full-layout]"""
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from cordum_amd.ops.pipeline import DevicePipeline
from cordum_amd.utils.threads import cap_torch_threads


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    full_layout = "--full-layout" in sys.argv[1:]
    reps = int(args[0]) if args else 400
    cap_torch_threads()
    dev = torch.device("cuda:0")
    kw = dict(device=dev, batch_size=16384, n_local_workers=1000,
              n_rules=1024, n_batches=2, mfma_pack_on_device=True)
    import inspect

    if "compact_staging" in inspect.signature(DevicePipeline.__init__).parameters:
        kw["compact_staging"] = False if full_layout else None
    pipe = DevicePipeline(**kw)
    pipe.e2e_run(8)  # allocates the staging rings, captures the graphs
    torch.cuda.synchronize(dev)
    B, W = pipe.B, pipe.payload_words
    ext = pipe.ext
    stamped = hasattr(pipe._e2e_encs[0], "fresh_stamped")
    nhost = len(pipe._e2e_hosts2)
    # what e2e_run stages and replays on this pipeline
    compact = bool(getattr(pipe, "_compact", False))
    dev_bufs = pipe.compact_bufs if compact else pipe.batch_bufs
    host_bufs = pipe._e2e_cbufs if compact else pipe._e2e_host_bufs
    graphs = pipe._cgraphs if compact else pipe._graphs

    def encode(s, threads):
        hb = pipe._e2e_hosts2[s % nhost]
        enc = pipe._e2e_encs[s % nhost]
        payload = pipe._e2e_payloads[s % len(pipe._e2e_payloads)]
        if compact:
            enc.fresh_compact(pipe._e2e_ccols[s % nhost], s, ext, pipe._e2e_ccolumns,
                              payload, W, threads=threads)
        elif stamped:
            enc.fresh_stamped(hb, s, ext, payload, W, threads=threads)
        else:
            enc.fresh_fast(hb, s, ext)
            payload.view(B, W)[:, 0] = s

    import gc

    gc.collect()
    gc.freeze()
    gc.disable()
    out = {"stamped_encoder": stamped, "reps": reps, "compact_staging": compact,
           "live_dims": list(getattr(pipe, "_live", [])) if compact else None}
    for threads in ((1, 2) if stamped else (1,)):
        ts = []
        for s in range(reps):
            t0 = time.perf_counter()
            encode(s, threads)
            ts.append(time.perf_counter() - t0)
        ts = ts[reps // 10:]
        out[f"encode_us_threads{threads}"] = {
            "p50": round(statistics.median(ts) * 1e6, 1),
            "mean": round(sum(ts) / len(ts) * 1e6, 1),
            "p90": round(sorted(ts)[int(len(ts) * 0.9)] * 1e6, 1),
        }

    # submit loop alone: what e2e_run's main thread enqueues per step
    fused_out = hasattr(pipe, "_e2e_out_blocks")
    main_stream = torch.cuda.current_stream(dev)
    nslots = 2
    runs = []
    for _ in range(5):
        torch.cuda.synchronize(dev)
        n = 64  # short enough that no queue fills and blocks the enqueue
        t0 = time.perf_counter()
        for s in range(n):
            slot = s % nslots
            with torch.cuda.stream(pipe._e2e_copy_stream):
                if s >= nslots:
                    # e2e_run proves graph s-2 done by harvesting it; with no
                    # harvest here, order the restage behind it on the device
                    # (one extra event wait per step, counted in the figure)
                    pipe._e2e_copy_stream.wait_event(pipe._e2e_ev[slot])
                dev_bufs[slot].copy_(host_bufs[s % nhost], non_blocking=True)
                pipe.payloads[slot].copy_(
                    pipe._e2e_payloads[s % len(pipe._e2e_payloads)],
                    non_blocking=True)
                pipe._e2e_in_ev[slot].record(pipe._e2e_copy_stream)
            main_stream.wait_event(pipe._e2e_in_ev[slot])
            graphs[slot].replay()
            if fused_out:
                pipe._e2e_out_blocks[slot].copy_(pipe._res_block, non_blocking=True)
            else:
                pipe._e2e_out_sums[slot].copy_(pipe.res_sums, non_blocking=True)
                pipe._e2e_out_dec[slot].copy_(pipe.out_decision, non_blocking=True)
                pipe._e2e_out_counts[slot].copy_(pipe._counts, non_blocking=True)
            pipe._e2e_ev[slot].record()
        t1 = time.perf_counter()
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        runs.append(((t1 - t0) / n * 1e6, (t2 - t0) / n * 1e6))
    # copy legs on an otherwise idle device, device events around n steps'
    # worth of copies: H2D = descriptors + payload (what a step stages),
    # D2H = what a step reads back; and the captured tick alone
    def timed(fn, n=50):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for s in range(n):
            fn(s)
        e1.record()
        torch.cuda.synchronize(dev)
        return round(e0.elapsed_time(e1) * 1e3 / n, 1)

    def h2d(s):
        dev_bufs[s % nslots].copy_(host_bufs[s % nhost], non_blocking=True)
        pipe.payloads[s % nslots].copy_(pipe._e2e_payloads[s % len(pipe._e2e_payloads)],
                                        non_blocking=True)

    def d2h(s):
        slot = s % nslots
        if fused_out:
            pipe._e2e_out_blocks[slot].copy_(pipe._res_block, non_blocking=True)
        else:
            pipe._e2e_out_sums[slot].copy_(pipe.res_sums, non_blocking=True)
            pipe._e2e_out_dec[slot].copy_(pipe.out_decision, non_blocking=True)
            pipe._e2e_out_counts[slot].copy_(pipe._counts, non_blocking=True)

    def h2d_desc(s):
        dev_bufs[s % nslots].copy_(host_bufs[s % nhost], non_blocking=True)

    def h2d_payload(s):
        pipe.payloads[s % nslots].copy_(pipe._e2e_payloads[s % len(pipe._e2e_payloads)],
                                        non_blocking=True)

    desc_bytes = dev_bufs[0].numel()
    h2d_bytes = desc_bytes + pipe.payloads[0].numel() * 4
    out["descriptor_bytes_per_step"] = desc_bytes
    out["descriptor_bytes_per_job"] = round(desc_bytes / B, 2)
    out["h2d_bytes_per_step"] = h2d_bytes
    out["h2d_us_per_step"] = [timed(h2d) for _ in range(3)]
    out["h2d_GBps"] = round(h2d_bytes / (min(out["h2d_us_per_step"]) * 1e-6) / 1e9, 1)
    # the two copies of a step on their own: what each costs beyond its bytes
    out["h2d_descriptors_us"] = [timed(h2d_desc) for _ in range(3)]
    out["h2d_payload_us"] = [timed(h2d_payload) for _ in range(3)]
    out["d2h_us_per_step"] = [timed(d2h) for _ in range(3)]
    out["graph_replay_us_per_step"] = [timed(lambda s: graphs[s % nslots].replay())
                                       for _ in range(3)]
    out["submit_us_per_step"] = [round(r[0], 1) for r in runs]
    out["submit_plus_drain_us_per_step"] = [round(r[1], 1) for r in runs]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
