#!/usr/bin/env python3
"""Train-step time of the compute modes against each other, in ONE process: bench.py's configs[1] workload (its model options,
synthetic batch and defaults: B=8, 256x256, T=23, imported from bench, not copied) with compute_dtype bf16 / fp16 / fp32.

bench.py's --dtype choices are part of the measuring contract and do not list 'fp16'; this tool is where that mode's step time
comes from.  Protocol: every mode is built and warmed up at size (--warmup steps), then the modes ALTERNATE in blocks of --steps
train steps (--alternations rounds: bf16, fp16, fp32, bf16, ...), each block bracketed by a device synchronise.  A mode's figure
is the median over its blocks of the block's ms/step; the spread is the blocks' min .. max.  Comparing modes inside one run
on one device is what makes a few-percent difference readable: the machine's drift lands on all of them.

Not bench.py's default line: the batch is ONE device-resident synthetic batch fed again every step (bench.py's default path
draws pinned host batches through its prefetcher), and all modes' models stay resident side by side (three B=8 models and
their workspaces).  The fp32 figure is comparable with bench.py's to the extent that the host-to-device copy hides under the
step there; the JSON line says so in "differs_from_bench".

Prints one JSON line.  Needs the GPU (no fallback)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import bench


def build_model(args, mode):
    from refid_amd.train import TwoImageEventRecurrentRestorationModel
    args.dtype = mode                                        # (bench.options reads it; set past bench's own --dtype choices)
    torch.manual_seed(1234)                                  # bench.main's initialisation
    model = TwoImageEventRecurrentRestorationModel(bench.options(args))
    with torch.no_grad():
        for k, p in model.net_g.named_parameters():
            if k.endswith((".beta", ".gamma")):
                p.normal_(0.0, 0.1)
    model.net_g.notify_params_changed()
    model.set_graph_mode("auto")                             # bench.py's default (--graph auto)
    return model


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--modes", default="bf16,fp16,fp32")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=None, help="default: bench.py's")
    ap.add_argument("--size", type=int, default=None, help="default: bench.py's")
    ap.add_argument("--T", type=int, default=None, help="default: bench.py's")
    o = ap.parse_args(argv)
    if o.alternations < 3 or o.steps < 5:
        ap.error("at least 3 alternations of at least 5 steps (fewer says nothing about the spread)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_compute_dtype.py needs a ROCm GPU (the HIP path has no CPU fallback)")
    args = bench.parse_args([])                              # configs[1]: bench.py's own defaults
    for k in ("batch", "size", "T"):
        if getattr(o, k) is not None:
            setattr(args, k, getattr(o, k))
    modes = o.modes.split(",")
    dev = torch.device("cuda", 0)
    x, ev, gt = bench.synthetic_batch(args.batch, args.T, args.size, args.size, args.img_chn, 100, dev)
    batch = {"lq": x, "voxel": ev, "gt": gt}
    models, its, loss = {}, {}, {}
    for m in modes:
        models[m], its[m] = build_model(args, m), 0

    def steps(m, n):
        for _ in range(n):
            its[m] += 1
            models[m].feed_data(batch)
            models[m].update_learning_rate(its[m])
            models[m].optimize_parameters(its[m])
        torch.cuda.synchronize()
        loss[m] = float(models[m].get_current_log()["l_pix"])

    for m in modes:                                          # warm-up at size: code objects, workspaces, allocator
        steps(m, o.warmup)
    blocks = {m: [] for m in modes}
    for _ in range(o.alternations):
        for m in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(m, o.steps)
            blocks[m].append((time.perf_counter() - t0) / o.steps * 1e3)
    res = {}
    for m in modes:
        med = statistics.median(blocks[m])
        res[m] = {"ms_per_step": round(med, 2), "min": round(min(blocks[m]), 2), "max": round(max(blocks[m]), 2),
                  "blocks_ms_per_step": [round(b, 2) for b in blocks[m]],
                  "frames_per_s": round(args.batch * args.T / (med * 1e-3), 1), "loss": loss[m],
                  "graph_replay": bool(getattr(models[m], "graph_on", False))}
    line = {"metric": "train step ms/step per compute_dtype, alternating blocks in one process",
            "workload": {"batch": args.batch, "size": args.size, "T": args.T, "img_chn": args.img_chn},
            "protocol": {"warmup_steps": o.warmup, "alternations": o.alternations, "steps_per_block": o.steps, "order": modes,
                         "figure": "median over a mode's blocks of the block's ms/step; spread = min .. max of the blocks"},
            "differs_from_bench": "one device-resident batch re-fed every step (no pinned-host prefetcher); all modes' models resident at once",
            "device": torch.cuda.get_device_name(0), "modes": res}
    if "bf16" in res and "fp16" in res:
        line["fp16_over_bf16"] = round(res["fp16"]["ms_per_step"] / res["bf16"]["ms_per_step"], 4)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
