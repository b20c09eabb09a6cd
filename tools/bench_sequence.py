#!/usr/bin/env python3
"""Time SequenceInterpolator.run end to end against the forward passes alone, in one process.

Workload: a synthetic 1280x720 sharp sequence, n = 7, 16 pairs, max_minibatch 2, released-size network (base 32
channels, random weights).
  (a) run, PNG writing off: upload, pair assembly on the side stream, forward, crop + val_tail.
  (b) run, PNG writing on: the same plus the device->host copy and the PNG writer pool.
  (c) the forward passes alone, on the same minibatches kept resident on the device.
Output frames/s = pairs * n / wall time of one call (synchronised wall clock, after a warm-up), the median of
`--rounds` rounds with min-max; the routes alternate.  forward_share = (c) / (a): 1.0 means the assembly and the tail hide
entirely behind the forward passes.  Prints one JSON line and writes it to --out.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from refid_amd import sequence  # noqa: E402
from refid_amd.archs import define_network  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--n", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--max-minibatch", type=int, default=2)
    ap.add_argument("--base", type=int, default=32)
    ap.add_argument("--events-per-pair", type=int, default=400000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequence_interpolate_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sequence.py needs the GPU (there is no CPU path)")
    H, W, n, P, mb = args.height, args.width, args.n, args.pairs, args.max_minibatch
    rng = np.random.Generator(np.random.PCG64(1))
    low = rng.integers(0, 256, (P + 1, H // 16 + 1, W // 16 + 1, 3), dtype=np.uint8)
    frames = np.ascontiguousarray(np.repeat(np.repeat(low, 16, axis=1), 16, axis=2)[:, :H, :W])     # blocky, compressible
    E = args.events_per_pair * P
    ev = np.stack([np.sort(rng.uniform(0.0, float(P), E)), rng.integers(0, W, E), rng.integers(0, H, E),
                   rng.integers(0, 2, E)], axis=1).astype(np.float32)
    pairs = sequence.make_pairs(ev[:, 0], *sequence.sharp_windows(np.arange(P + 1, dtype=np.float64)))
    torch.manual_seed(1)
    net = define_network(dict(type="FinalBidirectionAttenfusion", img_chn=6, ev_chn=2, num_encoders=3,
                              base_num_channels=args.base, num_block=1)).to("cuda")
    interp = sequence.SequenceInterpolator(net, 1, n, "sharp", max_minibatch=mb)
    tmp = tempfile.TemporaryDirectory(prefix="refid_sequence_bench_")
    # the same minibatches, resident: what the forward passes alone cost
    asm = sequence.SequenceAssembler(1, n, "sharp", multiple=8).load(frames, ev)
    resident = [asm.assemble(pairs[i:i + mb]) for i in range(0, P, mb)]

    def forward_only():
        net.eval()
        with torch.no_grad():
            for b in resident:
                net(x=b["lq"], event=b["voxel"])

    routes = {"run_png_off": lambda: interp.run(frames, ev, pairs),
              "run_png_on": lambda: interp.run(frames, ev, pairs, out_dir=tmp.name),
              "forward_only": forward_only}
    for fn in routes.values():                               # warm-up (kernel attributes, pinned buffers, page cache)
        fn()
    times = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            times[k].append(wall(fn))
    frames_out = P * n
    fps = {k: {"median_fps": frames_out / statistics.median(v), "min_max_fps": [frames_out / max(v), frames_out / min(v)],
               "median_s": statistics.median(v)} for k, v in times.items()}
    result = {"bench": "sequence_interpolate", "device": torch.cuda.get_device_name(0), "frame": [H, W], "n": n, "pairs": P,
              "max_minibatch": mb, "base_num_channels": args.base, "events": int(E), "rounds": args.rounds,
              "output_frames_per_call": frames_out, "routes": fps,
              "forward_share_png_off": statistics.median(times["forward_only"]) / statistics.median(times["run_png_off"]),
              "forward_share_png_on": statistics.median(times["forward_only"]) / statistics.median(times["run_png_on"])}
    tmp.cleanup()
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
