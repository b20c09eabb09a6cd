#!/usr/bin/env python3
"""Time SequenceInterpolator.run end to end against the forward passes alone, in one process.

Workload: a synthetic 1280x720 sharp sequence, n = 7, 16 pairs, max_minibatch 2, released-size network (base 32
channels, random weights).
  (a) run, PNG writing off: upload, pair assembly on the side stream, forward, crop + val_tail.
  (b) run, PNG writing on: the same plus the device->host copy and the PNG writer pool.
  (c) the forward passes alone, on the same minibatches kept resident on the device.
Output frames/s = pairs * n / wall time of one call (synchronised wall clock, after a warm-up), the median of
`--rounds` rounds with min-max; the routes alternate.  forward_share = (c) / (a): 1.0 means the assembly and the tail hide
entirely behind the forward passes.  Prints one JSON line and writes it to --out.  Needs the GPU: there is no CPU path.

``--layout single`` times the single-image assembly instead (``single_assembly`` below): ms per item at 1280x720, 6 bins,
for ``SequenceAssembler(layout='single')`` and for ``DeviceBatchAssembler(layout='single')`` with a per-item upload."""
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


def single_assembly(args):
    """--layout single: assembly alone, per item, at 6 bins.  (a) SequenceAssembler(layout='single'): the sequence resident,
    one launch set for all items.  (b) what the parent commit offers for the same inputs: DeviceBatchAssembler(
    layout='single', gt_size=None) fed whole frames (the blurry frame twice: it wants a ground truth) and per-item event
    slices from pinned host memory, uploaded on every call.  Same items, same outputs up to the padding; the routes
    alternate.  No threshold: this is a capability, and the comparison only says what it costs."""
    from refid_amd.data import DeviceBatchAssembler
    H, W, P, bins = args.height, args.width, args.pairs, args.num_bins
    rng = np.random.Generator(np.random.PCG64(2))
    low = rng.integers(0, 256, (P, H // 16 + 1, W // 16 + 1, 3), dtype=np.uint8)
    frames = np.ascontiguousarray(np.repeat(np.repeat(low, 16, axis=1), 16, axis=2)[:, :H, :W])
    E = args.events_per_pair * P
    ev = np.stack([np.sort(rng.uniform(0.0, float(P), E)), rng.integers(0, W, E), rng.integers(0, H, E),
                   rng.integers(0, 2, E)], axis=1).astype(np.float32)
    starts = np.arange(P, dtype=np.float64)
    items = sequence.make_pairs(ev[:, 0], *sequence.frame_windows(starts, starts + 1.0))
    asm = sequence.SequenceAssembler(layout="single", num_bins=bins, multiple=4).load(frames, ev)
    fr_pin, ev_pin = torch.from_numpy(frames).pin_memory(), torch.from_numpy(ev).pin_memory()
    raw = [dict(frames=fr_pin[[p.left, p.left]].pin_memory(), events=ev_pin[p.row0:p.row1], first_stamp=p.first_stamp,
                last_stamp=p.last_stamp) for p in items]
    dba = DeviceBatchAssembler(layout="single", num_bins=bins, gt_size=None)
    routes = {"sequence_resident": lambda: asm.assemble(items), "batch_assembler_upload_per_item": lambda: dba(raw)}
    for fn in routes.values():
        fn()
    calls = args.calls                                        # one call is a few ms: a timed window holds many of them
    times = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            times[k].append(wall(lambda: [fn() for _ in range(calls)]))
    n = calls * P
    per_item = {k: {"median_ms_per_item": 1e3 * statistics.median(v) / n, "min_max_ms_per_item": [1e3 * min(v) / n, 1e3 * max(v) / n],
                    "median_window_s": statistics.median(v)} for k, v in times.items()}
    return {"bench": "sequence_single_assembly", "device": torch.cuda.get_device_name(0), "frame": [H, W], "num_bins": bins,
            "items": P, "events": int(E), "rounds": args.rounds, "calls_per_window": calls, "routes": per_item}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layout", choices=("sharp", "single"), default="sharp",
                    help="sharp: SequenceInterpolator end to end (below); single: the single-image assembly per item")
    ap.add_argument("--num-bins", type=int, default=6, help="--layout single: voxel bins")
    ap.add_argument("--calls", type=int, default=50, help="--layout single: assembly calls per timed window")
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--n", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--max-minibatch", type=int, default=2)
    ap.add_argument("--base", type=int, default=32)
    ap.add_argument("--events-per-pair", type=int, default=400000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", help="default: profiles/sequence_interpolate_bench.json, or profiles/seq_single_bench.json "
                                  "with --layout single")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sequence.py needs the GPU (there is no CPU path)")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "seq_single_bench.json" if args.layout == "single"
                                else "sequence_interpolate_bench.json")
    if args.layout == "single":
        return write_result(single_assembly(args), args.out)
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
    write_result(result, args.out)


def write_result(result, path):
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
