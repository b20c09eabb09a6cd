#!/usr/bin/env python3
"""Time the assembly of a training batch from raw frames and events on the GPU, new route against old, in one process.

  new: refid_amd.data.DeviceBatchAssembler (csrc/sample.hip): events voxelised inside the crop only, 64-bit fixed-point
       integer atomics, one launch set per batch.
  old: refid_amd.data.events_to_voxel_grid on the whole frame per sample (float64 normalisation, fp32 float atomics), then
       torch crop / flip / transpose / stack for the voxel and the frames -- what a user had to write before.

Default shape: the shipped training set-up, B=8 samples of 25 frames 720x1280 (blur0, blur1, 23 sharp), crop 256, m=11,
n=1, with synthetic events uniform over the frame at two densities (2 M and 20 M per sample).  Raw inputs are already in
device memory for both routes (the upload is the same for both and is not timed).  The two routes alternate; each timing
is a device-event pair around `--reps` back-to-back calls after a warm-up.  Each stage of the new route (memset,
scatter, finish, frames) is also timed alone, `--reps` launches of it between one event pair, and the scatter kernel is
reported with its 64-bit integer atomic adds per second.
Prints one JSON line and writes it to --out.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from refid_amd import _lib  # noqa: E402
from refid_amd.data import DeviceBatchAssembler, events_to_voxel_grid, sliding_bin_pairs  # noqa: E402


def make_batch(args, n_events, gen):
    dev = "cuda"
    F = 2 * args.m + args.n + 2
    samples = []
    for b in range(args.batch):
        frames = torch.randint(0, 256, (F, args.height, args.width, 3), dtype=torch.uint8, device=dev, generator=gen)
        t = torch.sort(torch.rand(n_events, device=dev, generator=gen) * 0.5)[0]
        ev = torch.stack([t, torch.randint(0, args.width, (n_events,), device=dev, generator=gen).float(),
                          torch.randint(0, args.height, (n_events,), device=dev, generator=gen).float(),
                          torch.randint(0, 2, (n_events,), device=dev, generator=gen).float()], dim=1).contiguous()
        top = int(torch.randint(0, args.height - args.crop + 1, (1,), generator=gen, device=dev))
        left = int(torch.randint(0, args.width - args.crop + 1, (1,), generator=gen, device=dev))
        samples.append(dict(frames=frames, events=ev, first_stamp=float(ev[0, 0]), last_stamp=float(ev[-1, 0]), top=top,
                            left=left, hflip=b & 1, vflip=(b >> 1) & 1, rot90=(b >> 2) & 1))
    return samples


def old_route(samples, m, n, crop):
    bins = 2 * m + n + 1
    lqs, voxels, gts = [], [], []
    for s in samples:
        H, W = s["frames"].shape[1:3]
        vox = events_to_voxel_grid(s["events"], bins, W, H)                     # whole frame
        y, x = s["top"], s["left"]

        def aug(t):                                                            # (..., H, W) -> cropped, flipped, transposed
            t = t[..., y:y + crop, x:x + crop]
            if s["hflip"]:
                t = t.flip(-1)
            if s["vflip"]:
                t = t.flip(-2)
            if s["rot90"]:
                t = t.transpose(-1, -2)
            return t

        vox = aug(vox)
        img = aug(s["frames"].permute(0, 3, 1, 2)).flip(1).float() / 255.0       # BGR -> RGB, CHW
        lqs.append(torch.cat([img[0], vox[1:m], img[1], vox[m + 2 + n:]], dim=0))
        voxels.append(sliding_bin_pairs(vox))
        gts.append(img[2:])
    return {"lq": torch.stack(lqs), "voxel": torch.stack(voxels), "gt": torch.stack(gts)}


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def count_atomics(samples, bins, crop):
    total = 0
    for s in samples:
        ev = s["events"]
        first, last = ev[0, 0], ev[-1, 0]
        ts = (float(bins - 1) * (ev[:, 0] - first)) / (last - first)
        x, y = ev[:, 1].long() - s["left"], ev[:, 2].long() - s["top"]
        keep = (ts >= 0) & (ts < bins) & (x >= 0) & (x < crop) & (y >= 0) & (y < crop)
        total += int(keep.sum()) + int((keep & (ts.long() + 1 < bins)).sum())
    return total


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--crop", type=int, default=256)
    ap.add_argument("--m", type=int, default=11)
    ap.add_argument("--n", type=int, default=1)
    ap.add_argument("--events", type=int, nargs="+", default=[2_000_000, 20_000_000], help="events per sample")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="alternations new / old")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_assemble_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_assemble.py needs the GPU (there is no CPU path)")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    bins = 2 * args.m + args.n + 1
    asm = DeviceBatchAssembler(args.m, args.n, "blur", args.crop)
    result = {"bench": "sample_assemble", "device": torch.cuda.get_device_name(0), "batch": args.batch,
              "frame": [args.height, args.width], "frames_per_sample": bins + 1, "crop": args.crop, "m": args.m, "n": args.n,
              "reps": args.reps, "rounds": args.rounds,
              "scratch_bytes_zeroed_new": args.batch * bins * args.crop * args.crop * 8,
              "voxel_bytes_zeroed_old": args.batch * bins * args.height * args.width * 4, "densities": []}
    for n_events in args.events:
        samples = make_batch(args, n_events, gen)
        new = lambda: asm(samples)                                                  # noqa: E731
        old = lambda: old_route(samples, args.m, args.n, args.crop)                 # noqa: E731
        a, b = new(), old()                                                         # warm-up, and what the routes disagree by
        diff = {k: float((a[k] - b[k]).abs().max()) for k in ("lq", "voxel", "gt")}
        new(), old()
        t_new, t_old = [], []
        for _ in range(args.rounds):
            t_new.append(timed(new, args.reps))
            t_old.append(timed(old, args.reps))
        out = asm(samples)                                                          # keeps the outputs rerun() writes to alive
        stage_ms = {}
        for name, stage in (("zero", _lib.ASSEMBLE_ZERO), ("scatter", _lib.ASSEMBLE_SCATTER),      # scatter: the sums grow,
                            ("finish", _lib.ASSEMBLE_FINISH), ("frames", _lib.ASSEMBLE_FRAMES)):   # integers do not care
            asm.rerun(stage)
            stage_ms[name] = statistics.median(timed(lambda: asm.rerun(stage), args.reps) for _ in range(args.rounds))
        atomics = count_atomics(samples, bins, args.crop)
        sc = stage_ms["scatter"]
        result["densities"].append({
            "events_per_sample": n_events, "atomic_adds_per_batch": atomics,
            "new_ms": statistics.median(t_new), "new_ms_min_max": [min(t_new), max(t_new)],
            "old_ms": statistics.median(t_old), "old_ms_min_max": [min(t_old), max(t_old)],
            "speedup_old_over_new": statistics.median(t_old) / statistics.median(t_new),
            "stage_ms": stage_ms, "int64_atomic_adds_per_s": atomics / (sc * 1e-3),
            "events_read_per_s": args.batch * n_events / (sc * 1e-3),
            "max_abs_diff_new_vs_old": diff})
        del samples, a, b, out
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
