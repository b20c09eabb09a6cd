#!/usr/bin/env python3
"""Time the assembly of a single-image deblurring batch (lq, normalised voxel, gt) on the GPU, new route against what a
user had to write before, alternating in one process.

  new: refid_amd.data.DeviceBatchAssembler(layout='single') (csrc/sample.hip): events voxelised inside the crop only,
       voxel_norm as a two-pass reduction on the device, five launches per batch.
  old: refid_amd.data.events_to_voxel_grid on the whole frame per sample, torch crop / flip / transpose for the voxel and
       the two frames, and voxel_norm (event_util.py:141-160) written in torch on the device, per sample.

Default shape: B=8 samples of 2 frames 720x1280 (blur, sharp), crop 256, 6 bins, synthetic events uniform over the frame.
Raw inputs are in device memory for both routes.  Each timing is a device-event pair around `--reps` back-to-back calls
after a warm-up; the stages of the new route are also timed alone.  Prints one JSON line and writes it to --out.  Needs
the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from refid_amd import _lib  # noqa: E402
from refid_amd.data import DeviceBatchAssembler, events_to_voxel_grid  # noqa: E402


def make_batch(args, gen):
    dev = "cuda"
    samples = []
    for b in range(args.batch):
        frames = torch.randint(0, 256, (2, args.height, args.width, 3), dtype=torch.uint8, device=dev, generator=gen)
        t = torch.sort(torch.rand(args.events, device=dev, generator=gen) * 0.5)[0]
        ev = torch.stack([t, torch.randint(0, args.width, (args.events,), device=dev, generator=gen).float(),
                          torch.randint(0, args.height, (args.events,), device=dev, generator=gen).float(),
                          torch.randint(0, 2, (args.events,), device=dev, generator=gen).float()], dim=1).contiguous()
        top = int(torch.randint(0, args.height - args.crop + 1, (1,), generator=gen, device=dev))
        left = int(torch.randint(0, args.width - args.crop + 1, (1,), generator=gen, device=dev))
        samples.append(dict(frames=frames, events=ev, first_stamp=float(ev[0, 0]), last_stamp=float(ev[-1, 0]), top=top,
                            left=left, hflip=b & 1, vflip=(b >> 1) & 1, rot90=(b >> 2) & 1))
    return samples


def torch_voxel_norm(voxel):
    """event_util.py:141-160, on the device."""
    nonzero = voxel != 0
    num = nonzero.sum()
    if num > 0:
        mean = voxel.sum() / num
        std = torch.sqrt((voxel ** 2).sum() / num - mean ** 2)
        voxel = nonzero.float() * (voxel - mean) / std
    return voxel


def old_route(samples, bins, crop):
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

        img = aug(s["frames"].permute(0, 3, 1, 2)).flip(1).float() / 255.0       # BGR -> RGB, CHW
        lqs.append(img[0])
        gts.append(img[1])
        voxels.append(torch_voxel_norm(aug(vox).contiguous()))
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--crop", type=int, default=256)
    ap.add_argument("--bins", type=int, default=6)
    ap.add_argument("--events", type=int, default=2_000_000, help="events per sample")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="alternations new / old")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "single_assemble_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_single_assemble.py needs the GPU (there is no CPU path)")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    asm = DeviceBatchAssembler(layout="single", num_bins=args.bins, gt_size=args.crop)
    samples = make_batch(args, gen)
    new = lambda: asm(samples)                                                      # noqa: E731
    old = lambda: old_route(samples, args.bins, args.crop)                          # noqa: E731
    a, b = new(), old()                                                             # warm-up, and what the routes disagree by
    diff = {k: float((a[k] - b[k]).abs().max()) for k in ("lq", "voxel", "gt")}
    new(), old()
    t_new, t_old = [], []
    for _ in range(args.rounds):
        t_new.append(timed(new, args.reps))
        t_old.append(timed(old, args.reps))
    out = asm(samples)                                                              # keeps the outputs rerun() writes to alive
    stage_ms = {}
    for name, stage in (("zero", _lib.ASSEMBLE_ZERO), ("scatter", _lib.ASSEMBLE_SCATTER), ("stats", _lib.ASSEMBLE_STATS),
                        ("finish", _lib.ASSEMBLE_FINISH), ("frames", _lib.ASSEMBLE_FRAMES)):
        asm.rerun(stage)
        stage_ms[name] = statistics.median(timed(lambda: asm.rerun(stage), args.reps) for _ in range(args.rounds))
    result = {"bench": "single_assemble", "device": torch.cuda.get_device_name(0), "batch": args.batch,
              "frame": [args.height, args.width], "crop": args.crop, "bins": args.bins, "events_per_sample": args.events,
              "reps": args.reps, "rounds": args.rounds,
              "new_ms": statistics.median(t_new), "new_ms_min_max": [min(t_new), max(t_new)],
              "old_ms": statistics.median(t_old), "old_ms_min_max": [min(t_old), max(t_old)],
              "speedup_old_over_new": statistics.median(t_old) / statistics.median(t_new),
              "stage_ms": stage_ms, "max_abs_diff_new_vs_old": diff}
    del out
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
