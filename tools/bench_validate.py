#!/usr/bin/env python3
"""Time the validation of one item, new route against old, in one process.

  (a) old: what a user could assemble before -- model.test(), .cpu() of the fp32 result and gt, a numpy restatement of
      tensor2img per frame (clamp, transpose, x255, round, uint8) on one core, calculate_psnr_frames +
      calculate_ssim_frames on the device; with PNG writing on, write_png per frame on the same thread.
  (b) new: model.nondist_validation -- one fused refid_val_tail launch per item, uint8 frames to pinned memory on a side
      stream, PNGs encoded by a small thread pool behind the next item's forward pass.

Default shape: the GoPro test geometry, B=1, 720x1280, m=1, n=15 (T=17), base 32 channels, random weights; `--items` items
per timed call.  The routes alternate; each timing is a synchronised wall clock around one call after a warm-up, reported
per item as the median of `--rounds` rounds with min-max.  The tail is also timed alone with device events: the
refid_val_tail launch against refid_sqerr_u8 + refid_ssim3d_u8 on the same frames.
Prints one JSON line and writes it to --out.  Needs the GPU: there is no CPU path."""
import argparse
import ctypes as C
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
from refid_amd import _lib, metrics  # noqa: E402
from refid_amd.png import write_png  # noqa: E402
from refid_amd.train import TwoImageEventRecurrentRestorationModel  # noqa: E402


def tensor2img_numpy(frame):
    """(3, H, W) fp32 host tensor -> (H, W, 3) uint8, the steps of utils/img_util.py:90-117 (RGB kept for the PNG)."""
    img = frame.float().clamp_(0, 1).numpy().transpose(1, 2, 0)
    return (img * 255.0).round().astype(np.uint8)


def old_route(model, items, m, n, out_dir):
    book = metrics.ValidationMetrics(dict(psnr=dict(type="calculate_psnr"), ssim=dict(type="calculate_ssim")),
                                     dict(psnr=dict(type="calculate_psnr"), ssim=dict(type="calculate_ssim")), m, n)
    for data in items:
        model.feed_data(data)
        model.test()
        res, gt = model.output.detach().cpu(), model.gt.detach().cpu()
        for f in range(res.shape[1]):
            sr_img, gt_img = tensor2img_numpy(res[0, f]), tensor2img_numpy(gt[0, f])
            if out_dir:
                stem = os.path.join(out_dir, "old", data["seq"][0], f"{data['origin_index'][0]}_{f:02d}")
                write_png(stem + ".png", sr_img)
                write_png(stem + "_gt.png", gt_img)
        book.add_item({"calculate_psnr": metrics.calculate_psnr_frames(model.output[0], model.gt[0]),
                       "calculate_ssim": metrics.calculate_ssim_frames(model.output[0], model.gt[0])})
    book.finish()
    return book


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stat(xs):
    return {"median_ms": statistics.median(xs), "min_max_ms": [min(xs), max(xs)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--m", type=int, default=1)
    ap.add_argument("--n", type=int, default=15)
    ap.add_argument("--base", type=int, default=32)
    ap.add_argument("--items", type=int, default=3, help="items per timed call")
    ap.add_argument("--rounds", type=int, default=5, help="alternations old / new")
    ap.add_argument("--reps", type=int, default=10, help="launches between one event pair (tail alone)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validate_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_validate.py needs the GPU (there is no CPU path)")
    m, n, H, W = args.m, args.n, args.height, args.width
    T = 2 * m + n
    both = lambda: dict(psnr=dict(type="calculate_psnr", crop_border=0), ssim=dict(type="calculate_ssim", crop_border=0))  # noqa: E731
    tmp = tempfile.TemporaryDirectory(prefix="refid_validate_bench_")
    opt = {"name": "bench", "is_train": False, "num_gpu": 1, "dist": False,
           "network_g": dict(type="FinalBidirectionAttenfusion", img_chn=6, ev_chn=2, num_encoders=3,
                             base_num_channels=args.base, num_block=1),
           "path": {"pretrain_network_g": None, "visualization": os.path.join(tmp.name, "new")},
           "datasets": {"val": {"num_end_interpolation": m, "num_inter_interpolation": n}},
           "val": {"save_gt": True, "metrics_deblur": both(), "metrics_interpo": both()}}
    torch.manual_seed(1)
    model = TwoImageEventRecurrentRestorationModel(opt)
    gen = torch.Generator().manual_seed(2)
    items = []
    for k in range(args.items):                              # host tensors, as a DataLoader hands them over
        lq = torch.rand((1, 2, 3, H, W), generator=gen)
        ev = torch.where(torch.rand((1, T, 2, H, W), generator=gen) < 0.85, torch.zeros(()),
                         torch.round(torch.randn((1, T, 2, H, W), generator=gen) * 8) / 8)
        low = torch.nn.functional.interpolate(torch.rand((T, 3, H // 16, W // 16), generator=gen), size=(H, W), mode="bilinear")
        gt = (low + 0.02 * torch.randn((T, 3, H, W), generator=gen)).unsqueeze(0)      # smooth + sensor-like noise
        items.append({"lq": lq, "voxel": ev, "gt": gt, "seq": [f"seq{k % 2}"], "origin_index": [f"{k:06d}"]})
    routes = {
        "old_png_off": lambda: old_route(model, items, m, n, None),
        "old_png_on": lambda: old_route(model, items, m, n, tmp.name),
        "new_png_off": lambda: model.nondist_validation(items, 1, None, False, True, True),
        "new_png_on": lambda: model.nondist_validation(items, 1, None, True, True, True),
    }
    times = {k: [] for k in routes}
    for k, fn in routes.items():                             # warm-up (kernel attributes, pinned buffers, page cache)
        fn()
    a = routes["old_png_off"]()
    routes["new_png_off"]()
    agree = {"psnr_total_abs_diff": abs(a.total["psnr"] - model.metric_results_total["psnr"]),
             "ssim_total_abs_diff": abs(a.total["ssim"] - model.metric_results_total["ssim"])}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            times[k].append(wall(fn) / args.items)
    # the tail alone, on the last item's frames
    pred, gt = model.output.contiguous(), model.gt.contiguous()
    L, st = _lib.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nf, fe = T, 3 * H * W
    u8 = torch.empty((2, nf, H, W, 3), dtype=torch.uint8, device="cuda")
    words = torch.empty(2 * nf + L.refid_val_tail_parts(nf, H, W), dtype=torch.int64, device="cuda")
    b1 = torch.empty(nf + L.refid_sqerr_u8_parts(nf, fe), dtype=torch.float64, device="cuda")
    b2 = torch.empty(nf + L.refid_ssim3d_u8_parts(nf, H, W), dtype=torch.float64, device="cuda")

    def fused():                                             # launches only: no allocation, no device->host copy
        _lib.check(L.refid_val_tail(pred.data_ptr(), gt.data_ptr(), nf, H, W, 0, u8[0].data_ptr(), u8[1].data_ptr(),
                                    words.data_ptr(), words[nf:].data_ptr(), words[2 * nf:].data_ptr(), st), "refid_val_tail")

    def old_two():
        _lib.check(L.refid_sqerr_u8(pred.data_ptr(), gt.data_ptr(), nf, fe, b1.data_ptr(), b1[nf:].data_ptr(), st), "sqerr")
        _lib.check(L.refid_ssim3d_u8(pred.data_ptr(), gt.data_ptr(), nf, H, W, b2.data_ptr(), b2[nf:].data_ptr(), st), "ssim")

    fused(), old_two()
    t_fused = [timed(fused, args.reps) for _ in range(args.rounds)]
    t_two = [timed(old_two, args.reps) for _ in range(args.rounds)]
    result = {"bench": "validate", "device": torch.cuda.get_device_name(0), "frame": [H, W], "m": m, "n": n, "frames": T,
              "base_num_channels": args.base, "items_per_call": args.items, "rounds": args.rounds,
              "per_item": {k: stat(v) for k, v in times.items()},
              "ratio_new_over_old_png_off": statistics.median(times["new_png_off"]) / statistics.median(times["old_png_off"]),
              "ratio_new_over_old_png_on": statistics.median(times["new_png_on"]) / statistics.median(times["old_png_on"]),
              "tail_alone": {"val_tail": stat(t_fused), "sqerr_u8_plus_ssim3d_u8": stat(t_two), "reps": args.reps,
                             "note": "launches only; val_tail also writes both uint8 image sets"},
              "metrics_agree": agree}
    tmp.cleanup()
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
