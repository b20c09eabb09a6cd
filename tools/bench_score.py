#!/usr/bin/env python3
"""Device time of refid_score_u8 (csrc/score.hip) per frame, at 720x1280 and 1224x1632: each of the four outputs alone and all
four together, alternated round by round with refid_val_tail's PSNR + SSIM on the same frames (the fused tail that takes
the network's float32 output; it also writes the uint8 frames).  Device events around ``--iters`` back-to-back calls, the
median of ``--rounds`` rounds; the buffers are allocated once, outside the timed region.  Writes profiles/score_bench.json.

No target is fixed in advance: the 121-tap float64 filter is about 1.1 GFLOP per 720p frame.  The reference has no GPU
route for these scores (its ``test_y_channel`` path is numpy + cv2 on the host), so there is nothing of its to time here,
and this tool does not read the reference.

    python tools/bench_score.py [--frames 4] [--iters 10] [--rounds 5] [--out profiles/score_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SIZES = ((720, 1280), (1224, 1632))
MODES = (("psnr", (1, 0, 0, 0)), ("psnr_y", (0, 1, 0, 0)), ("ssim3d", (0, 0, 1, 0)), ("ssim_y", (0, 0, 0, 1)), ("all_four", (1, 1, 1, 1)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--crop-border", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "score_bench.json"))
    args = ap.parse_args()

    import torch
    from refid_amd._lib import check, lib
    L = lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nf, cb = args.frames, args.crop_border
    result = dict(device=torch.cuda.get_device_name(0), frames_per_call=nf, iters=args.iters, rounds=args.rounds, crop_border=cb,
                  unit="ms per frame, device events, median of rounds", sizes={},
                  not_measured=["the command line end to end (PNG decode + scoring)", "FrameScorer inside a sequence run",
                                "frame counts other than --frames", "the reference: it has no GPU route for these scores"])

    def timed(call):
        call()                                              # warm-up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / (args.iters * nf)

    for h, w in SIZES:
        g = torch.Generator(device="cuda").manual_seed(1)
        gt_f = torch.rand((nf, 3, h, w), device="cuda", generator=g)
        pred_f = (gt_f + 0.02 * torch.randn((nf, 3, h, w), device="cuda", generator=g)).clamp(0, 1)
        pred_u8 = torch.empty((nf, h, w, 3), dtype=torch.uint8, device="cuda")
        gt_u8 = torch.empty_like(pred_u8)
        tail_buf = torch.empty(2 * nf + L.refid_val_tail_parts(nf, h, w), dtype=torch.int64, device="cuda")
        buf = torch.empty(4 * nf + L.refid_score_u8_parts(nf, h, w, cb), dtype=torch.int64, device="cuda")

        def tail():
            check(L.refid_val_tail(pred_f.data_ptr(), gt_f.data_ptr(), nf, h, w, 0, pred_u8.data_ptr(), gt_u8.data_ptr(),
                                   tail_buf.data_ptr(), tail_buf[nf:].data_ptr(), tail_buf[2 * nf:].data_ptr(), st), "refid_val_tail")

        def scorer(mask):
            ptrs = [buf[i * nf:].data_ptr() if on else None for i, on in enumerate(mask)]

            def call():
                check(L.refid_score_u8(pred_u8.data_ptr(), gt_u8.data_ptr(), nf, h, w, 0, cb, *ptrs, buf[4 * nf:].data_ptr(),
                                       None, None, st), "refid_score_u8")
            return call

        tail()                                              # fills the uint8 frames the scorer reads
        calls = [("val_tail_psnr_ssim", tail)] + [(name, scorer(mask)) for name, mask in MODES]
        times = {name: [] for name, _ in calls}
        for _ in range(args.rounds):
            for name, call in calls:                        # alternated: every round times every variant once
                times[name].append(timed(call))
        torch.cuda.synchronize()
        same = bool((buf[:nf] == tail_buf[:nf]).all()) and bool((buf[2 * nf:3 * nf] == tail_buf[nf:2 * nf]).all())
        result["sizes"][f"{h}x{w}"] = dict({name: round(statistics.median(v), 5) for name, v in times.items()},
                                           rounds={name: [round(x, 5) for x in v] for name, v in times.items()},
                                           psnr_ssim_words_equal_val_tail=same)
        print(f"{h}x{w}: " + ", ".join(f"{name} {statistics.median(v):.4f}" for name, v in times.items()) +
              f" ms/frame; PSNR / SSIM words equal val_tail's: {same}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
