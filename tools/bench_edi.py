#!/usr/bin/env python3
"""Time the event-based double integral (csrc/edi.hip, refid_amd.edi) at 1280x720 on simulated events.

The clip is synthetic: one frame of tools/bench_png_decode.py's ``content`` (smooth waves, hard edges, sensor-like noise)
panning 2 pixels per frame, 49 frames at 240 fps, made on the device; its events come from ``EventSimulator`` (c = 0.2) and
are packed once by ``EdiStream.load``, which is timed on its own.  Two cases, the pairs of the clip in minibatches of 2
through ``ops.edi`` into a preallocated ``out``, as ``EdiInterpolator`` launches them:
  sharp_n7      every 8th frame is a key frame, 7 frames between two keys;
  blur_m11_n1   blurry keys of M = 11 frames with a gap of 1 (``blur_synth``), 2 M + N = 23 frames per pair.
Each figure is the median of ``--rounds`` windows after a warm-up, with min-max; a window is ``--repeats`` passes over all
pairs between two device events.
  ms_per_pair     one pair's share of a pass;
  bytes_per_pair  what the algorithm must move: two key frames read, the output frames written, the pair's packed events
                  (a 4-byte stamp and a 1-byte sign each, those between s0 and e1) read once, the 4-byte segment starts;
  fraction_of_copy_rate   bytes_per_pair / ms_per_pair over the copy rate profiles/blur_synth_bench.json records (6.3 TB/s);
  all_pairs_in_one_launch   the same two figures with every pair of the clip in ONE ``ops.edi`` call: the host's share of a
                  call (the tables it builds and uploads) spread over more work.
A 64 x 8 crop of the first pair of each case is compared with tests/edi_ref.py (pixels are independent, so the crop's
events alone give the crop).  No threshold is asserted: nothing did this work before.  Prints one JSON line and writes it
to --out (profiles/edi_bench.json).  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import edi_ref as R  # noqa: E402
from bench_blur_synth import COPY_RATE, timed  # noqa: E402
from bench_png_decode import content, stat  # noqa: E402
from refid_amd import blur_synth, edi, event_sim, ops  # noqa: E402

CROP = (100, 108, 200, 264)            # rows, columns of the check


def crop_check(keys, events, items, bounds, instants, m, c, got):
    """Whether the device's frames of the first item equal the restatement on the crop."""
    y0, y1, x0, x1 = CROP
    ev = events.cpu().numpy()
    x, y = np.trunc(ev[:, 1]), np.trunc(ev[:, 2])
    ev = ev[(x >= x0) & (x < x1) & (y >= y0) & (y < y1)].copy()
    ev[:, 1] -= x0
    ev[:, 2] -= y0
    small = keys[:, y0:y1, x0:x1].cpu().numpy()
    want, _ = R.edi(small, R.load(ev, y1 - y0, x1 - x0), items[:1], bounds[:1], instants[:1], m, R.SAMPLES, c, c)
    return bool(got[:1, :, y0:y1, x0:x1].cpu().numpy().tobytes() == want.tobytes())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=49)
    ap.add_argument("--size", default="720x1280")
    ap.add_argument("--c", type=float, default=0.2, help="both contrast thresholds")
    ap.add_argument("--repeats", type=int, default=10, help="passes over all pairs per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edi_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_edi.py needs the GPU (there is no CPU path)")
    h, w = (int(v) for v in args.size.split("x"))
    n, c = args.frames, event_sim.to_fixed(args.c)
    base = torch.from_numpy(content(1, h, w, 7)[0]).cuda()
    frames = torch.stack([torch.roll(base, shifts=2 * k, dims=1) for k in range(n)]).contiguous()
    stamps = np.arange(n, dtype=np.float64) / 240.0
    events, _ = event_sim.EventSimulator(h, w, c_pos=args.c, c_neg=args.c).simulate(frames, stamps, chunk=8)
    stream = edi.EdiStream().load(events, h, w)
    torch.cuda.synchronize()
    t_load = timed(lambda: edi.EdiStream().load(events, h, w), 3, args.rounds)
    frame_bytes = h * w * 3
    t_all = events[:, 0].cpu().numpy()
    result = {"bench": "edi", "device": torch.cuda.get_device_name(0), "frame": [h, w, 3], "frames": n, "c": args.c,
              "events": int(events.shape[0]), "events_per_pixel_and_interval": events.shape[0] / (h * w * (n - 1)),
              "repeats_per_window": args.repeats, "rounds": args.rounds, "copy_rate": COPY_RATE,
              "stream_pack": {"ms": stat(t_load, 1e3), "note": "EdiStream.load of all events: a stable sort by pixel, once per sequence"}}

    cases = {}
    s = stamps[::8]
    cases["sharp_n7"] = (frames[::8].contiguous(), np.array([[s[k], s[k], s[k + 1], s[k + 1]] for k in range(len(s) - 1)], dtype=np.float32),
                         "sharp", 1, 7)
    windows, _ = blur_synth.blur_windows(n, 11, 1)
    expo = blur_synth.exposures(stamps, windows)
    cases["blur_m11_n1"] = (ops.blur_synth(frames, windows), np.array([[expo[k, 0], expo[k, 1], expo[k + 1, 0], expo[k + 1, 1]]
                                                                        for k in range(len(expo) - 1)], dtype=np.float32), "blur", 11, 1)
    for name, (keys, bounds, layout, m, between) in cases.items():
        pairs = len(bounds)
        items = np.array([[k, k + 1] for k in range(pairs)])
        instants = np.stack([edi.output_instants(layout, b, m, between) for b in bounds])
        t_out = instants.shape[1]
        out = torch.empty((pairs, t_out, h, w, 3), dtype=torch.uint8, device="cuda")

        def one_pass():
            for at in range(0, pairs, 2):
                ops.edi(keys, stream, items[at:at + 2], bounds[at:at + 2], instants[at:at + 2], m=m, c_pos=c, c_neg=c, out=out[at:at + 2])

        def one_launch():
            ops.edi(keys, stream, items, bounds, instants, m=m, c_pos=c, c_neg=c, out=out)

        t = [v / pairs for v in timed(one_pass, args.repeats, args.rounds)]
        t_one = [v / pairs for v in timed(one_launch, args.repeats, args.rounds)]
        med = statistics.median(t)
        in_pair = [int(np.searchsorted(t_all, b[3], "right") - np.searchsorted(t_all, b[0], "right")) for b in bounds]
        moved = 2 * frame_bytes + t_out * frame_bytes + 5 * statistics.mean(in_pair) + 4 * (h * w + 1)
        one_pass()
        held = int(ops.edi(keys, stream, items[:1], bounds[:1], instants[:1], m=m, c_pos=c, c_neg=c)[1].sum())
        result[name] = {"pairs": pairs, "frames_per_pair": t_out, "ms_per_pair": stat(t, 1e3), "output_frames_per_s": t_out / med,
                        "events_per_pair": statistics.mean(in_pair), "bytes_per_pair": moved, "bytes_per_s": moved / med,
                        "fraction_of_copy_rate": moved / med / COPY_RATE, "all_pairs_in_one_launch": {
                            "ms_per_pair": stat(t_one, 1e3), "fraction_of_copy_rate": moved / statistics.median(t_one) / COPY_RATE},
                        "clamped_pixels_first_pair": held,
                        "crop_equals_the_restatement": crop_check(keys, events, items, bounds, instants, m, c, out)}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
