#!/usr/bin/env python3
"""Time NIQE on the device: the moments kernels per frame, and what ``niqe=`` adds to SequenceInterpolator.run.

  (a) refid_niqe_moments alone at 1224x1632 and at 720x1280, ``--frames`` frames per call: device time per frame from
      events around ``--calls`` back-to-back calls (synchronised), the median of ``--rounds`` windows with min-max, and the
      host finish (features + score) per frame.  Beside it the numpy restatement of the same arithmetic
      (tests/niqe_ref.py) on this host, one frame, and the largest deviation of the device's sums from it.
      Algorithmic bytes per frame: 3 B per pixel of the cropped frame read, 2 * blocks * 25 * 8 B written; their rate over
      the kernel time is given as a share of the 8 TB/s HBM peak -- a measurement, not a bar: per pixel and scale the
      kernel issues 98 float64 products and 98 float64 adds for three bytes read.
  (b) SequenceInterpolator.run (720x1280, n = 3, 8 pairs, released-size network, PNG writing off) with ``niqe=model``
      against ``niqe=None``, alternating, wall clock around a synchronise.
Prints one JSON line and writes it to --out (profiles/niqe_bench.json).  Needs the GPU: there is no CPU path.  ``--params``
defaults to the test fixture's copy of the reference's niqe_pris_params.npz."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from refid_amd import niqe, sequence  # noqa: E402
from refid_amd.archs import define_network  # noqa: E402

HBM_PEAK = 8.0e12


def texture(rng, n, h, w):
    """Smooth noise plus grain: frames whose blocks all give finite features."""
    low = rng.integers(0, 256, (n, h // 8 + 2, w // 8 + 2, 3)).astype(np.float32)
    up = np.repeat(np.repeat(low, 8, axis=1), 8, axis=2)[:, :h, :w]
    return np.clip(up * 0.7 + rng.integers(0, 77, (n, h, w, 3)), 0, 255).astype(np.uint8)


def moments_bench(model, h, w, args):
    import niqe_ref as R
    rng = np.random.Generator(np.random.PCG64(h))
    frames = texture(rng, args.frames, h, w)
    u8 = torch.from_numpy(frames).cuda()
    sums = niqe.moments(u8, model)                           # warm-up: code object, LDS attribute, window upload
    torch.cuda.synchronize()
    windows = []
    for _ in range(args.rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.calls):
            niqe.moments(u8, model)
        t1.record()
        t1.synchronize()
        windows.append(t0.elapsed_time(t1) * 1e-3 / (args.calls * args.frames))
    host = sums.cpu().numpy()
    t = time.perf_counter()
    scores = niqe.finish(host, model)
    finish_s = (time.perf_counter() - t) / args.frames
    t = time.perf_counter()
    ref = R.frame_stages(frames[0], model.window)["sums"]
    numpy_s = time.perf_counter() - t
    dev = np.abs(host[0][..., 2:] - ref[..., 2:]) / np.where(ref[..., 2:] != 0, np.abs(ref[..., 2:]), 1.0)
    hc, wc = niqe.cropped_size(h, w)
    nbytes = 3 * hc * wc + 2 * (hc // 96) * (wc // 96) * 25 * 8
    med = statistics.median(windows)
    return {"frame": [h, w], "frames_per_call": args.frames, "calls_per_window": args.calls,
            "device_ms_per_frame": {"median": 1e3 * med, "min_max": [1e3 * min(windows), 1e3 * max(windows)]},
            "window_s": med * args.calls * args.frames, "host_finish_ms_per_frame": 1e3 * finish_s,
            "numpy_restatement_s_per_frame": numpy_s, "algorithmic_bytes_per_frame": nbytes,
            "algorithmic_bytes_per_s": nbytes / med, "share_of_hbm_peak_on_algorithmic_bytes": nbytes / med / HBM_PEAK,
            "counts_equal_restatement": bool(np.array_equal(host[0][..., :2], ref[..., :2])),
            "largest_relative_sum_deviation_from_restatement": float(dev.max()), "scores": [round(s, 4) for s in scores]}


def runner_bench(model, args):
    H, W, n, P = 720, 1280, 3, args.pairs
    rng = np.random.Generator(np.random.PCG64(1))
    frames = texture(rng, P + 1, H, W)
    E = 200000 * P
    ev = np.stack([np.sort(rng.uniform(0.0, float(P), E)), rng.integers(0, W, E), rng.integers(0, H, E),
                   rng.integers(0, 2, E)], axis=1).astype(np.float32)
    pairs = sequence.make_pairs(ev[:, 0], *sequence.sharp_windows(np.arange(P + 1, dtype=np.float64)))
    torch.manual_seed(1)
    net = define_network(dict(type="FinalBidirectionAttenfusion", img_chn=6, ev_chn=2, num_encoders=3, base_num_channels=32,
                              num_block=1)).to("cuda")
    interp = sequence.SequenceInterpolator(net, 1, n, "sharp", max_minibatch=2)
    routes = {"niqe_none": lambda: interp.run(frames, ev, pairs), "niqe_model": lambda: interp.run(frames, ev, pairs, niqe=model)}
    for fn in routes.values():
        fn()
    times = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t)
    out = {k: {"median_s": statistics.median(v), "min_max_s": [min(v), max(v)]} for k, v in times.items()}
    return {"frame": [H, W], "n": n, "pairs": P, "max_minibatch": 2, "output_frames_per_call": P * n, "routes": out,
            "added_ms_per_output_frame": 1e3 * (out["niqe_model"]["median_s"] - out["niqe_none"]["median_s"]) / (P * n)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--params", default=os.path.join(ROOT, "tests", "golden", "niqe_pris_params.npz"))
    ap.add_argument("--frames", type=int, default=4, help="frames per moments call")
    ap.add_argument("--calls", type=int, default=1000, help="moments calls per timed window (a window of some 0.1-0.3 s)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--skip-runner", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "niqe_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_niqe.py needs the GPU (there is no CPU path)")
    model = niqe.NiqeModel.load(args.params)
    result = {"bench": "niqe", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
              "moments": [moments_bench(model, h, w, args) for h, w in ((1224, 1632), (720, 1280))]}
    if not args.skip_runner:
        result["sequence_interpolator"] = runner_bench(model, args)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
