#!/usr/bin/env python3
"""Time the PNG output route: row filters chosen on the device (csrc/png_filter.hip), deflate on the host.

One process, one GPU.  Per frame size (720x1280 and 1224x1632) two frame sets: ``synthetic`` -- the content of
tools/bench_png_decode.py (smooth waves, edges, sigma = 3 noise) -- and ``network`` -- the uint8 output frames of the
released-size network with random weights on that content as key frames plus uniform random events.
  (a) the refid_png_filter launch alone: device events around ``--calls`` adaptive launches over the resident set, ms per
      frame and GB/s over the algorithmic bytes, 3WH read + (1 + 3W)H written.
  (b) host encode per frame on one thread: png.encode_png (filter 0, level 1: the parent route) against
      png.encode_png_rows of the device's rows with Z_RLE and with Z_HUFFMAN_ONLY; time and size / raw (raw = 3WH).
  (c) validation.FrameWriter end to end from resident uint8 frames, ``--items`` dumps of the set, png_filter 'none' against
      'adaptive' (with encode_png_rows' default strategy, ``default_strategy`` in the JSON): frames/s of a wall clock that
      ends with close().
  (d) SequenceInterpolator.run with PNGs on, both settings: output frames/s (network frames only, by construction).
The routes of (b), (c) and (d) alternate after a warm-up; every figure is the median of ``--rounds`` rounds with min-max.
Files land in a temporary directory (page cache).  ``a_below_quarter_b``: four writer threads each take (b), so below
(b)/4 the launch cannot be what the writer waits for.  ``decoded_equals_source``: the files of (c) read back with
png.read_png.  Prints one JSON line and writes it to --out (profiles/png_encode_bench.json).  Needs the GPU."""
import argparse
import inspect
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_png_decode import content  # noqa: E402
from refid_amd import ops, png, sequence  # noqa: E402
from refid_amd.archs import define_network  # noqa: E402
from refid_amd.interpolate import RELEASED_NETWORK  # noqa: E402
from refid_amd.validation import FrameWriter  # noqa: E402


def stat(values, scale=1.0):
    return {"median": scale * statistics.median(values), "min_max": [scale * min(values), scale * max(values)]}


def strategy_name(value):
    return {zlib.Z_DEFAULT_STRATEGY: "Z_DEFAULT_STRATEGY", zlib.Z_RLE: "Z_RLE", zlib.Z_HUFFMAN_ONLY: "Z_HUFFMAN_ONLY"}.get(value, str(value))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench_set(frames, args, tmp):
    """(a), (b), (c) for one resident set ``frames``: uint8 numpy (N, H, W, 3)."""
    n, h, w = frames.shape[:3]
    pitch, raw = 1 + 3 * w, 3 * w * h
    dev = torch.from_numpy(frames).cuda()
    out = torch.empty((n, h, pitch), dtype=torch.uint8, device="cuda")
    ops.png_filter(dev, out=out)                                # warm-up, and the rows (b) encodes
    torch.cuda.synchronize()
    rows = out.cpu().numpy()
    histogram = {str(t): int((rows[:, :, 0] == t).sum()) for t in range(5)}
    # (a)
    t_a = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            ops.png_filter(dev, out=out)
        e1.record()
        e1.synchronize()
        t_a.append(e0.elapsed_time(e1) * 1e-3 / (args.calls * n))
    a = statistics.median(t_a)
    # (b)
    encoders = {"filter0_level1": lambda k: png.encode_png(frames[k], 1),
                "adaptive_rle": lambda k: png.encode_png_rows(rows[k], w, h, 1, zlib.Z_RLE),
                "adaptive_huffman_only": lambda k: png.encode_png_rows(rows[k], w, h, 1, zlib.Z_HUFFMAN_ONLY)}
    sizes = {name: sum(len(fn(k)) for k in range(n)) / (n * raw) for name, fn in encoders.items()}       # (also the warm-up)
    t_b = {name: [] for name in encoders}
    for _ in range(args.rounds):
        for name, fn in encoders.items():
            t = time.perf_counter()
            for k in range(n):
                fn(k)
            t_b[name].append((time.perf_counter() - t) / n)
    b = {name: statistics.median(v) for name, v in t_b.items()}
    # (c)
    t_c, equal = {"none": [], "adaptive": []}, True
    paths = {mode: [[os.path.join(tmp, f"c_{h}_{mode}", f"{i:02d}_{k:02d}.png") for k in range(n)] for i in range(args.items)]
             for mode in t_c}

    def writer_run(mode):
        writer = FrameWriter(torch.device("cuda"), png_filter=mode)
        try:
            for i in range(args.items):
                writer.dump([(dev, paths[mode][i])])
        finally:
            writer.close()

    for mode in t_c:
        writer_run(mode)                                        # warm-up: pinned buffers, directories, page cache
        equal = equal and all(np.array_equal(png.read_png(paths[mode][-1][k]), frames[k]) for k in range(n))
    for _ in range(args.rounds):
        for mode in t_c:
            t_c[mode].append(args.items * n / wall(lambda: writer_run(mode)))
    file_ratio = {mode: float(np.mean([os.path.getsize(p) for p in paths[mode][0]])) / raw for mode in t_c}
    return {"frame": [h, w, 3], "frames": n, "raw_bytes_per_frame": raw, "filter_histogram": histogram,
            "a_filter_launch_ms_per_frame": stat(t_a, 1e3), "a_window_s": a * args.calls * n,
            "a_algorithmic_gb_per_s": (raw + pitch * h) / a / 1e9,
            "b_host_encode_ms_per_frame": {name: stat(v, 1e3) for name, v in t_b.items()},
            "b_size_over_raw": sizes,
            "b_speedup_over_filter0": {name: b["filter0_level1"] / v for name, v in b.items()},
            "a_below_quarter_b": {"holds": bool(a < b["adaptive_rle"] / 4), "a_ms": 1e3 * a, "quarter_b_rle_ms": 1e3 * b["adaptive_rle"] / 4},
            "huffman_only_better_on_time_and_size": bool(b["adaptive_huffman_only"] < b["adaptive_rle"] and
                                                         sizes["adaptive_huffman_only"] < sizes["adaptive_rle"]),
            "c_frame_writer_fps": {mode: stat(v) for mode, v in t_c.items()}, "c_frames_per_window": args.items * n,
            "c_file_size_over_raw": file_ratio, "decoded_equals_source": bool(equal)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=8, help="frames per set")
    ap.add_argument("--items", type=int, default=4, help="(c): FrameWriter dumps of the set per window")
    ap.add_argument("--calls", type=int, default=4000, help="(a): launches over the set per window (a few tenths of a second)")
    ap.add_argument("--pairs", type=int, default=4, help="(d) and the network set: key-frame pairs")
    ap.add_argument("--n", type=int, default=7, help="(d) and the network set: frames per pair")
    ap.add_argument("--events-per-pair", type=int, default=400000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="720x1280,1224x1632")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_encode_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_png_encode.py needs the GPU (there is no CPU path)")
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    result = {"bench": "png_encode", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "writer_threads": FrameWriter.WORKERS,
              "zlib": zlib.ZLIB_VERSION, "default_strategy": strategy_name(inspect.signature(png.encode_png_rows).parameters["strategy"].default), "results": [], "sequence_interpolate": [],
              "not_measured": ["photographs or real footage (none on the machine)", "trained weights (the network set is the output "
                               "of random weights)", "grey, 16-bit or alpha files", "a disk: the files land in the page cache"]}
    torch.manual_seed(1)
    net = define_network(dict(RELEASED_NETWORK, img_chn=6)).to("cuda")
    interp = sequence.SequenceInterpolator(net, 1, args.n, "sharp", max_minibatch=2)
    with tempfile.TemporaryDirectory(prefix="refid_png_encode_bench_") as tmp:
        for h, w in sizes:
            P = args.pairs
            keys = content(max(args.frames, P + 1), h, w, h)
            rng = np.random.Generator(np.random.PCG64(h))
            E = args.events_per_pair * P
            ev = np.stack([np.sort(rng.uniform(0.0, float(P), E)), rng.integers(0, w, E), rng.integers(0, h, E),
                           rng.integers(0, 2, E)], axis=1).astype(np.float32)
            pairs = sequence.make_pairs(ev[:, 0], *sequence.sharp_windows(np.arange(P + 1, dtype=np.float64)))
            produced = interp.run(keys[:P + 1], ev, pairs, keep=True).reshape(-1, h, w, 3)
            sets = {"synthetic": keys[:args.frames], "network": np.ascontiguousarray(produced[:args.frames])}
            for name, frames in sets.items():
                result["results"].append(dict(set=name, **bench_set(frames, args, tmp)))
                print(json.dumps(result["results"][-1]), file=sys.stderr, flush=True)
            # (d)
            dirs = {mode: os.path.join(tmp, f"d_{h}_{mode}") for mode in ("none", "adaptive")}
            runs = {mode: (lambda mode=mode: interp.run(keys[:P + 1], ev, pairs, out_dir=dirs[mode], png_filter=mode)) for mode in dirs}
            for fn in runs.values():
                fn()
            names = sorted(os.listdir(dirs["none"]))
            same = names == sorted(os.listdir(dirs["adaptive"])) and all(
                np.array_equal(png.read_png(os.path.join(dirs["none"], f)), png.read_png(os.path.join(dirs["adaptive"], f))) for f in names[:4])
            t_d = {mode: [] for mode in dirs}
            for _ in range(args.rounds):
                for mode, fn in runs.items():
                    t_d[mode].append(P * args.n / wall(fn))
            result["sequence_interpolate"].append({
                "frame": [h, w, 3], "pairs": P, "n": args.n, "output_frames_per_call": P * args.n,
                "d_run_fps": {mode: stat(v) for mode, v in t_d.items()}, "same_pixels_in_both": bool(same),
                "file_size_over_raw": {mode: float(np.mean([os.path.getsize(os.path.join(d, f)) for f in names])) / (3 * w * h)
                                       for mode, d in dirs.items()}})
            print(json.dumps(result["sequence_interpolate"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
