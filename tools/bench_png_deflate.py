#!/usr/bin/env python3
"""Time the PNG output route with the deflate on the device (csrc/png_deflate.hip) against the host's zlib.

One process, one GPU.  The frame sets and the method are tools/bench_png_encode.py's: per frame size (720x1280 and
1224x1632) ``synthetic`` (smooth waves, edges, sigma = 3 noise) and ``network`` (the uint8 output of the released-size network
with random weights on that content); both routes work on the adaptive rows of ops.png_filter.
  (a) the three refid_png_deflate launches alone: device events around ``--calls`` calls over the resident rows, ms per frame
      and GB/s over the algorithmic bytes (the rows read twice, the stream written once).
  (b) host png.encode_png_rows (level 1, Z_HUFFMAN_ONLY) of the same rows on one thread, ms per frame.
  (c) validation.FrameWriter end to end from resident uint8 frames, ``--items`` dumps of the set, png_deflate 'host' against
      'device', both with png_filter 'adaptive': frames/s of a wall clock that ends with close().
  (d) SequenceInterpolator.run with PNGs on, both settings (png_filter 'adaptive'): output frames/s.
The routes of (c) and (d) alternate after a warm-up; every figure is the median of ``--rounds`` rounds with min-max.  File and
stream sizes of both routes are reported over raw (3WH).  ``device_streams_inflate_to_the_rows``: zlib.decompress of every
device stream of the set; ``decoded_equals_source``: the files of (c) read back with png.read_png.  Files land in a temporary
directory (page cache).  Prints one JSON line and writes it to --out (profiles/png_deflate_bench.json).  Needs the GPU."""
import argparse
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
from bench_png_encode import stat, wall  # noqa: E402
from refid_amd import _lib, ops, png, sequence  # noqa: E402
from refid_amd.archs import define_network  # noqa: E402
from refid_amd.interpolate import RELEASED_NETWORK  # noqa: E402
from refid_amd.validation import FrameWriter  # noqa: E402

ROUTES = ("host", "device")


def bench_set(frames, args, tmp):
    """(a), (b), (c) for one resident set ``frames``: uint8 numpy (N, H, W, 3)."""
    n, h, w = frames.shape[:3]
    pitch, raw = 1 + 3 * w, 3 * w * h
    dev = torch.from_numpy(frames).cuda()
    rows_dev = ops.png_filter(dev)
    out, lens = ops.png_deflate(rows_dev)                       # warm-up, and the streams whose sizes are reported
    torch.cuda.synchronize()
    rows, streams, lengths = rows_dev.cpu().numpy(), out.cpu().numpy(), lens.cpu().numpy()
    inflates = all(zlib.decompress(streams[k, :lengths[k]].tobytes()) == rows[k].tobytes() for k in range(n))
    # (a)
    t_a = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            ops.png_deflate(rows_dev, out=out)
        e1.record()
        e1.synchronize()
        t_a.append(e0.elapsed_time(e1) * 1e-3 / (args.calls * n))
    a = statistics.median(t_a)
    # (b)
    host_bytes = sum(len(png.encode_png_rows(rows[k], w, h)) for k in range(n)) / n                        # (also the warm-up)
    t_b = []
    for _ in range(args.rounds):
        t = time.perf_counter()
        for k in range(n):
            png.encode_png_rows(rows[k], w, h)
        t_b.append((time.perf_counter() - t) / n)
    # (c)
    t_c, equal = {route: [] for route in ROUTES}, True
    paths = {route: [[os.path.join(tmp, f"c_{h}_{route}", f"{i:02d}_{k:02d}.png") for k in range(n)] for i in range(args.items)]
             for route in ROUTES}

    def writer_run(route):
        writer = FrameWriter(torch.device("cuda"), png_filter="adaptive", png_deflate=route)
        try:
            for i in range(args.items):
                writer.dump([(dev, paths[route][i])])
        finally:
            writer.close()

    for route in ROUTES:
        writer_run(route)                                       # warm-up: pinned buffers, directories, page cache
        equal = equal and all(np.array_equal(png.read_png(paths[route][-1][k]), frames[k]) for k in range(n))
    for _ in range(args.rounds):
        for route in ROUTES:
            t_c[route].append(args.items * n / wall(lambda: writer_run(route)))
    file_ratio = {route: float(np.mean([os.path.getsize(p) for p in paths[route][0]])) / raw for route in ROUTES}
    device_bytes = float(np.mean(lengths)) + len(png.wrap_zlib_stream(b"\x78\x01" + bytes(9), w, h)) - 11
    return {"frame": [h, w, 3], "frames": n, "raw_bytes_per_frame": raw, "block_bytes": _lib.PNG_DEFLATE_BLOCK,
            "blocks_per_frame": -(-pitch * h // _lib.PNG_DEFLATE_BLOCK),
            "a_deflate_launches_ms_per_frame": stat(t_a, 1e3), "a_window_s": a * args.calls * n,
            "a_algorithmic_gb_per_s": (2 * pitch * h + float(np.mean(lengths))) / a / 1e9,
            "b_host_encode_ms_per_frame": stat(t_b, 1e3),
            "b_over_a": statistics.median(t_b) / a,
            "png_bytes_over_raw": {"host": host_bytes / raw, "device": device_bytes / raw},
            "device_over_host_bytes": device_bytes / host_bytes,
            "c_frame_writer_fps": {route: stat(v) for route, v in t_c.items()}, "c_frames_per_window": args.items * n,
            "c_file_size_over_raw": file_ratio, "device_streams_inflate_to_the_rows": bool(inflates),
            "decoded_equals_source": bool(equal)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=8, help="frames per set")
    ap.add_argument("--items", type=int, default=32, help="(c): FrameWriter dumps of the set per window (256 frames: the device "
                                                          "route's window is still only 0.1-0.5 s)")
    ap.add_argument("--calls", type=int, default=2000, help="(a): calls over the set per window (a few tenths of a second)")
    ap.add_argument("--pairs", type=int, default=4, help="(d) and the network set: key-frame pairs")
    ap.add_argument("--n", type=int, default=7, help="(d) and the network set: frames per pair")
    ap.add_argument("--events-per-pair", type=int, default=400000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="720x1280,1224x1632")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_deflate_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_png_deflate.py needs the GPU (there is no CPU path)")
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    result = {"bench": "png_deflate", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "writer_threads": FrameWriter.WORKERS,
              "zlib": zlib.ZLIB_VERSION, "host_route": "encode_png_rows, level 1, Z_HUFFMAN_ONLY", "results": [], "sequence_interpolate": [],
              "not_measured": ["photographs or real footage (none on the machine)", "trained weights (the network set is the output "
                               "of random weights)", "a disk: the files land in the page cache", "block sizes other than the default",
                               "the three launches one by one (no kernel trace was taken)"]}
    torch.manual_seed(1)
    net = define_network(dict(RELEASED_NETWORK, img_chn=6)).to("cuda")
    interp = sequence.SequenceInterpolator(net, 1, args.n, "sharp", max_minibatch=2)
    with tempfile.TemporaryDirectory(prefix="refid_png_deflate_bench_") as tmp:
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
            dirs = {route: os.path.join(tmp, f"d_{h}_{route}") for route in ROUTES}
            runs = {route: (lambda route=route: interp.run(keys[:P + 1], ev, pairs, out_dir=dirs[route], png_filter="adaptive",
                                                           png_deflate=route)) for route in ROUTES}
            for fn in runs.values():
                fn()
            names = sorted(os.listdir(dirs["host"]))
            same = names == sorted(os.listdir(dirs["device"])) and all(
                np.array_equal(png.read_png(os.path.join(dirs["host"], f)), png.read_png(os.path.join(dirs["device"], f))) for f in names[:4])
            t_d = {route: [] for route in ROUTES}
            for _ in range(args.rounds):
                for route, fn in runs.items():
                    t_d[route].append(P * args.n / wall(fn))
            result["sequence_interpolate"].append({
                "frame": [h, w, 3], "pairs": P, "n": args.n, "output_frames_per_call": P * args.n,
                "d_run_fps": {route: stat(v) for route, v in t_d.items()}, "same_pixels_in_both": bool(same),
                "file_size_over_raw": {route: float(np.mean([os.path.getsize(os.path.join(d, f)) for f in names])) / (3 * w * h)
                                       for route, d in dirs.items()}})
            print(json.dumps(result["sequence_interpolate"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
