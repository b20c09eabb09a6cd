#!/usr/bin/env python3
"""Time the PNG key-frame route: host inflate on a thread pool, unfilter on the device (csrc/png.hip).

The tool writes its own files into a temporary directory: ``--frames`` (16) frames each of 720x1280 and 1224x1632 RGB,
smooth synthetic content plus noise, encoded by tests/png_filter_ref.py with the adaptive (least sum of absolute values)
heuristic at zlib level 6; when PIL is importable a second set is written by PIL.  ``sets`` in the JSON says which ran.
Per set and size, per frame, each window ending in a device synchronise:
  (a) read + inflate alone: png.read_filtered over the files on a pool of ``--workers`` threads;
  (b) the whole sequence.load_png_frames (pool, pinned staging, upload, unfilter launches);
  (c) the unfilter launches alone: device events around ``--calls`` passes over the resident inflated chunks;
  (d) the host route interpolate.load_frames (serial png.read_png) on 2 frames only, scaled per frame: it takes seconds.
Every figure is the median of ``--rounds`` windows after a warm-up, with min-max; the files were just written, so reads
come from the page cache.  Also: the filter-type histogram of the files, the band count, and whether the decoded frames
equal the source arrays.  Two relations are stated with their numbers: (c) < (a) -- inflate cannot move to the GPU, so
unfiltering then no longer decides the decode time -- and (b) < (d).
Prints one JSON line and writes it to --out (profiles/png_decode_bench.json).  Needs the GPU: there is no CPU path."""
import argparse
import ctypes
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import png_filter_ref as R  # noqa: E402
from refid_amd import _lib, png, sequence  # noqa: E402
from refid_amd.interpolate import load_frames  # noqa: E402


def content(n, h, w, seed):
    """Smooth waves, a few hard edges and sensor-like noise."""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = np.empty((n, h, w, 3), dtype=np.uint8)
    for k in range(n):
        base = 118 + 60 * np.sin((xx + 31 * k) / 53.0) + 45 * np.cos((yy - 17 * k) / 37.0) + 20 * np.sin((xx + yy) / 11.0)
        base += 40 * ((xx // 160 + yy // 120 + k) % 3 == 0)
        img = base[:, :, None] + np.array([0.0, 14.0, -22.0], dtype=np.float32) + rng.normal(0, 3.0, (h, w, 3)).astype(np.float32)
        out[k] = np.clip(img, 0, 255).astype(np.uint8)
    return out


def stat(values, scale=1.0):
    return {"median": scale * statistics.median(values), "min_max": [scale * min(values), scale * max(values)]}


def bench_set(files, frames, args):
    n, h, w = frames.shape[:3]
    pitch = 1 + 3 * w
    # what the files hold
    rows = [png.read_filtered(f)[3] for f in files]
    filters = np.stack([r[:, 0] for r in rows])
    per = args.frames_per_launch
    chunks = [(i, min(i + per, n)) for i in range(0, n, per)]
    bands = [png.find_bands(filters[i:j]) for i, j in chunks]
    # (b) first: it is also the warm-up of the kernel and the check of the result
    got = sequence.load_png_frames(files, workers=args.workers, frames_per_launch=per)
    torch.cuda.synchronize()
    equal = bool(torch.equal(got.cpu(), torch.from_numpy(frames)))
    t_a, t_b, t_c, t_d = [], [], [], []
    dev_rows = [torch.from_numpy(np.stack(rows[i:j])).cuda() for i, j in chunks]
    dev_bands = [torch.from_numpy(b).cuda() for b in bands]
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    descs = [_lib.PngUnfilterDesc(rows=r.data_ptr(), frames=out[i:j].data_ptr(), bands=b.data_ptr(), n_bands=int(b.shape[0]),
                                  n_frames=j - i, height=h, width=w, channels=3) for (i, j), r, b in zip(chunks, dev_rows, dev_bands)]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launches():
        for d in descs:
            _lib.check(_lib.lib().refid_png_unfilter(ctypes.byref(d), stream), "refid_png_unfilter")

    launches()
    torch.cuda.synchronize()
    equal = equal and bool(torch.equal(out, got))
    with tempfile.TemporaryDirectory() as two:
        for f in files[:2]:
            shutil.copy(f, two)
        with ThreadPoolExecutor(max_workers=args.workers) as pool:
            list(pool.map(png.read_filtered, files))            # warm-up of the pool's threads
            for _ in range(args.rounds):
                torch.cuda.synchronize()
                t = time.perf_counter()
                list(pool.map(png.read_filtered, files))
                torch.cuda.synchronize()
                t_a.append((time.perf_counter() - t) / n)
                t = time.perf_counter()
                sequence.load_png_frames(files, workers=args.workers, frames_per_launch=per)
                torch.cuda.synchronize()
                t_b.append((time.perf_counter() - t) / n)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    launches()
                e1.record()
                e1.synchronize()
                t_c.append(e0.elapsed_time(e1) * 1e-3 / (args.calls * n))
                t = time.perf_counter()
                host = load_frames(two)
                torch.cuda.synchronize()
                t_d.append((time.perf_counter() - t) / 2)
        equal = equal and np.array_equal(host, frames[:2])
    a, b, c, d = (statistics.median(v) for v in (t_a, t_b, t_c, t_d))
    return {"frame": [h, w, 3], "files": n, "file_bytes_mean": int(np.mean([os.path.getsize(f) for f in files])),
            "inflated_bytes_per_frame": h * pitch, "frames_per_launch": per,
            "filter_histogram": {str(t): int((filters == t).sum()) for t in range(5)},
            "bands": int(sum(len(b) for b in bands)), "bands_per_frame": sum(len(b) for b in bands) / n,
            "decoded_equals_source": equal,
            "a_read_inflate_ms_per_frame": stat(t_a, 1e3), "b_load_png_frames_ms_per_frame": stat(t_b, 1e3),
            "c_unfilter_launches_ms_per_frame": stat(t_c, 1e3), "c_window_s": c * args.calls * n,
            "d_host_route_ms_per_frame": stat(t_d, 1e3), "d_frames_timed": 2,
            "c_below_a": {"holds": bool(c < a), "c_ms": 1e3 * c, "a_ms": 1e3 * a},
            "b_below_d": {"holds": bool(b < d), "b_ms": 1e3 * b, "d_ms": 1e3 * d}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=16, help="files per set and size")
    ap.add_argument("--workers", type=int, default=8, help="inflate threads (load_png_frames' default)")
    ap.add_argument("--frames-per-launch", type=int, default=8)
    ap.add_argument("--calls", type=int, default=50, help="passes over the resident chunks per (c) window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="720x1280,1224x1632")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_decode_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_png_decode.py needs the GPU (there is no CPU path)")
    try:
        from PIL import Image
    except ImportError:
        Image = None
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    result = {"bench": "png_decode", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "workers": args.workers,
              "sets": ["adaptive"] + (["pil"] if Image is not None else []), "results": []}
    with tempfile.TemporaryDirectory() as tmp:
        for h, w in sizes:
            frames = content(args.frames, h, w, h)
            for name in result["sets"]:
                files = []
                for k, img in enumerate(frames):
                    path = os.path.join(tmp, f"{name}_{h}", f"{k:04d}.png")
                    if name == "adaptive":
                        R.write_filtered_png(path, img, R.adaptive_types(img), level=6)
                    else:
                        os.makedirs(os.path.dirname(path), exist_ok=True)
                        Image.fromarray(img).save(path)
                    files.append(path)
                result["results"].append(dict(set=name, **bench_set(files, frames, args)))
                print(json.dumps(result["results"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
