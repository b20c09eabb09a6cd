#!/usr/bin/env python3
"""Time the JPEG key-frame route: host entropy decode on a thread pool (csrc/jpeg_entropy.h), IDCT, upsampling and colour on
the device (csrc/jpeg_decode.hip).

The tool makes its own files in a temporary directory: ``--frames`` (16) frames each of 720x1280 and 1080x1920 RGB, smooth
synthetic content plus noise (tools/bench_png_decode.py's), encoded 4:2:0 at quality 90 by the project's encoder
(``ops.jpeg_encode``, restart markers every MCU row), and the decoded pixels written again as adaptively filtered PNGs
(tests/png_filter_ref.py, zlib level 6) for the comparison.  Per size, per frame, each window ending in a device synchronise:
  (a) the host stage alone, on ONE thread: read + jpeg.probe + jpeg.entropy_decode over the files, serially;
  (a8) the same on a pool of ``--workers`` threads;
  (b) the whole sequence.load_jpeg_frames (pool, pinned staging, uploads, one decode per chunk);
  (c) the device launches alone: device events around ``--calls`` passes of refid_jpeg_decode over the resident
      coefficients of all chunks; also as a fraction of the HBM rate (MI355X: 8 TB/s peak, about 6.3 TB/s achievable) on
      3 bytes per pixel of coefficients in (4:2:0: 1.5 int16 per pixel) plus 3 bytes per pixel out;
  (d) sequence.load_png_frames on the same pixels.
Every figure is the median of ``--rounds`` windows after a warm-up, with min-max; the files were just written, so reads come
from the page cache.  Also: whether the decoded frames equal PIL's decode of the same files (null without PIL).  No
threshold is asserted: this path had not been measured before.  Prints one JSON line and writes it to --out
(profiles/jpeg_decode_bench.json).  Needs the GPU: there is no CPU path."""
import argparse
import ctypes
import io
import json
import os
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import png_filter_ref as R  # noqa: E402
from bench_png_decode import content, stat  # noqa: E402
from refid_amd import _lib, jpeg, ops, sequence  # noqa: E402

HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12


def host_stage(path):
    with open(path, "rb") as f:
        data = f.read()
    info = jpeg.probe(data)
    coefs = np.empty((info.total_blocks, 64), dtype=np.int16)
    quant = np.empty((info.components, 64), dtype=np.uint16)
    jpeg.entropy_decode(data, info, coefs, quant)
    return coefs, quant


def bench_size(tmp, frames, args, Image):
    n, h, w = frames.shape[:3]
    per = args.frames_per_launch
    out, lens = ops.jpeg_encode(torch.from_numpy(frames).cuda(), quality=90, subsampling="420")
    out, lens = out.cpu().numpy(), lens.cpu().numpy()
    assert (lens > 0).all(), lens
    files = []
    for k in range(n):
        files.append(os.path.join(tmp, f"jpg_{h}", f"{k:04d}.jpg"))
        os.makedirs(os.path.dirname(files[-1]), exist_ok=True)
        with open(files[-1], "wb") as f:
            f.write(out[k, :lens[k]].tobytes())
    # (b) first: the warm-up of the kernels and the check of the result
    got = sequence.load_jpeg_frames(files, workers=args.workers, frames_per_launch=per)
    torch.cuda.synchronize()
    pixels = got.cpu().numpy()
    equal = None
    if Image is not None:
        equal = all(np.array_equal(np.asarray(Image.open(io.BytesIO(open(f, "rb").read())).convert("RGB")), pixels[k]) for k, f in enumerate(files))
    pngs = []
    for k in range(n):
        pngs.append(os.path.join(tmp, f"png_{h}", f"{k:04d}.png"))
        R.write_filtered_png(pngs[-1], pixels[k], R.adaptive_types(pixels[k]), level=6)
    png_equal = bool(torch.equal(sequence.load_png_frames(pngs, workers=args.workers, frames_per_launch=per), got))
    # the resident coefficients of all chunks, for (c)
    decoded = [host_stage(f) for f in files]
    chunks = [(i, min(i + per, n)) for i in range(0, n, per)]
    coefs = [torch.from_numpy(np.stack([decoded[k][0] for k in range(i, j)])).cuda() for i, j in chunks]
    quant = [torch.from_numpy(np.stack([decoded[k][1] for k in range(i, j)]).view(np.int16)).cuda() for i, j in chunks]
    dev_out = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    work = torch.empty((_lib.lib().refid_jpeg_decode_work_bytes(per, h, w, _lib.JPEG_DEC_420) // 8,), dtype=torch.int64, device="cuda")
    descs = [_lib.JpegDecodeDesc(coefs=c.data_ptr(), quant=q.data_ptr(), frames=dev_out[i:j].data_ptr(), work=work.data_ptr(), n_frames=j - i,
                                 height=h, width=w, sampling=_lib.JPEG_DEC_420) for (i, j), c, q in zip(chunks, coefs, quant)]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launches():
        for d in descs:
            _lib.check(_lib.lib().refid_jpeg_decode(ctypes.byref(d), stream), "refid_jpeg_decode")

    launches()
    torch.cuda.synchronize()
    launches_equal = bool(torch.equal(dev_out, got))
    t_a, t_a8, t_b, t_c, t_d = [], [], [], [], []
    with ThreadPoolExecutor(max_workers=args.workers) as pool:
        list(pool.map(host_stage, files))                       # warm-up of the pool's threads
        for _ in range(args.rounds):
            t = time.perf_counter()
            for f in files:
                host_stage(f)
            t_a.append((time.perf_counter() - t) / n)
            t = time.perf_counter()
            list(pool.map(host_stage, files))
            t_a8.append((time.perf_counter() - t) / n)
            torch.cuda.synchronize()
            t = time.perf_counter()
            sequence.load_jpeg_frames(files, workers=args.workers, frames_per_launch=per)
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
            sequence.load_png_frames(pngs, workers=args.workers, frames_per_launch=per)
            torch.cuda.synchronize()
            t_d.append((time.perf_counter() - t) / n)
    b, c, d = (statistics.median(v) for v in (t_b, t_c, t_d))
    bytes_per_frame = 6 * h * w
    return {"frame": [h, w, 3], "files": n, "sampling": "420", "quality": 90, "frames_per_launch": per,
            "jpeg_bytes_mean": int(np.mean([os.path.getsize(f) for f in files])), "png_bytes_mean": int(np.mean([os.path.getsize(f) for f in pngs])),
            "decoded_equals_pil": equal, "png_route_gives_the_same_pixels": png_equal, "launches_give_the_same_pixels": launches_equal,
            "a_host_stage_one_thread_ms_per_frame": stat(t_a, 1e3), "a8_host_stage_pool_ms_per_frame": stat(t_a8, 1e3),
            "b_load_jpeg_frames_ms_per_frame": stat(t_b, 1e3), "b_frames_per_s": 1.0 / b,
            "c_decode_launches_ms_per_frame": stat(t_c, 1e3), "c_frames_per_s": 1.0 / c, "c_window_s": c * args.calls * n,
            "c_bytes_per_frame": bytes_per_frame, "c_bytes_per_s": bytes_per_frame / c,
            "c_fraction_of_hbm_peak_8TBps": bytes_per_frame / c / HBM_PEAK, "c_fraction_of_hbm_achievable_6p3TBps": bytes_per_frame / c / HBM_ACHIEVABLE,
            "d_load_png_frames_ms_per_frame": stat(t_d, 1e3), "d_frames_per_s": 1.0 / d,
            "b_over_d": b / d}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=16, help="files per size")
    ap.add_argument("--workers", type=int, default=8, help="host threads (load_jpeg_frames' default)")
    ap.add_argument("--frames-per-launch", type=int, default=8)
    ap.add_argument("--calls", type=int, default=2000, help="passes over the resident chunks per (c) window (a window of tenths of a second)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="720x1280,1080x1920")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_decode.py needs the GPU (there is no CPU path)")
    try:
        from PIL import Image
    except ImportError:
        Image = None
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    result = {"bench": "jpeg_decode", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "workers": args.workers,
              "calls": args.calls, "results": []}
    with tempfile.TemporaryDirectory() as tmp:
        for h, w in sizes:
            result["results"].append(bench_size(tmp, content(args.frames, h, w, h), args, Image))
            print(json.dumps(result["results"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
