#!/usr/bin/env python3
"""Time the Motion-JPEG output route (csrc/jpeg.hip, validation.VideoWriter) against the PNG route with the deflate on the
device (csrc/png_deflate.hip, validation.FrameWriter).

One process, one GPU.  The frame sets and the method are tools/bench_png_deflate.py's: per frame size (720x1280 and
1224x1632) ``synthetic`` (smooth waves, edges, sigma = 3 noise) and ``network`` (the uint8 output of the released-size network
with random weights on that content).
  (a) the three refid_jpeg_encode launches alone, per subsampling at quality 90: device events around ``--calls`` calls over
      the resident frames, ms per frame and GB/s over the algorithmic bytes (the frames read once, the file written once).
  (b) validation.VideoWriter end to end from resident uint8 frames, ``--items`` adds of the set, against
      validation.FrameWriter(png_filter='adaptive', png_deflate='device') dumping the same frames as PNGs: frames/s of a wall
      clock that ends with close().
  (c) SequenceInterpolator.run with video= (key frames included) against out_dir= with PNGs (adaptive, device): output
      frames/s of the interpolated frames.
  (d) file bytes over raw (3WH) at qualities 75 / 90 / 95 for both subsamplings, next to PIL's own encode of the same frames
      at the same settings (optimize=False), when PIL is installed.
The routes of (b) and (c) alternate after a warm-up; every figure is the median of ``--rounds`` rounds with min-max.
``frames_decode_in_pil``: every frame of the container of (b) opens in PIL with the right size.  Files land in a temporary
directory (page cache).  Prints one JSON line and writes it to --out (profiles/jpeg_bench.json).  Needs the GPU."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_png_decode import content  # noqa: E402
from bench_png_encode import stat, wall  # noqa: E402
from refid_amd import ops, sequence  # noqa: E402
from refid_amd.archs import define_network  # noqa: E402
from refid_amd.interpolate import RELEASED_NETWORK  # noqa: E402
from refid_amd.validation import FrameWriter, VideoWriter  # noqa: E402
from refid_amd.video import read_mjpeg_avi  # noqa: E402

try:
    from PIL import Image
except ImportError:
    Image = None

QUALITIES = (75, 90, 95)
SUBSAMPLINGS = ("420", "444")
ROUTES = ("png_device", "mjpeg")


def bench_set(frames, args, tmp):
    """(a), (b), (d) for one resident set ``frames``: uint8 numpy (N, H, W, 3)."""
    n, h, w = frames.shape[:3]
    raw = 3 * w * h
    dev = torch.from_numpy(frames).cuda()
    # (d), and the warm-up
    sizes, pil_sizes = {}, {}
    for ss in SUBSAMPLINGS:
        for q in QUALITIES:
            out, lens = ops.jpeg_encode(dev, q, ss)
            lengths = lens.cpu().numpy()
            assert (lengths > 0).all(), "a frame of the set does not fit the default pitch"
            sizes[f"{ss}_q{q}"] = float(np.mean(lengths)) / raw
            if Image is not None:
                total = 0
                for k in range(n):
                    buf = io.BytesIO()
                    Image.fromarray(frames[k]).save(buf, "JPEG", quality=q, subsampling={"444": 0, "420": 2}[ss], optimize=False)
                    total += buf.tell()
                pil_sizes[f"{ss}_q{q}"] = total / n / raw
    # (a)
    a = {}
    for ss in SUBSAMPLINGS:
        out, lens = ops.jpeg_encode(dev, 90, ss)
        mean_len = float(lens.float().mean())
        t_a = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                ops.jpeg_encode(dev, 90, ss, out=out)
            e1.record()
            e1.synchronize()
            t_a.append(e0.elapsed_time(e1) * 1e-3 / (args.calls * n))
        med = statistics.median(t_a)
        a[ss] = {"ms_per_frame": stat(t_a, 1e3), "window_s": med * args.calls * n, "algorithmic_gb_per_s": (raw + mean_len) / med / 1e9}
    # (b)
    paths = [[os.path.join(tmp, f"b_{h}", f"{i:02d}_{k:02d}.png") for k in range(n)] for i in range(args.items)]
    avi = os.path.join(tmp, f"b_{h}.avi")

    def png_run():
        writer = FrameWriter(torch.device("cuda"), png_filter="adaptive", png_deflate="device")
        try:
            for i in range(args.items):
                writer.dump([(dev, paths[i])])
        finally:
            writer.close()

    def mjpeg_run():
        writer = VideoWriter(torch.device("cuda"), avi, 30)
        try:
            for i in range(args.items):
                writer.add(dev)
        finally:
            writer.close()

    runs = {"png_device": png_run, "mjpeg": mjpeg_run}
    for fn in runs.values():
        fn()                                                    # warm-up: pinned buffers, directories, page cache
    head, video = read_mjpeg_avi(avi)
    decodes = None
    if Image is not None:
        decodes = len(video) == args.items * n
        for data in video[:n]:
            with Image.open(io.BytesIO(data)) as im:
                im.load()
                decodes = decodes and im.size == (w, h)
    t_b = {route: [] for route in ROUTES}
    for _ in range(args.rounds):
        for route, fn in runs.items():
            t_b[route].append(args.items * n / wall(fn))
    png_bytes = float(np.mean([os.path.getsize(p) for p in paths[0]]))
    return {"frame": [h, w, 3], "frames": n, "raw_bytes_per_frame": raw, "a_jpeg_launches_q90": a,
            "b_writer_fps": {route: stat(v) for route, v in t_b.items()}, "b_frames_per_window": args.items * n,
            "b_mjpeg_over_png_device_fps": statistics.median(t_b["mjpeg"]) / statistics.median(t_b["png_device"]),
            "b_bytes_over_raw": {"png_device": png_bytes / raw, "mjpeg_avi": os.path.getsize(avi) / (args.items * n) / raw},
            "d_jpeg_bytes_over_raw": sizes, "d_pil_bytes_over_raw": pil_sizes or None, "frames_decode_in_pil": decodes}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=8, help="frames per set")
    ap.add_argument("--items", type=int, default=32, help="(b): adds / dumps of the set per window")
    ap.add_argument("--calls", type=int, default=2000, help="(a): calls over the set per window (a few tenths of a second)")
    ap.add_argument("--pairs", type=int, default=4, help="(c) and the network set: key-frame pairs")
    ap.add_argument("--n", type=int, default=7, help="(c) and the network set: frames per pair")
    ap.add_argument("--events-per-pair", type=int, default=400000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="720x1280,1224x1632")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg.py needs the GPU (there is no CPU path)")
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    result = {"bench": "jpeg", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "png_writer_threads": FrameWriter.WORKERS,
              "pil": None if Image is None else Image.__version__, "results": [], "sequence_interpolate": [],
              "not_measured": ["photographs or real footage (none on the machine)", "trained weights (the network set is the output "
                               "of random weights)", "a disk: the files land in the page cache", "playback: no player or ffmpeg is "
                               "installed; PIL decodes the frames, read_mjpeg_avi walks the container",
                               "restart intervals other than one MCU row", "the three launches one by one (no kernel trace was taken)",
                               "qualities other than 90 for the launch times", "PSNR at these sizes (tests/test_jpeg_ref_host.py "
                               "compares with PIL's encode on the small cases)"]}
    torch.manual_seed(1)
    net = define_network(dict(RELEASED_NETWORK, img_chn=6)).to("cuda")
    interp = sequence.SequenceInterpolator(net, 1, args.n, "sharp", max_minibatch=2)
    with tempfile.TemporaryDirectory(prefix="refid_jpeg_bench_") as tmp:
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
            # (c)
            png_dir, avi = os.path.join(tmp, f"c_{h}_png"), os.path.join(tmp, f"c_{h}.avi")
            runs = {"png_device": lambda: interp.run(keys[:P + 1], ev, pairs, out_dir=png_dir, png_filter="adaptive", png_deflate="device"),
                    "mjpeg": lambda: interp.run(keys[:P + 1], ev, pairs, video=avi)}
            for fn in runs.values():
                fn()
            head, video = read_mjpeg_avi(avi)
            t_c = {route: [] for route in ROUTES}
            for _ in range(args.rounds):
                for route, fn in runs.items():
                    t_c[route].append(P * args.n / wall(fn))
            result["sequence_interpolate"].append({
                "frame": [h, w, 3], "pairs": P, "n": args.n, "output_frames_per_call": P * args.n, "video_frames": len(video),
                "c_run_fps": {route: stat(v) for route, v in t_c.items()},
                "bytes_over_raw": {"png_device": float(np.mean([os.path.getsize(os.path.join(png_dir, f)) for f in os.listdir(png_dir)])) / (3 * w * h),
                                   "mjpeg_avi": os.path.getsize(avi) / len(video) / (3 * w * h)}})
            print(json.dumps(result["sequence_interpolate"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
