#!/usr/bin/env python3
"""Time blur synthesis (csrc/blur_synth.hip, refid_amd.blur_synth) at 1280x720: 240 resident frames, M = 11, gap 1, which
is 20 blurry key frames of 11 frames each, in one launch.

The clip is synthetic (tools/bench_png_decode.py's ``content``: smooth waves, hard edges and sensor-like noise, panning):
24 frames made on the host, repeated on the device with a horizontal shift per repetition.  Measured per mode -- plain (the
codes are averaged), response (``gamma_table(2.2)``: the levels are averaged, the code looked up), and plain again with
``out`` 3 bytes off a 16-byte boundary, which takes the kernel's general path -- each figure the median of ``--rounds``
windows after a warm-up, with min-max; a window is ``--launches`` launches of the entry point back to back between two
device events, the two tables already on the device (``plain_through_ops`` is ``ops.blur_synth``, which uploads them):
  ms             one launch;
  keys_per_s     blurry frames written per second, ``input_frames_per_s`` sharp frames read per second;
  bytes          what the launch must move: K M frames read, K frames written (the two 1 KiB tables are not counted);
  fraction_of_copy_rate_6.3TBps   bytes / time over the 6.3 TB/s a streaming kernel reaches on an MI355X (HBM is the bound:
                 a launch moves 663 MB, more than the 256 MiB last-level cache holds, so repeated launches do not hit in it).
For comparison, timed in the same process and the same way: the torch formulation, per key
``(frames[a:a + M].float().mean(0) + 0.5).floor().to(uint8)`` -- and whether its bytes equal plain mode's (float32 means
may round a tie differently; nothing is asserted).  The first two keys of each mode are compared with tests/blur_ref.py.
No threshold is asserted: nothing did this work before.  Prints one JSON line and writes it to --out
(profiles/blur_synth_bench.json).  Needs the GPU: there is no CPU path."""
import argparse
import ctypes
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
import blur_ref as R  # noqa: E402
from bench_png_decode import content, stat  # noqa: E402
from refid_amd import _lib, blur_synth, ops  # noqa: E402

COPY_RATE = 6.3e12


def timed(fn, launches, rounds):
    """Seconds per call of ``fn``: ``rounds`` windows of ``launches`` calls between two device events."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3 / launches)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=240, help="sharp frames of the clip")
    ap.add_argument("--size", default="720x1280")
    ap.add_argument("--m", type=int, default=11, help="frames per blurry key frame")
    ap.add_argument("--gap", type=int, default=1)
    ap.add_argument("--gamma", type=float, default=2.2, help="the response mode's table")
    ap.add_argument("--launches", type=int, default=200, help="launches per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blur_synth_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_blur_synth.py needs the GPU (there is no CPU path)")
    h, w = (int(v) for v in args.size.split("x"))
    n, m = args.frames, args.m
    base = torch.from_numpy(content(min(n, 24), h, w, 7)).cuda()
    frames = torch.stack([torch.roll(base[k % base.shape[0]], shifts=7 * (k // base.shape[0]), dims=1) for k in range(n)]).contiguous()
    windows, first = blur_synth.blur_windows(n, m, args.gap)
    k = int(windows.shape[0])
    table = blur_synth.gamma_table(args.gamma)
    frame_bytes = h * w * 3
    moved = k * m * frame_bytes + k * frame_bytes
    out = torch.empty((k, h, w, 3), dtype=torch.uint8, device="cuda")
    off = torch.empty((k * frame_bytes + 16,), dtype=torch.uint8, device="cuda")[3:3 + k * frame_bytes]

    def torch_form():
        return torch.stack([(frames[a:a + m].float().mean(0) + 0.5).floor().to(torch.uint8) for a in first.tolist()])

    win_dev, lin_dev = torch.from_numpy(windows).cuda(), torch.from_numpy(table.view(np.int32)).cuda()
    L, stream = _lib.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def entry_point(to, response):
        """The entry alone, its tables already on the device: what one launch costs without ``ops.blur_synth``'s two uploads."""
        desc = _lib.BlurSynthDesc(frames=frames.data_ptr(), windows_host=windows.ctypes.data, windows=win_dev.data_ptr(),
                                  to_linear_host=table.ctypes.data if response else None, to_linear=lin_dev.data_ptr() if response else None,
                                  out=to.data_ptr(), n_frames=n, height=h, width=w, n_windows=k, max_groups=0)

        def launch():
            _lib.check(L.refid_blur_synth(ctypes.byref(desc), stream), "refid_blur_synth")
            return to.view(k, h, w, 3)
        return launch

    runs = {"plain": entry_point(out, False), "response": entry_point(out, True), "plain_general_path": entry_point(off, False),
            "plain_through_ops": lambda: ops.blur_synth(frames, windows, out=out), "torch_float_mean": torch_form}
    result = {"bench": "blur_synth", "device": torch.cuda.get_device_name(0), "frame": [h, w, 3], "frames": n, "m": m, "gap": args.gap, "keys": k,
              "gamma": args.gamma, "launches_per_window": args.launches, "rounds": args.rounds, "bytes_read": k * m * frame_bytes,
              "bytes_written": k * frame_bytes, "base_aligned_16": frames.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0,
              "general_path_out_offset": off.data_ptr() % 16}
    host = frames[:int(windows[1, 0] + windows[1, 1])].cpu().numpy() if k >= 2 else frames[:m].cpu().numpy()
    for name, fn in runs.items():
        launches = args.launches if name != "torch_float_mean" else max(1, args.launches // 10)
        t = timed(fn, launches, args.rounds)
        med = statistics.median(t)
        entry = {"ms": stat(t, 1e3), "keys_per_s": k / med, "input_frames_per_s": k * m / med, "bytes_per_s": moved / med,
                 "fraction_of_copy_rate_6.3TBps": moved / med / COPY_RATE}
        got = fn()
        torch.cuda.synchronize()
        if name == "torch_float_mean":
            entry["bytes_equal_plain_mode"] = bool(torch.equal(got, ops.blur_synth(frames, windows)))
            entry["note"] = "reads the same frames; writes and re-reads a float32 copy of every window on the way"
        else:
            want = R.blur_synth(host, windows[:2], table if name == "response" else None)        # (K = 1: one key)
            entry["first_keys_equal_the_restatement"] = bool(got[:len(want)].reshape(want.shape).cpu().numpy().tobytes() == want.tobytes())
        result[name] = entry
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
