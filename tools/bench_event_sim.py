#!/usr/bin/env python3
"""Time the event simulator (csrc/event_sim.hip, refid_amd.event_sim) at 1280x720 over one chunk of 64 resident frames.

The clip is synthetic (tools/bench_png_decode.py's ``content``: smooth waves, hard edges and sensor-like noise, panning),
stamped at 240 frames per second, thresholds 0.2 / 0.2.  Measured, each figure the median of ``--rounds`` windows after a
warm-up, with min-max:
  wall     ``EventSimulator.simulate`` over the resident clip, host clock, ending in a device synchronise: reset, count,
           ``torch.cumsum``, the call's one synchronisation, emit, ``torch.sort``, gather;
  device   the same call between two device events on its stream (it contains the host round trip in the middle);
  stages   the launches of one call one by one, a device event between them: where the device time goes.  count and emit
           also as a fraction of the HBM rate (MI355X: 8 TB/s peak) on the bytes they must move: the frames once per pass,
           plus 4 bytes per pixel of counts (count) or 24 bytes per row and 12 per pixel (emit).
Reported as frames/s (intervals per second) and events/s.  For orientation only, the numpy restatement
(tests/event_sim_ref.py) is timed on the first ``--ref-frames`` frames of the same clip on this machine's CPU, and its rows
are compared with the device's.  No threshold is asserted: nothing did this work before.  Prints one JSON line and writes
it to --out (profiles/event_sim_bench.json).  Needs the GPU: there is no CPU path."""
import argparse
import ctypes
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import event_sim_ref as R  # noqa: E402
from bench_png_decode import content, stat  # noqa: E402
from refid_amd import _lib, ops  # noqa: E402
from refid_amd.event_sim import EventSimulator  # noqa: E402

HBM_PEAK = 8.0e12


def staged(sim, frames, stamps_host):
    """One call's launches with a device event between them -> ({stage: seconds}, rows).  The sequence of ``ops.event_sim``."""
    n, h, w = frames.shape[:3]
    L, stream = _lib.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
    stamps_dev = torch.from_numpy(stamps_host).cuda()
    counts = torch.empty((h * w,), dtype=torch.int32, device="cuda")
    totals = torch.zeros((n + 1,), dtype=torch.int64, device="cuda")
    marks[0].record()
    state = ops.event_sim_reset(frames[0], sim.lut)
    marks[1].record()
    desc = _lib.EventSimDesc(frames=frames.data_ptr(), stamps_host=stamps_host.ctypes.data, stamps_dev=stamps_dev.data_ptr(), lut=sim.lut.data_ptr(),
                             state=state.data_ptr(), counts=counts.data_ptr(), totals=totals.data_ptr(), n_frames=n, height=h, width=w,
                             c_pos=sim.c_pos, c_neg=sim.c_neg, lut_min=sim.lut_range[0], lut_max=sim.lut_range[1], stage=_lib.EVENT_SIM_COUNT)
    _lib.check(L.refid_event_sim(ctypes.byref(desc), stream), "count")
    marks[2].record()
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    marks[3].record()
    total = int(ends[-1])
    rows = torch.empty((total, 4), dtype=torch.float32, device="cuda")
    keys = torch.empty((total,), dtype=torch.int64, device="cuda")
    out = torch.empty_like(rows)
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record()
    desc.ends, desc.rows, desc.keys, desc.n_rows, desc.stage = ends.data_ptr(), rows.data_ptr(), keys.data_ptr(), total, _lib.EVENT_SIM_EMIT
    _lib.check(L.refid_event_sim(ctypes.byref(desc), stream), "emit")
    marks[4].record()
    perm = torch.sort(keys)[1]
    marks[5].record()
    desc.perm, desc.sorted, desc.stage = perm.data_ptr(), out.data_ptr(), _lib.EVENT_SIM_GATHER
    _lib.check(L.refid_event_sim(ctypes.byref(desc), stream), "gather")
    marks[6].record()
    marks[6].synchronize()
    ms = lambda a, b: a.elapsed_time(b) * 1e-3        # noqa: E731
    return {"reset": ms(marks[0], marks[1]), "count": ms(marks[1], marks[2]), "cumsum": ms(marks[2], marks[3]), "emit": ms(e0, marks[4]),
            "sort": ms(marks[4], marks[5]), "gather": ms(marks[5], marks[6])}, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64, help="frames of the chunk")
    ap.add_argument("--size", default="720x1280")
    ap.add_argument("--fps", type=float, default=240.0)
    ap.add_argument("--c", type=float, default=0.2, help="both thresholds, natural-log units")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ref-frames", type=int, default=5, help="frames the numpy restatement is timed on (0: skip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "event_sim_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_event_sim.py needs the GPU (there is no CPU path)")
    h, w = (int(v) for v in args.size.split("x"))
    n = args.frames
    host = content(n, h, w, 7)
    stamps = np.arange(n, dtype=np.float64) / args.fps
    frames = torch.from_numpy(host).cuda()
    sim = EventSimulator(h, w, c_pos=args.c, c_neg=args.c)
    events, offsets = sim.simulate(frames, stamps, chunk=n)       # warm-up: code objects, the allocator's blocks, sort's choices
    torch.cuda.synchronize()
    total = int(offsets[-1])
    stage_times, rows = staged(sim, frames, stamps)
    stages_equal = bool(torch.equal(rows, events))
    t_wall, t_dev, t_stage = [], [], {k: [] for k in stage_times}
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        e0.record()
        sim.simulate(frames, stamps, chunk=n)
        e1.record()
        torch.cuda.synchronize()
        t_wall.append(time.perf_counter() - t)
        t_dev.append(e0.elapsed_time(e1) * 1e-3)
        for k, v in staged(sim, frames, stamps)[0].items():
            t_stage[k].append(v)
    wall, dev = statistics.median(t_wall), statistics.median(t_dev)
    frame_bytes = n * h * w * 3
    count_bytes, emit_bytes = frame_bytes + 4 * h * w, frame_bytes + 24 * total + 12 * h * w
    med = {k: statistics.median(v) for k, v in t_stage.items()}
    result = {"bench": "event_sim", "device": torch.cuda.get_device_name(0), "frame": [h, w, 3], "frames": n, "intervals": n - 1, "fps": args.fps,
              "c_pos": args.c, "c_neg": args.c, "events": total, "events_per_pixel_per_interval": total / ((n - 1) * h * w), "rounds": args.rounds,
              "t_is_sorted": bool(torch.all(events[1:, 0] >= events[:-1, 0])), "staged_launches_give_the_same_rows": stages_equal,
              "wall_ms": stat(t_wall, 1e3), "wall_frames_per_s": (n - 1) / wall, "wall_events_per_s": total / wall,
              "device_ms": stat(t_dev, 1e3), "device_frames_per_s": (n - 1) / dev, "device_events_per_s": total / dev,
              "stages_ms": {k: stat(v, 1e3) for k, v in t_stage.items()}, "stages_sum_ms": 1e3 * sum(med.values()),
              "kernels_frames_per_s": (n - 1) / sum(med.values()), "kernels_events_per_s": total / sum(med.values()),
              "count_bytes": count_bytes, "count_fraction_of_hbm_peak_8TBps": count_bytes / med["count"] / HBM_PEAK,
              "emit_bytes": emit_bytes, "emit_fraction_of_hbm_peak_8TBps": emit_bytes / med["emit"] / HBM_PEAK}
    if args.ref_frames >= 2:
        m = min(args.ref_frames, n)
        t = time.perf_counter()
        want = R.simulate(host[:m], stamps[:m], R.reset(host[0], sim.lut_host), sim.lut_host, sim.c_pos, sim.c_neg)
        ref_s = time.perf_counter() - t
        result.update({"restatement_frames": m, "restatement_s": ref_s, "restatement_frames_per_s": (m - 1) / ref_s,
                       "restatement_events_per_s": len(want[0]) / ref_s,
                       "restatement_rows_equal_the_device": bool(events[:offsets[m - 1]].cpu().numpy().tobytes() == want[0].tobytes())})
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
