"""``python -m refid_amd.simulate``: high-frame-rate frames -> simulated events (the ESIM model, csrc/event_sim.hip).

    python -m refid_amd.simulate --frames clip240/ --fps 240 --out sim --split 8
    python -m refid_amd.interpolate --checkpoint net.pth --n 7 --frames sim/keys --events sim/events/*.npz \\
        --stamps sim/key_stamps.txt --gt sim/gt --out sim/out

``--frames`` is what ``refid_amd.interpolate`` takes: a directory of PNGs or baseline JPEGs, a Motion-JPEG ``.avi`` or a
``.npy`` stack (N, H, W, 3) uint8.  The frames' time stamps come from ``--fps F`` (frame k at k / F seconds) or from
``--stamps FILE`` (one stamp per line).  ``{out}/events/{k:06d}.npz`` holds the events of the interval from frame k to frame
k + 1 in the reference's layout (``x``, ``y``, ``timestamp``, ``polarity``), ``{out}/stamps.txt`` the stamps.  ``--split S`` also
writes every S-th frame to ``{out}/keys/{i:06d}.png`` with ``{out}/key_stamps.txt``, and the frames between key i and key
i + 1 to ``{out}/gt/{i:06d}_{f:02d}.png``, f = 0 .. S - 2, the names ``refid_amd.interpolate --n S-1`` gives its outputs: the
second command above then interpolates the key frames from the simulated events and scores the result against the
held-out frames.  Frames behind the last key frame are simulated but belong to no pair.

    python -m refid_amd.simulate --frames clip240/ --fps 240 --out sim --blur 11 --gap 1
    python -m refid_amd.interpolate --checkpoint net.pth --layout blur --m 11 --n 1 --frames sim/keys \\
        --events sim/events/*.npz --stamps sim/key_stamps.txt --gt sim/gt --out sim/out
    python -m refid_amd.deblur --checkpoint evhinet.pth --num-bins 6 --frames sim/keys --events sim/events/*.npz \\
        --stamps sim/key_stamps.txt --gt sim/gt_mid --out sim/deblur

``--blur M --gap N`` (instead of ``--split``) writes BLURRY key frames, synthesised on the GPU (``refid_amd.blur_synth``,
csrc/blur_synth.hip), in the reference's GoPro indexing (basicsr/data/image_npy_dataset.py:75-86): with P = M + N, key i
is the average of the sharp frames [iP, iP + M), written to ``{out}/keys/{i:06d}.png``; ``{out}/key_stamps.txt`` holds
``start end`` per line, the stamps of the first and of the last averaged frame; ``{out}/gt/{i:06d}_{f:02d}.png``,
f = 0 .. 2M + N - 1, are the sharp frames iP + f of pair i, the names ``refid_amd.interpolate --layout blur --m M --n N``
gives its outputs; for odd M ``{out}/gt_mid/{i:06d}.png`` is the sharp frame iP + M // 2 in the middle of key i's
exposure, the target of ``refid_amd.deblur --gt``.  ``--blur-gamma G`` (1 .. 3) averages in linear light, (c / 255)^G at
24 bits, as GoPro's ``blur_gamma`` frames are made; without it the codes are averaged, as in ``blur/``.  The events are
simulated from the sharp frames either way.

``--c-pos`` / ``--c-neg`` are the contrast thresholds in natural-log units, ``--sigma-c`` the standard deviation of their
per-pixel spread (seeded by ``--seed``), ``--eps`` the offset inside the logarithm, ``--chunk`` the frames per device call.
The simulator runs on the GPU only."""
import argparse
import os
import sys

import numpy as np


def _stamps(args, n):
    if (args.fps is None) == (args.stamps is None):
        raise SystemExit("give exactly one of --fps and --stamps")
    if args.fps is not None:
        from fractions import Fraction
        try:
            fps = Fraction(args.fps)
        except (ValueError, ZeroDivisionError):
            raise SystemExit(f"--fps: {args.fps!r} is not a number or a fraction") from None
        if fps <= 0:
            raise SystemExit(f"--fps: {args.fps} must be positive")
        return None if n is None else np.array([float(Fraction(k) / fps) for k in range(n)], dtype=np.float64)
    if n is None:
        return None
    try:
        stamps = np.loadtxt(args.stamps, dtype=np.float64, ndmin=1)
    except (OSError, ValueError) as e:
        raise SystemExit(f"--stamps: {e}") from None
    if stamps.ndim != 1 or stamps.shape[0] != n:
        raise SystemExit(f"--stamps: {stamps.shape[0]} lines for {n} frames (one stamp per line)")
    if not np.all(np.isfinite(stamps)) or not np.all(stamps[1:] > stamps[:-1]):
        raise SystemExit("--stamps: the stamps must be finite and strictly increasing")
    return stamps


def _write_stamps(path, stamps):
    with open(path, "w") as f:
        for s in stamps:
            f.write(f"{float(s)!r}\n")


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m refid_amd.simulate", description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", required=True, help="directory of PNG or JPEG frames, a Motion-JPEG .avi, or a .npy stack (N, H, W, 3) uint8")
    ap.add_argument("--fps", help="frames per second of the clip: a number or a fraction such as 240000/1001")
    ap.add_argument("--stamps", help="a text file with one time stamp per frame, strictly increasing")
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--c-pos", type=float, default=0.2, help="threshold of positive events, natural-log units (default 0.2)")
    ap.add_argument("--c-neg", type=float, default=0.2, help="threshold of negative events (default 0.2)")
    ap.add_argument("--sigma-c", type=float, default=0.0, help="per-pixel spread of the thresholds (default 0: one threshold)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the per-pixel thresholds")
    ap.add_argument("--eps", type=float, default=1e-3, help="offset inside the logarithm (default 1e-3)")
    ap.add_argument("--chunk", type=int, default=64, help="frames per device call, 2 .. 512 (default 64)")
    ap.add_argument("--bgr", action="store_true", help="the frames are BGR")
    ap.add_argument("--split", type=int, metavar="S", help="also write every S-th frame as a key frame and the others as ground truth")
    ap.add_argument("--blur", type=int, metavar="M", help="also write blurry key frames, each the average of M frames, and the sharp frames as ground truth")
    ap.add_argument("--gap", type=int, metavar="N", help="with --blur: frames between the exposures of two blurry key frames")
    ap.add_argument("--blur-gamma", type=float, metavar="G", help="with --blur: average in linear light, (c / 255)^G, 1 .. 3 (default: average the codes)")
    args = ap.parse_args(argv)

    from . import _lib, event_sim
    from ._lib import RefidHipError
    _stamps(args, None)                      # bad flags exit before anything is loaded
    if not 2 <= args.chunk <= _lib.EVENT_SIM_MAX_FRAMES:
        raise SystemExit(f"--chunk: {args.chunk} must be 2 .. {_lib.EVENT_SIM_MAX_FRAMES}")
    if args.split is not None and not 2 <= args.split <= 100:
        raise SystemExit(f"--split: {args.split} must be 2 .. 100 (S - 1 held-out frames between two key frames)")
    if not args.eps > 0.0:
        raise SystemExit(f"--eps: {args.eps} must be positive")
    if not args.sigma_c >= 0.0:
        raise SystemExit(f"--sigma-c: {args.sigma_c} must not be negative")
    bound = event_sim.min_threshold(event_sim.default_lut(args.eps))
    for flag, c in (("--c-pos", args.c_pos), ("--c-neg", args.c_neg)):
        if not np.isfinite(c) or not c < 32768 or event_sim.to_fixed(c) < bound:
            raise SystemExit(f"{flag}: {c} must be at least {bound / event_sim.FIXED_ONE:.4f} ({bound} in units of 2^-16: at most "
                             f"{_lib.EVENT_SIM_CAP} events per pixel between two frames)")
    if args.blur is not None and args.split is not None:
        raise SystemExit("--blur and --split exclude each other: blurry or sharp key frames")
    if args.blur is None:
        for flag, value in (("--gap", args.gap), ("--blur-gamma", args.blur_gamma)):
            if value is not None:
                raise SystemExit(f"{flag}: needs --blur M")
    else:
        if args.gap is None:
            raise SystemExit("--blur: needs --gap N, the frames between two exposures")
        if not 1 <= args.blur <= _lib.BLUR_MAX_COUNT:
            raise SystemExit(f"--blur: {args.blur} must be 1 .. {_lib.BLUR_MAX_COUNT} frames per blurry key frame")
        if not 0 <= args.gap <= 100:
            raise SystemExit(f"--gap: {args.gap} must be 0 .. 100")
        if 2 * args.blur + args.gap > 100:
            raise SystemExit(f"--blur {args.blur} --gap {args.gap}: a pair has 2 M + N = {2 * args.blur + args.gap} ground-truth frames, "
                             f"100 are the most (two digits in their names)")
        if args.blur_gamma is not None and not 1.0 <= args.blur_gamma <= 3.0:
            raise SystemExit(f"--blur-gamma: {args.blur_gamma} must be 1 .. 3")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("refid_amd.simulate needs the GPU: the event simulator is csrc/event_sim.hip and has no host fallback")

    from .interpolate import load_frames_resident
    from .png import write_png
    frames = load_frames_resident(args.frames)
    n = int(frames.shape[0])
    if n < 2:
        raise SystemExit(f"--frames: {n} frame, at least 2 are needed")
    if args.blur is not None and n < args.blur:
        raise SystemExit(f"--frames: {n} frames do not hold one blurry key frame of --blur {args.blur}")
    stamps = _stamps(args, n)
    try:
        sim = event_sim.EventSimulator(int(frames.shape[1]), int(frames.shape[2]), args.c_pos, args.c_neg, sigma=args.sigma_c, seed=args.seed,
                                       eps=args.eps)
        os.makedirs(args.out, exist_ok=True)
        sim.reset(frames[0], bgr=args.bgr)
        total = 0
        for at in range(0, n - 1, args.chunk - 1):           # chunk by chunk: the rows of a chunk leave before the next is made
            rows, offsets = sim.step(frames[at:at + args.chunk], stamps[at:at + args.chunk], bgr=args.bgr)
            event_sim.save_event_npz(os.path.join(args.out, "events"), rows, offsets, first=at)
            total += int(offsets[-1])
    except RefidHipError as e:
        raise SystemExit(str(e))
    _write_stamps(os.path.join(args.out, "stamps.txt"), stamps)
    print(f"{total} events of {n - 1} intervals -> {os.path.join(args.out, 'events')}")
    if args.split:
        s = args.split
        host = frames.cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)
        if args.bgr:
            host = host[..., ::-1]
        keys = list(range(0, n, s))
        for d in ("keys", "gt"):
            os.makedirs(os.path.join(args.out, d), exist_ok=True)
        for i, k in enumerate(keys):
            write_png(os.path.join(args.out, "keys", f"{i:06d}.png"), np.ascontiguousarray(host[k]))
            if i + 1 < len(keys):
                for f in range(s - 1):
                    write_png(os.path.join(args.out, "gt", f"{i:06d}_{f:02d}.png"), np.ascontiguousarray(host[k + 1 + f]))
        _write_stamps(os.path.join(args.out, "key_stamps.txt"), stamps[keys])
        print(f"{len(keys)} key frames -> {os.path.join(args.out, 'keys')}, {(len(keys) - 1) * (s - 1)} held-out frames -> "
              f"{os.path.join(args.out, 'gt')}")
    if args.blur is not None:
        from . import blur_synth
        m, period = args.blur, args.blur + args.gap
        try:
            resident = frames if torch.is_tensor(frames) and frames.is_cuda else torch.as_tensor(np.ascontiguousarray(frames)).to("cuda")
            keys, windows = blur_synth.synthesize(resident, m, args.gap, gamma=args.blur_gamma)
        except RefidHipError as e:
            raise SystemExit(f"--blur: {e}")
        host, blurry = resident.cpu().numpy(), keys.cpu().numpy()
        if args.bgr:
            host, blurry = host[..., ::-1], blurry[..., ::-1]
        k, mid = int(windows.shape[0]), m % 2 == 1
        for d in ("keys", "gt") + (("gt_mid",) if mid else ()):
            os.makedirs(os.path.join(args.out, d), exist_ok=True)
        for i in range(k):
            write_png(os.path.join(args.out, "keys", f"{i:06d}.png"), np.ascontiguousarray(blurry[i]))
            if mid:
                write_png(os.path.join(args.out, "gt_mid", f"{i:06d}.png"), np.ascontiguousarray(host[i * period + m // 2]))
            if i + 1 < k:
                for f in range(2 * m + args.gap):
                    write_png(os.path.join(args.out, "gt", f"{i:06d}_{f:02d}.png"), np.ascontiguousarray(host[i * period + f]))
        with open(os.path.join(args.out, "key_stamps.txt"), "w") as f:
            for start, end in blur_synth.exposures(stamps, windows):
                f.write(f"{float(start)!r} {float(end)!r}\n")
        print(f"{k} blurry key frames of {m} frames -> {os.path.join(args.out, 'keys')}, {(k - 1) * (2 * m + args.gap)} sharp frames -> "
              f"{os.path.join(args.out, 'gt')}")
        if mid:
            print(f"{k} mid-exposure frames -> {os.path.join(args.out, 'gt_mid')}")
        else:
            print(f"no gt_mid: --blur {m} is even, an exposure has no middle frame")
    return 0


if __name__ == "__main__":
    sys.exit(main())
