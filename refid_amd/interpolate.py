"""``python -m refid_amd.interpolate``: key frames + one event stream + a checkpoint -> interpolated PNG frames.

    python -m refid_amd.interpolate --opt options/test/GoPro/7skip.yml --frames seq/frames --events seq/events/*.npz \\
        --stamps seq/timestamps.txt --out out/seq

``--opt`` supplies ``network_g``, ``path.pretrain_network_g`` and ``datasets.test.num_*`` (the layout follows the model
type: the ``*Sharp*`` classes take sharp key frames); or give ``--checkpoint`` with ``--n`` / ``--m`` / ``--layout`` and the
released network size.  ``--frames`` is a directory of 8-bit PNGs (sorted by name), a ``.npy`` stack (N, H, W, 3) uint8
RGB, or -- decoded on the GPU -- a directory of baseline JPEGs (``*.jpg`` / ``*.jpeg``) or a Motion-JPEG ``.avi`` such as
``--video`` writes; ``--stamps`` a text file with one key-frame timestamp per line (sharp layout) or an exposure ``start end`` per line
(blur layout), in the events' clock.  Frame f of pair k is written to ``{out}/{k:06d}_{f:02d}.png``.  ``--niqe PARAMS.npz``
(the reference's ``niqe_pris_params.npz``) also scores every output frame with NIQE: ``{out}/niqe.txt`` holds one
``file score`` line per frame and a last ``mean`` line over the finite scores, which is printed too.  ``--gt DIR`` (PNGs
named as the output frames) scores every output frame against ground truth while it is on the GPU: ``{out}/scores.txt``
holds ``file psnr ssim`` per frame and a last ``mean`` line (``python -m refid_amd.score`` scores a finished directory, with
``--crop-border`` and the Y-channel variants).

``--method edi`` needs no checkpoint: the frames come from the event-based double integral (``refid_amd.edi``,
csrc/edi.hip), at the instants the network's outputs stand for and under the same names, so ``--gt``, ``--niqe`` and
``--video`` work as above.  Give ``--n`` (and ``--layout blur --m M`` for blurry key frames), the stream's thresholds
``--c-pos`` / ``--c-neg`` (natural-log units, default 0.2), ``--edi-exposure samples`` (default: a key frame is the mean of M
frames, as ``refid_amd.simulate --blur M`` writes it) or ``continuous`` (a real shutter), and ``--eps``.  ``--checkpoint`` and
``--opt`` are refused.  A last line counts the pixels whose gain had to be clamped and the event rows outside the frame."""
import argparse
import glob
import os
import sys

import numpy as np

RELEASED_NETWORK = dict(type="FinalBidirectionAttenfusion", ev_chn=2, num_encoders=3, base_num_channels=32, num_block=1,
                        num_residual_blocks=2)


def load_frames(path):
    """A directory of PNGs (sorted by name) or a ``.npy`` stack -> uint8 (N, H, W, 3) RGB."""
    from .png import read_png
    if os.path.isdir(path):
        files = sorted(glob.glob(os.path.join(path, "*.png")))
        if not files:
            raise SystemExit(f"--frames: no *.png under {path}")
        imgs = [read_png(f) for f in files]
        imgs = [np.repeat(i[:, :, None], 3, axis=2) if i.ndim == 2 else i for i in imgs]
        if len({i.shape for i in imgs}) != 1:
            raise SystemExit(f"--frames: the PNGs under {path} differ in size")
        return np.stack(imgs)
    stack = np.load(path)
    if stack.dtype != np.uint8 or stack.ndim != 4 or stack.shape[3] != 3:
        raise SystemExit(f"--frames: {path} must hold uint8 (N, H, W, 3), got {stack.dtype} {stack.shape}")
    return stack


def _jpeg_input(path):
    """True for what only the JPEG route reads: a Motion-JPEG ``.avi`` file, or a directory that holds ``*.jpg`` / ``*.jpeg``."""
    if os.path.isdir(path):
        return bool(glob.glob(os.path.join(path, "*.jpg")) or glob.glob(os.path.join(path, "*.jpeg")))
    return str(path).lower().endswith(".avi")


def load_frames_resident(path):
    """``--frames`` of the command lines: a directory of PNGs is inflated by a thread pool and unfiltered on the GPU
    (``sequence.load_png_frames``, csrc/png.hip) into the resident uint8 (N, H, W, 3) tensor the runners take, the same bytes
    ``load_frames`` gives; a ``.npy`` stack, or a machine without a GPU, goes through ``load_frames``.  A directory of JPEGs
    or a Motion-JPEG ``.avi`` goes through ``sequence.load_key_frames`` (host entropy decode, csrc/jpeg_decode.hip); there is
    no host JPEG decoder, so these need the GPU."""
    import torch
    if _jpeg_input(path):
        if not torch.cuda.is_available():
            raise SystemExit("--frames: JPEG key frames need the GPU (a directory of *.jpg / *.jpeg or a Motion-JPEG .avi is decoded by "
                             "csrc/jpeg_decode.hip; without a GPU give PNGs or a .npy stack)")
        from . import sequence
        from ._lib import RefidHipError
        try:
            return sequence.load_key_frames(path)
        except RefidHipError as e:
            raise SystemExit(f"--frames: {e}")
    if not (os.path.isdir(path) and torch.cuda.is_available()):
        return load_frames(path)
    from . import sequence
    from ._lib import RefidHipError
    files = sorted(glob.glob(os.path.join(path, "*.png")))
    if not files:
        raise SystemExit(f"--frames: no *.png under {path}")
    try:
        return sequence.load_png_frames(files)
    except RefidHipError as e:
        raise SystemExit(f"--frames: {e}")


def write_niqe(out_dir, files, scores):
    """``{out_dir}/niqe.txt``: one ``file score`` line per frame, then ``mean`` over the finite scores (nan when there is
    none).  Returns the mean."""
    finite = [s for s in scores if np.isfinite(s)]
    mean = float(np.mean(finite)) if finite else float("nan")
    with open(os.path.join(out_dir, "niqe.txt"), "w") as f:
        for name, s in zip(files, scores):
            f.write(f"{name} {s:.6f}\n")
        f.write(f"mean {mean:.6f}\n")
    return mean


def parsed_opt(args):
    """The options of ``--opt``, parsed once per ``args`` however many settings are read from them; {} without ``--opt``."""
    if getattr(args, "parsed_opt", None) is None:
        from .options import parse
        args.parsed_opt = parse(args.opt, is_train=False) if args.opt else {}
    return args.parsed_opt


def settings(args):
    """(network options, checkpoint path or None, m, n, layout) from --opt, overridden by the explicit arguments."""
    net, ckpt, m, n, layout = None, None, 1, None, None
    if args.opt:
        opt = parsed_opt(args)
        net = dict(opt["network_g"])
        ckpt = opt.get("path", {}).get("pretrain_network_g")
        ds = opt.get("datasets", {}).get("test", {})
        m, n = int(ds.get("num_end_interpolation", 1)), ds.get("num_inter_interpolation")
        layout = "sharp" if "Sharp" in str(opt.get("model_type", "")) else "blur"
    ckpt = args.checkpoint or ckpt
    m = args.m if args.m is not None else m
    n = args.n if args.n is not None else n
    layout = args.layout or layout or "sharp"
    if n is None:
        raise SystemExit("give --opt (datasets.test.num_inter_interpolation) or --n")
    if net is None:
        net = dict(RELEASED_NETWORK, img_chn=6 if layout == "sharp" else 6 + 2 * (m - 1))
    return net, ckpt, int(m), int(n), layout


def _val_setting(args, flag, key, check):
    """The command line's ``flag`` (an attribute of ``args``), else ``val.<key>`` of ``--opt`` through ``check``, whose default
    stands for an absent key or no ``--opt``; a bad value in the file exits with ``check``'s message."""
    from ._lib import RefidHipError
    if getattr(args, flag) is not None:
        return getattr(args, flag)
    try:
        return check((parsed_opt(args).get("val") or {}).get(key), f"--opt: val.{key}")
    except RefidHipError as ex:
        raise SystemExit(str(ex))


def png_filter_setting(args):
    """``--png-filter``, else ``val.png_filter`` of ``--opt``, else 'none' (what ``settings`` leaves out: it is the same
    for both command lines)."""
    from .validation import check_png_filter
    return _val_setting(args, "png_filter", "png_filter", check_png_filter)


def png_deflate_setting(args):
    """``--png-deflate``, else ``val.png_deflate`` of ``--opt``, else 'host'; as ``png_filter_setting``."""
    from .validation import check_png_deflate
    return _val_setting(args, "png_deflate", "png_deflate", check_png_deflate)


def parser(prog, doc, opt_help, frames_help, stamps_help):
    """The arguments both command lines take; the caller adds its own.  ``doc``: the module's docstring."""
    ap = argparse.ArgumentParser(prog=prog, description=doc.split("\n\n")[0])
    ap.add_argument("--opt", help=opt_help)
    ap.add_argument("--checkpoint", help="a .pth with the network's state dict (under 'params' or bare)")
    ap.add_argument("--frames", required=True, help=frames_help)
    ap.add_argument("--events", required=True, nargs="+", help="event .npz files (x, y, timestamp, polarity), in time order")
    ap.add_argument("--stamps", required=True, help=stamps_help)
    ap.add_argument("--out", help="output directory (PNG frames; optional with --video)")
    ap.add_argument("--swap-xy", action="store_true", help="the HighREV files' swapped x / y columns")
    ap.add_argument("--niqe", metavar="PARAMS.npz", help="score every output frame with NIQE (niqe_pris_params.npz) -> niqe.txt")
    ap.add_argument("--gt", metavar="DIR", help="ground-truth PNGs named as the output frames: PSNR and SSIM of every output "
                                                "frame against them -> scores.txt (more: python -m refid_amd.score)")
    ap.add_argument("--png-filter", choices=("none", "adaptive"),
                    help="PNG row filters of the output: none (type 0 on every row) or adaptive (chosen per row on the GPU: "
                         "smaller files, cheaper to write); default: val.png_filter of --opt, else none")
    ap.add_argument("--png-deflate", choices=("host", "device"),
                    help="where the output PNGs are deflated: host (zlib in the writer threads) or device (Huffman codes per "
                         "block on the GPU; the threads only write); default: val.png_deflate of --opt, else host")
    ap.add_argument("--video", metavar="PATH", help="also (or, without --out, only) write the output frames, in order, as one "
                                                    "Motion-JPEG AVI file; JPEG frames are encoded on the GPU")
    ap.add_argument("--video-fps", default="30", help="frames per second of --video: a number or a fraction such as 30000/1001")
    ap.add_argument("--video-quality", default="90", help="JPEG quality of --video, 1 .. 100")
    ap.add_argument("--video-subsampling", default="420", help="chroma subsampling of --video: 420 or 444")
    ap.add_argument("--method", choices=("network", "edi"), default="network",
                    help="network (default): the checkpoint's network; edi: the event-based double integral (refid_amd.edi), "
                         "which needs no checkpoint")
    ap.add_argument("--c-pos", type=float, help="--method edi: the stream's positive contrast threshold, natural-log units (default 0.2)")
    ap.add_argument("--c-neg", type=float, help="--method edi: the negative contrast threshold (default 0.2)")
    ap.add_argument("--edi-exposure", choices=("samples", "continuous"),
                    help="--method edi: a blurry key frame is the mean of M frames (samples, the default: what simulate --blur M "
                         "writes) or of a continuous shutter")
    ap.add_argument("--eps", type=float, help="--method edi: the offset inside the logarithm (default 1e-3, the simulator's)")
    return ap


EDI_FLAGS = ("c_pos", "c_neg", "edi_exposure", "eps")


def edi_settings(args, network_only=()):
    """None for ``--method network`` (a flag of the other method exits naming it); for ``--method edi`` the keywords of the
    ``refid_amd.edi`` runners.  ``network_only``: the caller's own flags that only the network reads; under ``--method edi``
    they are refused, not ignored.  A bad flag exits before anything is loaded."""
    flag = lambda name: "--" + name.replace("_", "-")             # noqa: E731
    if args.method != "edi":
        for name in EDI_FLAGS:
            if getattr(args, name) is not None:
                raise SystemExit(f"{flag(name)}: needs --method edi")
        return None
    if args.checkpoint:
        raise SystemExit("--checkpoint: --method edi runs no network and takes no checkpoint")
    if args.opt:
        raise SystemExit("--opt: --method edi runs no network: give its settings as flags (--c-pos, --c-neg, --edi-exposure, --eps)")
    for name in network_only:
        if getattr(args, name) is not None:
            raise SystemExit(f"{flag(name)}: --method edi runs no network and does not read it (the exposure bounds of --stamps and "
                             "the events between them are all it takes)")
    out = dict(c_pos=0.2 if args.c_pos is None else args.c_pos, c_neg=0.2 if args.c_neg is None else args.c_neg,
               exposure=args.edi_exposure or "samples", eps=1e-3 if args.eps is None else args.eps)
    for name in ("c_pos", "c_neg"):
        if not 2.0 ** -16 <= out[name] <= 16.0:                   # (a NaN fails both)
            raise SystemExit(f"{flag(name)}: {out[name]} must be at least 2^-16 and at most 16")
    if not 0.0 <= out["eps"] < float("inf"):
        raise SystemExit(f"--eps: {out['eps']} must be finite and not negative")
    return out


def edi_needs_gpu(prog):
    """The last check before anything is loaded: without a GPU ``--method edi`` says so and stops."""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(f"{prog} --method edi needs the GPU: the double integral runs in csrc/edi.hip and has no host fallback")


def report_edi(runner):
    print(f"edi: {runner.clamped} clamped pixels, {runner.dropped} dropped event rows")


def video_settings(args):
    """The keywords ``run`` takes for --video (empty without it); a bad value exits naming its flag.  Also: one of --out and
    --video is needed, and the score files need --out."""
    from fractions import Fraction
    from ._lib import RefidHipError
    from .validation import check_video_options
    if not args.out and not args.video:
        raise SystemExit("give --out, --video or both")
    if not args.out and (args.gt or args.niqe):
        raise SystemExit("--gt and --niqe write their files into --out: give --out")
    if not args.video:
        return {}
    try:
        fps = Fraction(args.video_fps)
    except (ValueError, ZeroDivisionError):
        raise SystemExit(f"--video-fps: {args.video_fps!r} is not a number or a fraction") from None
    try:
        quality = int(args.video_quality)
    except ValueError:
        raise SystemExit(f"--video-quality: {args.video_quality!r} is not an integer 1 .. 100") from None
    try:
        check_video_options(fps, quality, args.video_subsampling, None, "--video")
    except RefidHipError as ex:
        raise SystemExit(str(ex).replace("--video: video_", "--video-")) from None
    out = dict(video=args.video, video_fps=fps, video_quality=quality, video_subsampling=args.video_subsampling)
    if getattr(args, "video_no_keys", False):
        out["video_keys"] = False
    return out


def load_inputs(args, noun):
    """(NIQE model or None, frames, events, stamps) of a command line; ``noun``: what --stamps counts ('key frames')."""
    from . import sequence
    niqe_model = None
    if args.niqe:
        from .niqe import NiqeModel
        niqe_model = NiqeModel.load(args.niqe)
    frames = load_frames_resident(args.frames)
    events = sequence.load_event_npz(args.events, swap_xy=args.swap_xy)
    stamps = np.loadtxt(args.stamps, dtype=np.float64, ndmin=2)
    if stamps.shape[0] != frames.shape[0]:
        raise SystemExit(f"--stamps: {stamps.shape[0]} lines for {frames.shape[0]} {noun}")
    return niqe_model, frames, events, stamps


def load_network(net_opt, ckpt):
    """The network on the GPU with the checkpoint's weights ('params' or bare, with or without the ``module.`` prefix)."""
    import torch
    from .archs import define_network
    net = define_network(net_opt).to("cuda")
    if ckpt:
        state = torch.load(ckpt, map_location="cpu")
        state = state.get("params", state)
        net.load_state_dict({(k[7:] if k.startswith("module.") else k): v for k, v in state.items()}, strict=True)
    else:
        print("warning: no checkpoint given: the network runs with its initial weights", file=sys.stderr)
    return net


def run_and_report(runner, args, frames, events, items, niqe_model, noun, file_name):
    """Runs ``items`` (named by their index) into --out and, with --niqe, writes niqe.txt; ``file_name``: the format of an
    output file's name from ``name`` and the frame ``f`` of the item."""
    names = [f"{k:06d}" for k in range(len(items))]
    from ._lib import RefidHipError
    try:
        runner.run(frames, events, items, out_dir=args.out, names=names, niqe=niqe_model, png_filter=png_filter_setting(args),
                   png_deflate=png_deflate_setting(args), gt=args.gt, **video_settings(args))
    except RefidHipError as ex:
        if args.gt and "ground truth" in str(ex):
            raise SystemExit(f"--gt: {ex}")
        raise
    if args.out:
        print(f"{len(items)} {noun} -> {args.out}")
    if args.video:
        print(f"{len(items)} {noun} -> {', '.join(runner.video_paths)}")
    if args.gt:
        from .score import format_lines
        sc = runner.scores
        lines = format_lines([file_name.format(name=name, f=f) for name, f, _ in sc], ["psnr", "ssim"],
                             [(s.psnr, s.ssim) for _, _, s in sc])
        with open(os.path.join(args.out, "scores.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        print(f"scores against {args.gt}: {lines[-1]} over {len(sc)} frames -> {os.path.join(args.out, 'scores.txt')}")
    if niqe_model is not None:
        scores = runner.niqe_scores
        mean = write_niqe(args.out, [file_name.format(name=name, f=f) for name, f, _ in scores], [s for _, _, s in scores])
        print(f"NIQE mean {mean:.6f} over {len(scores)} frames -> {os.path.join(args.out, 'niqe.txt')}")


def main(argv=None):
    ap = parser("python -m refid_amd.interpolate", __doc__, "a test YAML: network_g, path.pretrain_network_g, datasets.test.num_*",
                "directory of PNG or JPEG key frames, a Motion-JPEG .avi, or a .npy stack (N, H, W, 3) uint8 RGB",
                "key-frame timestamps, one per line ('start end' per line for blur)")
    ap.add_argument("--n", type=int, help="frames to interpolate between two key frames")
    ap.add_argument("--m", type=int, help="frames to recover from each blurry key frame (blur layout)")
    ap.add_argument("--layout", choices=("sharp", "blur"))
    ap.add_argument("--max-minibatch", type=int, default=2)
    ap.add_argument("--video-no-keys", action="store_true",
                    help="--video holds the interpolated frames only (default for sharp key frames: the key frames too, in place)")
    args = ap.parse_args(argv)
    video_settings(args)                      # a bad flag exits before anything is loaded
    edi_opt = edi_settings(args)

    from . import sequence
    if edi_opt is None:
        net_opt, ckpt, m, n, layout = settings(args)
    else:
        if args.n is None:
            raise SystemExit("--method edi: give --n")
        layout = args.layout or "sharp"
        if layout == "blur" and edi_opt["exposure"] == "samples" and args.m is None:
            raise SystemExit("--m: --method edi --layout blur with --edi-exposure samples needs the number of frames averaged into a "
                             "blurry key frame (simulate --blur M); give --m M, or --edi-exposure continuous")
        m, n = (1 if args.m is None else args.m), args.n
        edi_needs_gpu("refid_amd.interpolate")
    niqe_model, frames, events, stamps = load_inputs(args, "key frames")
    if layout == "sharp":
        windows = sequence.sharp_windows(stamps[:, 0])
    elif stamps.shape[1] >= 2:
        windows = sequence.exposure_windows(stamps[:, 0], stamps[:, 1])
    else:
        raise SystemExit("--stamps: the blur layout needs an exposure 'start end' per line")
    if edi_opt is not None:
        from . import edi
        from ._lib import RefidHipError
        pairs = sequence.make_pairs(events[:, 0], *windows, stamps="bounds") if layout == "sharp" else \
            edi.exposure_pairs(stamps[:, 0], stamps[:, 1])
        try:
            runner = edi.EdiInterpolator(m, n, layout, max_minibatch=args.max_minibatch, **edi_opt)
        except RefidHipError as ex:
            raise SystemExit(f"--method edi: {ex}")
        run_and_report(runner, args, frames, events, pairs, niqe_model, "pairs", "{name}_{f:02d}.png")
        report_edi(runner)
        return 0
    pairs = sequence.make_pairs(events[:, 0], *windows)
    runner = sequence.SequenceInterpolator(load_network(net_opt, ckpt), m, n, layout, args.max_minibatch)
    run_and_report(runner, args, frames, events, pairs, niqe_model, "pairs", "{name}_{f:02d}.png")
    return 0


if __name__ == "__main__":
    sys.exit(main())
