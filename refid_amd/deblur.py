"""``python -m refid_amd.deblur``: blurry frames + one event stream + a checkpoint -> deblurred PNG frames.

    python -m refid_amd.deblur --opt options/test/HighREV/evhinet.yml --frames seq/blur --events seq/events/*.npz \\
        --stamps seq/exposures.txt --out out/seq

``--opt`` supplies ``network_g``, ``path.pretrain_network_g``, ``datasets.test.num_bins``, ``val.max_minibatch`` and, when
``val.grids`` is set, ``val.crop_size`` (tiled inference); or give ``--checkpoint`` with ``--num-bins``: the network is then
``SingleMultiConnectEVHINet`` with its defaults and ``ev_chn = num_bins``.  ``--frames`` is a directory of 8-bit PNGs
(sorted by name) or a ``.npy`` stack (N, H, W, 3) uint8 RGB; ``--stamps`` a text file with the exposure ``start end`` of
every frame per line, in the events' clock.  Frame k is written to ``{out}/{k:06d}.png``.  ``--niqe PARAMS.npz`` (the
reference's ``niqe_pris_params.npz``) also scores every output frame with NIQE: ``{out}/niqe.txt`` holds one ``file score``
line per frame and a last ``mean`` line over the finite scores, which is printed too."""
import argparse
import os
import sys

import numpy as np

from .interpolate import load_frames, load_frames_resident, png_filter_setting, write_niqe  # noqa: F401  (load_frames: for other callers)


def settings(args):
    """(network options, checkpoint path or None, num_bins, max_minibatch, crop_size or None) from --opt, overridden by
    the explicit arguments."""
    net, ckpt, bins, mb, crop = None, None, None, None, None
    if args.opt:
        from .options import parse
        opt = parse(args.opt, is_train=False)
        net = dict(opt["network_g"])
        ckpt = opt.get("path", {}).get("pretrain_network_g")
        bins = opt.get("datasets", {}).get("test", {}).get("num_bins")
        val = opt.get("val") or {}
        mb = val.get("max_minibatch")
        if val.get("grids") is not None:
            crop = val.get("crop_size")
            if crop is None:
                raise SystemExit("--opt: val.grids needs val.crop_size")
    ckpt = args.checkpoint or ckpt
    bins = args.num_bins if args.num_bins is not None else bins
    mb = args.max_minibatch if args.max_minibatch is not None else mb
    crop = args.crop_size if args.crop_size is not None else crop
    if bins is None:
        raise SystemExit("give --opt (datasets.test.num_bins) or --num-bins")
    if net is None:
        net = dict(type="SingleMultiConnectEVHINet", ev_chn=int(bins))
    return net, ckpt, int(bins), int(mb or 1), (None if crop is None else int(crop))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m refid_amd.deblur", description=__doc__.split("\n\n")[0])
    ap.add_argument("--opt", help="a test YAML: network_g, path.pretrain_network_g, datasets.test.num_bins, val.*")
    ap.add_argument("--checkpoint", help="a .pth with the network's state dict (under 'params' or bare)")
    ap.add_argument("--num-bins", type=int, help="voxel bins per frame (the network's ev_chn)")
    ap.add_argument("--frames", required=True, help="directory of blurry PNG frames, or a .npy stack (N, H, W, 3) uint8 RGB")
    ap.add_argument("--events", required=True, nargs="+", help="event .npz files (x, y, timestamp, polarity), in time order")
    ap.add_argument("--stamps", required=True, help="the exposure 'start end' of every frame, one frame per line")
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--max-minibatch", type=int, help="frames (with --crop-size: tiles) per network call; default 1")
    ap.add_argument("--crop-size", type=int, help="tiled inference with tiles of this size (val.grids)")
    ap.add_argument("--swap-xy", action="store_true", help="the HighREV files' swapped x / y columns")
    ap.add_argument("--stamps-mode", choices=("events", "bounds"), default="events",
                    help="normalise event times from the first to the last event of a window, or from start to end")
    ap.add_argument("--niqe", metavar="PARAMS.npz", help="score every output frame with NIQE (niqe_pris_params.npz) -> niqe.txt")
    ap.add_argument("--png-filter", choices=("none", "adaptive"),
                    help="PNG row filters of the output: none (type 0 on every row) or adaptive (chosen per row on the GPU: "
                         "smaller files, cheaper to write); default: val.png_filter of --opt, else none")
    args = ap.parse_args(argv)

    import torch
    from . import sequence
    from .archs import define_network
    net_opt, ckpt, bins, mb, crop = settings(args)
    niqe_model = None
    if args.niqe:
        from .niqe import NiqeModel
        niqe_model = NiqeModel.load(args.niqe)
    frames = load_frames_resident(args.frames)
    events = sequence.load_event_npz(args.events, swap_xy=args.swap_xy)
    stamps = np.loadtxt(args.stamps, dtype=np.float64, ndmin=2)
    if stamps.shape[0] != frames.shape[0]:
        raise SystemExit(f"--stamps: {stamps.shape[0]} lines for {frames.shape[0]} frames")
    if stamps.shape[1] < 2:
        raise SystemExit("--stamps: an exposure 'start end' per line is needed")
    items = sequence.make_pairs(events[:, 0], *sequence.frame_windows(stamps[:, 0], stamps[:, 1]), stamps=args.stamps_mode)
    net = define_network(net_opt).to("cuda")
    if ckpt:
        state = torch.load(ckpt, map_location="cpu")
        state = state.get("params", state)
        net.load_state_dict({(k[7:] if k.startswith("module.") else k): v for k, v in state.items()}, strict=True)
    else:
        print("warning: no checkpoint given: the network runs with its initial weights", file=sys.stderr)
    names = [f"{k:06d}" for k in range(len(items))]
    runner = sequence.SequenceDeblurrer(net, bins, mb, crop)
    runner.run(frames, events, items, out_dir=args.out, names=names, niqe=niqe_model, png_filter=png_filter_setting(args))
    print(f"{len(items)} frames -> {args.out}")
    if niqe_model is not None:
        mean = write_niqe(args.out, [f"{name}.png" for name, _, _ in runner.niqe_scores], [s for _, _, s in runner.niqe_scores])
        print(f"NIQE mean {mean:.6f} over {len(runner.niqe_scores)} frames -> {os.path.join(args.out, 'niqe.txt')}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
