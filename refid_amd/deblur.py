"""``python -m refid_amd.deblur``: blurry frames + one event stream + a checkpoint -> deblurred PNG frames.

    python -m refid_amd.deblur --opt options/test/HighREV/evhinet.yml --frames seq/blur --events seq/events/*.npz \\
        --stamps seq/exposures.txt --out out/seq

``--opt`` supplies ``network_g``, ``path.pretrain_network_g``, ``datasets.test.num_bins``, ``val.max_minibatch`` and, when
``val.grids`` is set, ``val.crop_size`` (tiled inference); or give ``--checkpoint`` with ``--num-bins``: the network is then
``SingleMultiConnectEVHINet`` with its defaults and ``ev_chn = num_bins``.  ``--frames`` is a directory of 8-bit PNGs
(sorted by name), a ``.npy`` stack (N, H, W, 3) uint8 RGB, or -- decoded on the GPU -- a directory of baseline JPEGs or a
Motion-JPEG ``.avi``; ``--stamps`` a text file with the exposure ``start end`` of
every frame per line, in the events' clock.  Frame k is written to ``{out}/{k:06d}.png``.  ``--niqe PARAMS.npz`` (the
reference's ``niqe_pris_params.npz``) also scores every output frame with NIQE: ``{out}/niqe.txt`` holds one ``file score``
line per frame and a last ``mean`` line over the finite scores, which is printed too.  ``--gt DIR`` (sharp PNGs named as
the output frames) scores every output frame against ground truth while it is on the GPU: ``{out}/scores.txt``, as for
``refid_amd.interpolate``.

``--method edi`` needs no checkpoint: every frame comes from the event-based double integral (``refid_amd.edi``) at the
middle of its exposure, under the same name.  Give ``--m M`` (the frames averaged into a blurry frame, what
``refid_amd.simulate --blur M`` writes: required, since with M = 1 nothing is deblurred; not read with ``--edi-exposure
continuous``), ``--c-pos`` / ``--c-neg`` and ``--eps`` as for ``refid_amd.interpolate``; ``--checkpoint``, ``--opt`` and what only the
network reads (``--num-bins``, ``--crop-size``, ``--stamps-mode``) are refused."""
import sys

from .interpolate import load_frames, load_frames_resident, png_deflate_setting, png_filter_setting, write_niqe  # noqa: F401  (for other callers)
from .interpolate import edi_needs_gpu, edi_settings, load_inputs, load_network, parsed_opt, parser, report_edi, run_and_report, video_settings


def settings(args):
    """(network options, checkpoint path or None, num_bins, max_minibatch, crop_size or None) from --opt, overridden by
    the explicit arguments."""
    net, ckpt, bins, mb, crop = None, None, None, None, None
    if args.opt:
        opt = parsed_opt(args)
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
    ap = parser("python -m refid_amd.deblur", __doc__, "a test YAML: network_g, path.pretrain_network_g, datasets.test.num_bins, val.*",
                "directory of blurry PNG or JPEG frames, a Motion-JPEG .avi, or a .npy stack (N, H, W, 3) uint8 RGB",
                "the exposure 'start end' of every frame, one frame per line")
    ap.add_argument("--num-bins", type=int, help="voxel bins per frame (the network's ev_chn)")
    ap.add_argument("--max-minibatch", type=int, help="frames (with --crop-size: tiles) per network call; default 1")
    ap.add_argument("--crop-size", type=int, help="tiled inference with tiles of this size (val.grids)")
    ap.add_argument("--stamps-mode", choices=("events", "bounds"),
                    help="normalise event times from the first to the last event of a window (events, the default), or from start to end")
    ap.add_argument("--m", type=int, help="--method edi, exposure samples: the frames averaged into a blurry frame (simulate --blur M)")
    args = ap.parse_args(argv)
    video_settings(args)                      # a bad flag exits before anything is loaded
    edi_opt = edi_settings(args, network_only=("num_bins", "crop_size", "stamps_mode"))
    if edi_opt is None and args.m is not None:
        raise SystemExit("--m: needs --method edi")
    if edi_opt is not None and edi_opt["exposure"] == "samples" and args.m is None:
        raise SystemExit("--m: --method edi with --edi-exposure samples needs the number of frames averaged into a blurry frame "
                         "(simulate --blur M); give --m M (1: the frames are sharp), or --edi-exposure continuous")
    if edi_opt is not None:
        edi_needs_gpu("refid_amd.deblur")

    from . import sequence
    if edi_opt is None:
        net_opt, ckpt, bins, mb, crop = settings(args)
    niqe_model, frames, events, stamps = load_inputs(args, "frames")
    if stamps.shape[1] < 2:
        raise SystemExit("--stamps: an exposure 'start end' per line is needed")
    if edi_opt is not None:
        from . import edi
        from ._lib import RefidHipError
        items = sequence.make_pairs(events[:, 0], *sequence.frame_windows(stamps[:, 0], stamps[:, 1]), stamps="bounds")
        try:
            runner = edi.EdiDeblurrer(1 if args.m is None else args.m, max_minibatch=args.max_minibatch or 1, **edi_opt)
        except RefidHipError as ex:
            raise SystemExit(f"--method edi: {ex}")
        run_and_report(runner, args, frames, events, items, niqe_model, "frames", "{name}.png")
        report_edi(runner)
        return 0
    items = sequence.make_pairs(events[:, 0], *sequence.frame_windows(stamps[:, 0], stamps[:, 1]), stamps=args.stamps_mode or "events")
    runner = sequence.SequenceDeblurrer(load_network(net_opt, ckpt), bins, mb, crop)
    run_and_report(runner, args, frames, events, items, niqe_model, "frames", "{name}.png")
    return 0


if __name__ == "__main__":
    sys.exit(main())
