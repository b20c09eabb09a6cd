"""Scores of uint8 frames against ground truth, as the restoration literature reports them: all of ``calculate_psnr`` and
``calculate_ssim`` of the reference's basicsr/metrics/psnr_ssim.py -- ``crop_border``, and with ``test_y_channel`` the PSNR on
the BT.601 Y plane and the 2-D 11x11 SSIM of ``_ssim_cly`` -- for frames that are already on the device as uint8
(..., H, W, 3): another method's results, a previous run's output directory, the frames ``load_png_frames`` has just
decoded, the frames ``metrics.val_tail`` has just written.

    python -m refid_amd.score --pred out/seq --gt data/seq/gt --crop-border 4 --y --out scores.txt
    python -m refid_amd.score --pred visualization/val --gt-suffix _gt          # the validation dumps X.png / X_gt.png

The per-pixel work is csrc/score.hip (``ops.score_u8``); what comes back is four 8-byte words per frame.  The arithmetic
contract (include/refid_hip.h, INTEGRATION.md "Scoring against ground truth") is shared with the numpy restatement in
tests/score_ref.py.  ``ssim`` is the reference's 3-D variant, bit for bit what ``metrics.val_tail`` gives for the same
uint8 frames.  The YAML keys ``crop_border`` / ``test_y_channel`` stay refused by ``metrics.check_metric_options``: the
validation loop's numbers do not change; this module is the new surface."""
import collections
import math
import os
import sys

from ._lib import RefidHipError
from .metrics import psnr_from_sqerr

Scores = collections.namedtuple("Scores", "psnr ssim psnr_y ssim_y")
COLUMNS = Scores._fields


def psnr_y_from_sq(sq_y, count):
    """calculate_psnr(test_y_channel=True)'s last lines from the sum of the float32 squared differences of the Y planes."""
    mse = sq_y / count
    return float("inf") if mse == 0 else 20.0 * math.log10(255.0 / math.sqrt(mse))


def scores_from_words(words, hc, wc, psnr=True, ssim=True, psnr_y=False, ssim_y=False):
    """``words``: the (4, nf) int64 host tensor of ``ops.score_u8`` for cropped frames of (hc, wc) -> ``Scores`` of per-frame
    lists (None for what was not asked for)."""
    import torch
    f64 = words.view(torch.float64)
    n = hc * wc
    return Scores([psnr_from_sqerr(v, 3 * n) for v in words[0].tolist()] if psnr else None,
                  [v / (3 * n) for v in f64[2].tolist()] if ssim else None,
                  [psnr_y_from_sq(v, n) for v in f64[1].tolist()] if psnr_y else None,
                  [v / n for v in f64[3].tolist()] if ssim_y else None)


def _as_device_u8(t, device=None):
    import numpy as np
    import torch
    if not torch.is_tensor(t):
        t = np.ascontiguousarray(t)
        t = torch.from_numpy(t if t.flags.writeable else t.copy())
    if t.dtype != torch.uint8 or t.dim() < 3 or t.shape[-1] != 3:
        raise RefidHipError(f"score: uint8 frames (..., H, W, 3) are required, got {t.dtype} {tuple(t.shape)}")
    return t if t.is_cuda else t.to("cuda" if device is None else device)


def score_u8(pred_u8, gt_u8, *, bgr=False, crop_border=0, psnr=True, ssim=True, psnr_y=False, ssim_y=False):
    """``calculate_psnr`` / ``calculate_ssim`` (``crop_border``; ``psnr_y`` / ``ssim_y``: their ``test_y_channel=True``) per
    frame of two uint8 (..., H, W, 3) frame sets of one shape: CUDA tensors, or host tensors / numpy arrays (uploaded).
    ``bgr``: the channel order of both (the reference takes BGR; the PNG path here holds RGB); it matters to the Y
    plane only.  One device->host copy for the call.  Returns ``Scores(psnr, ssim, psnr_y, ssim_y)``, each a per-frame list
    or None."""
    from . import ops
    pred_u8 = _as_device_u8(pred_u8)
    gt_u8 = _as_device_u8(gt_u8, pred_u8.device)
    words = ops.score_u8(pred_u8, gt_u8, bgr, crop_border, psnr, psnr_y, ssim, ssim_y)
    cb = int(crop_border)
    return scores_from_words(words.cpu(), int(pred_u8.shape[-3]) - 2 * cb, int(pred_u8.shape[-2]) - 2 * cb, psnr, ssim,
                             psnr_y, ssim_y)


class FrameScorer:
    """``score_u8`` for loops: ``add`` queues the kernels on the current stream and copies the four words per frame, without
    blocking, into pinned memory; nothing synchronises before ``finish``, which returns one ``Scores`` over all frames in
    the order they were added (frame sizes may differ between calls).  ``capacity``: frames per pinned block (a call with
    more frames gets a block of its own)."""

    def __init__(self, *, bgr=False, crop_border=0, psnr=True, ssim=True, psnr_y=False, ssim_y=False, capacity=256):
        self.bgr, self.crop_border = bool(bgr), int(crop_border)
        self.want = (bool(psnr), bool(ssim), bool(psnr_y), bool(ssim_y))
        if self.crop_border < 0:
            raise RefidHipError(f"FrameScorer: crop_border {crop_border} is negative")
        if not any(self.want):
            raise RefidHipError("FrameScorer: no score was asked for")
        self.capacity = int(capacity)
        self._block, self._used = None, 0          # the pinned block being filled: 1-D int64
        self._calls = []                           # (pinned segment of 4 * nf words, nf, hc, wc)
        self._stream = None

    def __len__(self):
        return sum(c[1] for c in self._calls)

    def add(self, pred_u8, gt_u8):
        """Frames of one size: uint8 CUDA (..., H, W, 3), both of one shape.  Does not synchronise."""
        import torch
        from . import ops
        psnr, ssim, psnr_y, ssim_y = self.want
        words = ops.score_u8(pred_u8, gt_u8, self.bgr, self.crop_border, psnr, psnr_y, ssim, ssim_y)
        n = words.numel()
        if self._block is None or self._used + n > self._block.numel():
            self._block, self._used = torch.empty(max(n, 4 * self.capacity), dtype=torch.int64).pin_memory(), 0
        seg = self._block[self._used:self._used + n]
        self._used += n
        seg.copy_(words.reshape(-1), non_blocking=True)
        self._stream = torch.cuda.current_stream(words.device)
        cb = self.crop_border
        self._calls.append((seg, n // 4, int(pred_u8.shape[-3]) - 2 * cb, int(pred_u8.shape[-2]) - 2 * cb))

    def finish(self):
        """Waits for the stream of the last ``add`` and returns ``Scores`` over every frame added; the scorer is empty after."""
        if self._stream is not None:
            self._stream.synchronize()
        out = [[] if w else None for w in self.want]
        for seg, nf, hc, wc in self._calls:
            for dst, vals in zip(out, scores_from_words(seg.view(4, nf), hc, wc, *self.want)):
                if dst is not None:
                    dst.extend(vals)
        self._block, self._used, self._calls, self._stream = None, 0, [], None
        return Scores(*out)


# ---- the command line ------------------------------------------------------------------------------------------------------
def png_key(path):
    """(height, width, colour type) from a PNG's IHDR without decoding it; RefidHipError naming the file when it is no PNG."""
    with open(path, "rb") as f:
        head = f.read(26)
    if len(head) < 26 or head[:8] != b"\x89PNG\r\n\x1a\n" or head[12:16] != b"IHDR":
        raise RefidHipError(f"score: {path} is not a PNG file")
    return int.from_bytes(head[20:24], "big"), int.from_bytes(head[16:20], "big"), head[25]


def pair_files(pred_dir, gt_dir=None, gt_suffix=""):
    """[(name, pred path, gt path)] sorted by name: ``{pred_dir}/X.png`` goes with ``{gt_dir}/X{gt_suffix}.png``.  ``gt_dir``
    defaults to ``pred_dir``, which needs a suffix: files named ``X{gt_suffix}.png`` are then ground truth, the others
    predictions (the validation loop's ``X.png`` / ``X_gt.png`` dumps).  A file without its partner, on either side:
    RefidHipError naming it."""
    gt_dir = pred_dir if gt_dir is None else gt_dir
    same = os.path.abspath(pred_dir) == os.path.abspath(gt_dir)
    if same and not gt_suffix:
        raise RefidHipError("score: --pred and --gt name one directory: give --gt-suffix (e.g. _gt) to tell the files apart")
    for d in (pred_dir, gt_dir):
        if not os.path.isdir(d):
            raise RefidHipError(f"score: {d} is not a directory")
    tail = gt_suffix + ".png"
    stems = lambda d: sorted(f[:-4] for f in os.listdir(d) if f.endswith(".png"))      # noqa: E731
    preds = [s for s in stems(pred_dir) if not (same and s.endswith(gt_suffix))]
    gts = {s[:len(s) - len(gt_suffix)] for s in stems(gt_dir) if s.endswith(gt_suffix) or not gt_suffix}
    if not preds:
        raise RefidHipError(f"score: no prediction *.png under {pred_dir}")
    for s in preds:
        if s not in gts:
            raise RefidHipError(f"score: {os.path.join(pred_dir, s + '.png')} has no ground truth {os.path.join(gt_dir, s + tail)}")
    for s in sorted(gts - set(preds)):
        raise RefidHipError(f"score: {os.path.join(gt_dir, s + tail)} has no prediction {os.path.join(pred_dir, s + '.png')}")
    return [(s + ".png", os.path.join(pred_dir, s + ".png"), os.path.join(gt_dir, s + tail)) for s in preds]


def size_chunks(pairs, per=8):
    """Runs of at most ``per`` consecutive pairs whose files share (H, W, colour type) on both sides: what one
    ``load_png_frames`` call per side and one ``FrameScorer.add`` take.  A pair whose two files differ in (H, W):
    RefidHipError naming the prediction."""
    chunks, last = [], None
    for pair in pairs:
        kp, kg = png_key(pair[1]), png_key(pair[2])
        if kp[:2] != kg[:2]:
            raise RefidHipError(f"score: {pair[1]} is {kp[0]}x{kp[1]}, its ground truth {pair[2]} is {kg[0]}x{kg[1]}")
        if (kp, kg) != last or len(chunks[-1]) >= per:
            chunks.append([])
            last = (kp, kg)
        chunks[-1].append(pair)
    return chunks


def format_lines(names, columns, rows):
    """The report: a ``# file <columns>`` header, one ``name v v ...`` line per frame and a last ``mean`` line: the
    arithmetic mean per column (of the finite values for ``niqe``, whose frames without two usable blocks are nan)."""
    lines = ["# file " + " ".join(columns)]
    for name, row in zip(names, rows):
        lines.append(name + " " + " ".join(f"{v:.6f}" for v in row))
    means = []
    for c, col in zip(columns, zip(*rows)):
        vals = [v for v in col if math.isfinite(v)] if c == "niqe" else list(col)
        means.append(sum(vals) / len(vals) if vals else float("nan"))
    lines.append("mean " + " ".join(f"{v:.6f}" for v in means))
    return lines


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m refid_amd.score", description=__doc__.split("\n\n")[0])
    ap.add_argument("--pred", required=True, help="directory of 8-bit PNG frames to score")
    ap.add_argument("--gt", help="directory of ground-truth PNGs of the same names (default: --pred, with --gt-suffix)")
    ap.add_argument("--gt-suffix", default="", help="ground truth of X.png is X<suffix>.png (the validation dumps: _gt)")
    ap.add_argument("--crop-border", type=int, default=0, help="pixels cut from every side of both frames first")
    ap.add_argument("--y", action="store_true", help="also PSNR / SSIM on the BT.601 Y plane (test_y_channel)")
    ap.add_argument("--niqe", metavar="PARAMS.npz", help="also NIQE of the predictions (niqe_pris_params.npz)")
    ap.add_argument("--out", metavar="FILE", help="write the report there instead of printing it")
    ap.add_argument("--frames-per-launch", type=int, default=8)
    args = ap.parse_args(argv)

    import torch
    from . import niqe as niqe_mod
    from .sequence import load_png_frames
    if args.frames_per_launch < 1:
        raise RefidHipError(f"score: --frames-per-launch {args.frames_per_launch} must be >= 1")
    pairs = pair_files(args.pred, args.gt, args.gt_suffix)
    chunks = size_chunks(pairs, args.frames_per_launch)
    model = niqe_mod.NiqeModel.load(args.niqe) if args.niqe else None
    scorer = FrameScorer(crop_border=args.crop_border, psnr_y=args.y, ssim_y=args.y)
    sums = []                                              # NIQE moment sums per chunk, on the device until the loop is over
    for chunk in chunks:
        pred = load_png_frames([p[1] for p in chunk], frames_per_launch=len(chunk))
        gt = load_png_frames([p[2] for p in chunk], frames_per_launch=len(chunk))
        scorer.add(pred, gt)
        if model is not None:
            sums.append(niqe_mod.moments(pred, model, crop_border=args.crop_border))
    sc = scorer.finish()
    columns = [c for c, v in zip(COLUMNS, sc) if v is not None]
    cols = [v for v in sc if v is not None]
    if model is not None:
        columns.append("niqe")
        cols.append([s for t in sums for s in niqe_mod.finish(t.cpu().numpy(), model)])
    lines = format_lines([p[0] for p in pairs], columns, list(zip(*cols)))
    text = "\n".join(lines) + "\n"
    if args.out:
        parent = os.path.dirname(os.path.abspath(args.out))
        os.makedirs(parent, exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        print(f"{len(pairs)} frames: {lines[-1]} -> {args.out}")
    else:
        sys.stdout.write(text)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
