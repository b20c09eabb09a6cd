#!/usr/bin/env python3
"""Generate tests/golden/val_tail.npz: the validation tail computed by THE REFERENCE's own functions.

Test infrastructure, run once on a CPU where a checkout of the reference is available (its path in REFID_REFERENCE);
the fixture is data and is all the tests need.  Imported from the reference, unedited: ``tensor2img``
(utils/img_util.py:59-121), ``calculate_psnr`` and ``calculate_ssim`` (metrics/psnr_ssim.py:9-63, :225-303 -> _ssim_3d
:135-182).  cv2, skimage and torchvision.utils are not installed and there is no GPU, so, as oracle/make_golden.py's
run_metrics does: cv2 is a stub holding ``getGaussianKernel`` (OpenCV's closed form for ksize > 7, sigma > 0) and
``cvtColor(RGB2BGR)`` (channel reversal), and ``.cuda()`` is the identity for the duration of the calls.

Per case `(n_frames, H, W)` the file holds the fp32 ``pred`` / ``gt`` (n_frames, 3, H, W), the reference's uint8 BGR images
and the per-frame PSNR / SSIM.  The inputs: uniform in [-0.2, 1.2] (on a coarse grid of float32 values, and from 64 levels of it in the later frames and in
the largest case, so that the file compresses); in frame 0 every tie (k + 0.5)/255, k = 0..254, and exact 0, -0.0, 1, 1 + 2^-23 where the frame has room;
gt = an independent draw (frame 0), pred + a few grey levels of noise (later frames), pred itself (last frame of a
case with three or more frames: PSNR inf, SSIM 1).  Every pred frame holds a value above 1/255, so the reference's
``max_value = 1 if img.max() <= 1 else 255`` takes its 255 branch, the only one the kernels implement.

For one run of 3 items over 2 sequences at m=1, n=3 (T=5: the five frames of case (5,16,16), rotated per item) it also
holds the aggregated deblur / interpolation / total values, formed from the per-frame numbers by the formulas of
twoImage_event_recurrent_model.py:499-521.  Run:  REFID_REFERENCE=<reference checkout> python tools/make_val_golden.py"""
import importlib
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFID_REFERENCE")

CASES = [(1, 1, 1), (3, 17, 35), (5, 16, 16), (2, 40, 56)]
BOOK_M, BOOK_N = 1, 3


def import_reference():
    if not REF or not os.path.isdir(os.path.join(REF, "basicsr")):
        raise SystemExit("set REFID_REFERENCE to a checkout of the reference (the directory that holds basicsr/)")
    sys.dont_write_bytecode = True

    def pkg(name, path):
        mod = types.ModuleType(name)
        mod.__path__ = [path]
        sys.modules[name] = mod
        return mod

    pkg("basicsr", f"{REF}/basicsr")
    pkg("basicsr.utils", f"{REF}/basicsr/utils")
    pkg("basicsr.metrics", f"{REF}/basicsr/metrics")
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_RGB2BGR = 4

    def get_gaussian_kernel(ksize, sigma):
        assert ksize > 7 and sigma > 0                # below that OpenCV switches to fixed tables / derived sigma
        x = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2.0
        k = np.exp(-(x * x) / (2.0 * sigma * sigma))
        return (k / k.sum()).reshape(ksize, 1)

    def cvt_color(img, code):
        assert code == cv2.COLOR_RGB2BGR and img.shape[2] == 3
        return np.ascontiguousarray(img[:, :, ::-1])

    cv2.getGaussianKernel, cv2.cvtColor = get_gaussian_kernel, cvt_color
    sys.modules["cv2"] = cv2
    for nm in ("skimage", "skimage.metrics"):
        sys.modules.setdefault(nm, types.ModuleType(nm))
    sys.modules["skimage"].metrics = sys.modules["skimage.metrics"]
    tv, tvu = types.ModuleType("torchvision"), types.ModuleType("torchvision.utils")
    tvu.make_grid = None                              # only reached for 4-D mini-batches
    tv.utils = tvu
    sys.modules["torchvision"], sys.modules["torchvision.utils"] = tv, tvu
    iu = importlib.import_module("basicsr.utils.img_util")
    ps = importlib.import_module("basicsr.metrics.psnr_ssim")
    return iu, ps


def coarse(x):
    """float32 values with the low 16 mantissa bits cleared."""
    return (np.asarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def make_inputs(rng, nf, h, w):
    pred = coarse(rng.uniform(-0.2, 1.2, (nf, 3, h, w)))
    levels = coarse(rng.uniform(-0.2, 1.2, 64))       # later frames (and the largest case): 64 levels each, a small file
    first = 0 if h * w > 1024 else 1
    pred[first:] = levels[rng.integers(0, 64, pred[first:].shape)]
    special = np.concatenate([(np.arange(255, dtype=np.float64) + 0.5) / 255,
                              [0.0, -0.0, 1.0, 1.0 + 2.0 ** -23]]).astype(np.float32)
    flat = pred[0].reshape(-1)
    if flat.size >= special.size:
        flat[:special.size] = special
    else:                                             # (1,1,1): a tie, a value below 0 and one above 1
        flat[:] = np.array([2.5 / 255, -0.1, 1.2], dtype=np.float32)[:flat.size]
    pred[:, 0, 0, 0] = np.maximum(pred[:, 0, 0, 0], np.float32(2.5 / 255))     # max_value == 255 in every frame
    gt = np.empty_like(pred)
    gt[0] = coarse(rng.uniform(-0.2, 1.2, (3, h, w))) if first else levels[rng.integers(0, 64, (3, h, w))]
    if flat.size >= special.size:
        gt[0].reshape(-1)[:special.size] = np.roll(special, 7)
    for f in range(1, nf):
        gt[f] = (pred[f] + rng.integers(-6, 7, (3, h, w)).astype(np.float32) / np.float32(255)).astype(np.float32)
    if nf > 2:
        gt[nf - 1] = pred[nf - 1]
    return pred, gt


def bookkeeping(psnr, ssim):
    """3 items (sequences A, A, B) of T = 2m+n = 5 frames; item k uses the case's frames rotated by k."""
    m, n = BOOK_M, BOOK_N
    t = 2 * m + n
    items = [np.roll(np.arange(t), k) for k in range(3)]
    deblur, interpo = {"psnr": 0, "ssim": 0}, {"psnr": 0, "ssim": 0}
    cnt = 0
    for order in items:
        for idx, f in enumerate(order):
            dst = interpo if m <= idx < m + n else deblur
            dst["psnr"] += float(psnr[f])
            dst["ssim"] += float(ssim[f])
        cnt += 1
    total = {}
    for k in deblur:                                  # :499-521
        deblur[k] /= (cnt * 2 * m)
    for k in interpo:
        interpo[k] /= (cnt * n)
    for k in deblur:
        total[k] = deblur[k] * 2 * m + interpo[k] * n
        total[k] /= 2 * m + n
    return np.array(items), deblur, interpo, total


def main():
    iu, ps = import_reference()
    rec = {"cases": np.array(CASES)}
    saved = (torch.Tensor.cuda, torch.nn.Module.cuda)
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    try:
        for ci, (nf, h, w) in enumerate(CASES):
            rng = np.random.Generator(np.random.PCG64(2000 + ci))
            pred, gt = make_inputs(rng, nf, h, w)
            key = f"{nf}x{h}x{w}"
            pu8, gu8, psnr, ssim = [], [], [], []
            for f in range(nf):
                sr_img = iu.tensor2img([torch.from_numpy(pred[f].copy())])      # the call of :429 (uint8, BGR)
                gt_img = iu.tensor2img([torch.from_numpy(gt[f].copy())])        # :432
                sr_img, gt_img = sr_img.reshape(h, w, 3), gt_img.reshape(h, w, 3)
                assert sr_img.max() > 1
                pu8.append(sr_img)
                gu8.append(gt_img)
                psnr.append(ps.calculate_psnr(sr_img, gt_img, crop_border=0))
                ssim.append(ps.calculate_ssim(sr_img, gt_img, crop_border=0))
            rec[f"{key}/pred"], rec[f"{key}/gt"] = pred, gt
            rec[f"{key}/pred_u8_bgr"], rec[f"{key}/gt_u8_bgr"] = np.stack(pu8), np.stack(gu8)
            rec[f"{key}/psnr"], rec[f"{key}/ssim"] = np.array(psnr, dtype=np.float64), np.array(ssim, dtype=np.float64)
            print(key, "psnr", np.round(psnr, 3), "ssim", np.round(ssim, 5))
    finally:
        torch.Tensor.cuda, torch.nn.Module.cuda = saved
    items, deblur, interpo, total = bookkeeping(rec["5x16x16/psnr"][[0, 1, 2, 3, 1]], rec["5x16x16/ssim"][[0, 1, 2, 3, 1]])
    rec["book/frames"] = np.array([0, 1, 2, 3, 1])[items]            # which frame of case 5x16x16 each item's frame is
    rec["book/seq"] = np.array(["A", "A", "B"])
    rec["book/mn"] = np.array([BOOK_M, BOOK_N])
    for nm, d in (("deblur", deblur), ("interpo", interpo), ("total", total)):
        rec[f"book/{nm}"] = np.array([d["psnr"], d["ssim"]], dtype=np.float64)
    path = os.path.join(REPO, "tests", "golden", "val_tail.npz")
    np.savez_compressed(path, **rec)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
