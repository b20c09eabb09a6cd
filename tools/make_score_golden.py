#!/usr/bin/env python3
"""Generate tests/golden/score.npz: PSNR / SSIM computed by THE REFERENCE's own ``calculate_psnr`` and ``calculate_ssim``
(basicsr/metrics/psnr_ssim.py) with ``crop_border`` and ``test_y_channel``.

Test infrastructure, run once on a CPU where a checkout of the reference is available (its path in REFID_REFERENCE) and
scipy is installed; the fixture is data and is all the tests need.  ``psnr_ssim.py`` is imported unedited.  cv2 and skimage
are not installed, so they are stubs:
  ``cv2.getGaussianKernel(11, 1.5)``  the closed form exp(-(i - 5)^2 / (2 sigma^2)) in float64, divided by its sum
  ``cv2.filter2D(img, -1, window, borderType=BORDER_REPLICATE)``  ``scipy.ndimage.correlate(img, window, mode="nearest")``
  ``skimage.metrics``  empty (the reference imports it and never calls it)
NONE of these stand-ins has been compared with a real cv2: what cv2 rounds differently (its kernel is normalised by a
multiplication with the reciprocal sum, its filter engine adds the taps in an order of its own) is what the 1e-12 bar of
tests/test_score_ref_host.py on the Y-channel SSIM leaves room for.  The 3-D SSIM (``test_y_channel=False``) needs no
reference value: its contract is equality with the project's existing kernel (and the reference's needs a GPU).

Per case the file holds the uint8 BGR frames as the reference takes them (stored, not regenerated) and the reference's
``calculate_psnr`` at the crop, ``calculate_psnr(test_y_channel=True)`` and ``calculate_ssim(test_y_channel=True)`` per frame.
(h, w, crop_border, frames):
  (7, 9, 0, 1)     every tap clamped; the frame is smaller than the halo
  (17, 16, 0, 1)   one tile row of a single line
  (23, 37, 3, 1)   odd crop on an odd pitch: every row segment misaligned; partial tiles both ways
  (40, 50, 4, 3)   frame folding; scored one at a time and reversed for the position-independence check
each in three families of the prediction -- independent noise, gt +- 2, one bit flipped in one green value -- and two
more pairs: identical frames (PSNR inf, SSIM-Y exactly 1) and a flat frame against noise.
``entries`` lists ``name gt_key pred_key crop_border``; ``ref_<name>`` is float64 (frames, 3) = psnr, psnr_y, ssim_y.

The tool prints how far tests/score_ref.py is from the reference: the figures recorded in score_ref.py.
Run:  REFID_REFERENCE=<reference checkout> python tools/make_score_golden.py"""
import importlib
import math
import os
import sys
import types
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFID_REFERENCE")
CASES = ((7, 9, 0, 1), (17, 16, 0, 1), (23, 37, 3, 1), (40, 50, 4, 3))
SEED = 20261


def import_reference():
    if not REF or not os.path.isdir(os.path.join(REF, "basicsr")):
        raise SystemExit("set REFID_REFERENCE to a checkout of the reference (the directory that holds basicsr/)")
    from scipy import ndimage
    sys.dont_write_bytecode = True
    for name in ("basicsr", "basicsr.utils", "basicsr.metrics"):
        mod = types.ModuleType(name)
        mod.__path__ = [os.path.join(REF, *name.split("."))]
        sys.modules[name] = mod
    cv2 = types.ModuleType("cv2")
    cv2.BORDER_REPLICATE = 1

    def get_gaussian_kernel(ksize, sigma):
        assert (ksize, sigma) == (11, 1.5)
        g = [math.exp(-((i - 5) * (i - 5)) / (2.0 * sigma * sigma)) for i in range(ksize)]
        s = 0.0
        for v in g:
            s += v
        return np.array([[v / s] for v in g], dtype=np.float64)

    def filter2d(img, ddepth, kernel, borderType=None):
        assert ddepth == -1 and borderType == cv2.BORDER_REPLICATE and img.dtype == np.float64 and img.ndim == 2
        return ndimage.correlate(img, kernel, mode="nearest")

    cv2.getGaussianKernel, cv2.filter2D = get_gaussian_kernel, filter2d
    sys.modules["cv2"] = cv2
    skimage = types.ModuleType("skimage")
    skimage.metrics = types.ModuleType("skimage.metrics")
    sys.modules["skimage"], sys.modules["skimage.metrics"] = skimage, skimage.metrics
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return importlib.import_module("basicsr.metrics.psnr_ssim")


def make_entries(seed):
    """({key: uint8 (frames, h, w, 3) BGR}, [(name, gt key, pred key, crop_border)]).  The ground truth is a ramp plus
    4-bit noise (it compresses), the noise family full-range."""
    rng = np.random.Generator(np.random.PCG64(seed))
    arrays, entries = {}, []
    for c, (h, w, cb, nf) in enumerate(CASES):
        yy, xx = np.mgrid[0:h, 0:w]
        ramp = (3 * yy + 2 * xx)[None, :, :, None] + np.array([0, 40, 90])[None, None, None, :] + 17 * np.arange(nf)[:, None, None, None]
        gt = ((ramp + rng.integers(0, 16, (nf, h, w, 3))) % 256).astype(np.uint8)
        noise = rng.integers(0, 256, (nf, h, w, 3), dtype=np.uint8)
        pm2 = np.clip(gt.astype(np.int64) + rng.choice([-2, 2], size=gt.shape), 0, 255).astype(np.uint8)
        flip = gt.copy()
        flip[nf - 1, h // 2, w // 2, 1] ^= 8                # inside the crop of every case
        arrays[f"c{c}_gt"], arrays[f"c{c}_noise"], arrays[f"c{c}_pm2"], arrays[f"c{c}_flip"] = gt, noise, pm2, flip
        entries += [(f"c{c}_{fam}", f"c{c}_gt", f"c{c}_{fam}", cb) for fam in ("noise", "pm2", "flip")]
    arrays["flat"] = np.full((1, 23, 37, 3), 128, dtype=np.uint8)
    entries.append(("identical", "c2_gt", "c2_gt", 3))
    entries.append(("flat_vs_noise", "flat", "c2_noise", 3))
    return arrays, entries


def main():
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import score_ref as R
    ref = import_reference()
    arrays, entries = make_entries(SEED)
    out = dict(arrays)
    dev = [0.0, 0.0, 0.0]
    for name, gk, pk, cb in entries:
        rows = []
        for g, p in zip(arrays[gk], arrays[pk]):
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                row = (float(ref.calculate_psnr(p, g, cb)), float(ref.calculate_psnr(p, g, cb, test_y_channel=True)),
                       float(ref.calculate_ssim(p, g, cb, test_y_channel=True)))
            ours = R.scores(R.frame_stages(p, g, bgr=True, crop_border=cb))
            for k in range(3):
                if math.isinf(row[k]) or math.isinf(ours[k]):
                    assert row[k] == ours[k], (name, k, row[k], ours[k])
                else:
                    dev[k] = max(dev[k], abs(row[k] - ours[k]))
            rows.append(row)
        out[f"ref_{name}"] = np.array(rows, dtype=np.float64)
        print(f"{name}: crop {cb}, reference psnr / psnr_y / ssim_y of frame 0: {rows[0][0]:.6f} {rows[0][1]:.6f} {rows[0][2]:.9f}")
    out["entries"] = np.array([" ".join(map(str, e)) for e in entries])
    print(f"restatement against the reference: largest |d psnr| {dev[0]:.3e} dB, |d psnr_y| {dev[1]:.3e} dB, |d ssim_y| {dev[2]:.3e}")
    dst = os.path.join(REPO, "tests", "golden", "score.npz")
    np.savez_compressed(dst, **out)
    print(f"wrote {dst} ({os.path.getsize(dst)} bytes)")


if __name__ == "__main__":
    main()
