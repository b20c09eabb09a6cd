#!/usr/bin/env python3
"""Generate tests/golden/niqe.npz: NIQE computed by THE REFERENCE's own ``calculate_niqe`` (basicsr/metrics/niqe.py).

Test infrastructure, run once on a CPU where a checkout of the reference is available (its path in REFID_REFERENCE) and
scipy is installed; the fixture is data and is all the tests need.  ``niqe.py`` is imported unedited.  cv2 is not installed,
so it is a stub whose ``resize`` is NIQE's one call of it: ``resize(img / 255., (w // 2, h // 2), INTER_LINEAR)`` on an image
whose sides are multiples of 96.  At an exact factor 2 bilinear resampling is a 2x2 mean, taken here in float32,
horizontal pair first, each ``a * 0.5 + b * 0.5``.  This stand-in has NOT been compared with a real cv2.  The reference
reads ``basicsr/metrics/niqe_pris_params.npz`` relative to the working directory, so the tool changes into the checkout
for the calls; the parameter file itself goes to tests/golden/niqe_pris_params.npz.

Per frame the file holds the uint8 BGR input (stored, not regenerated: FFT rounding may differ between machines), the
two per-scale feature matrices (blocks, 18) captured by wrapping ``compute_feature``, and the score:
  f0  192x192  1/f texture
  f1  200x301  1/f texture: the crop, an odd width, 6 blocks
  f2  192x288  1/f texture with one block of constant 255 (the map is exactly zero inside it and positive within three pixels
               of its neighbours: a one-sided map, NaN features, a row that the score leaves out) and one block clipped to
               <= 40 (large areas of exact zeros, which count on neither side)
  f3  192x192  white noise: a wrong in-block wrap of the neighbour products shows here

The tool prints how far tests/niqe_ref.py is from the reference (alphas that differ, largest feature and score deviation:
the figures behind the bars in niqe_ref.py) and refuses to write a fixture on which an alpha differs: then it tries the
next seed.  Run:  REFID_REFERENCE=<reference checkout> python tools/make_niqe_golden.py"""
import importlib
import os
import shutil
import sys
import types
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFID_REFERENCE")
ALPHA_COLS = (0, 2, 6, 10, 14)


def import_reference():
    if not REF or not os.path.isdir(os.path.join(REF, "basicsr")):
        raise SystemExit("set REFID_REFERENCE to a checkout of the reference (the directory that holds basicsr/)")
    sys.dont_write_bytecode = True
    for name in ("basicsr", "basicsr.utils", "basicsr.metrics"):
        mod = types.ModuleType(name)
        mod.__path__ = [os.path.join(REF, *name.split("."))]
        sys.modules[name] = mod
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR = 1

    def resize(img, dsize, interpolation=None):
        h, w = img.shape
        assert interpolation == cv2.INTER_LINEAR and dsize == (w // 2, h // 2) and h % 2 == 0 and w % 2 == 0
        assert img.dtype == np.float32
        hz = img[:, 0::2] * np.float32(0.5) + img[:, 1::2] * np.float32(0.5)
        return hz[0::2] * np.float32(0.5) + hz[1::2] * np.float32(0.5)

    cv2.resize = resize
    sys.modules["cv2"] = cv2
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return importlib.import_module("basicsr.metrics.niqe")


def texture(rng, h, w):
    """1/f noise per channel, stretched to [0, 255]."""
    fy, fx = np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :]
    amp = 1.0 / np.maximum(np.sqrt(fy * fy + fx * fx), 1.0 / max(h, w))
    out = np.empty((h, w, 3))
    for c in range(3):
        t = np.real(np.fft.ifft2(np.fft.fft2(rng.standard_normal((h, w))) * amp))
        out[..., c] = (t - t.min()) / (t.max() - t.min())
    return np.round(out * 255.0).astype(np.uint8)


def make_frames(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    f0 = texture(rng, 192, 192)
    f1 = texture(rng, 200, 301)
    f2 = texture(rng, 192, 288)
    f2[0:96, 96:192] = 255
    f2[96:192, 192:288] = np.minimum(f2[96:192, 192:288], 40)
    f3 = rng.integers(0, 256, (192, 192, 3), dtype=np.uint8)
    return [f0, f1, f2, f3]


def reference_run(niqe_mod, frame):
    """(score, [features scale 1, features scale 2]) of calculate_niqe on one uint8 BGR frame."""
    rows = []
    inner = niqe_mod.compute_feature

    def capture(block):
        feat = inner(block)
        rows.append([float(v) for v in feat])
        return feat

    niqe_mod.compute_feature = capture
    cwd = os.getcwd()
    try:
        os.chdir(REF)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            score = float(niqe_mod.calculate_niqe(frame, 0, input_order="HWC", convert_to="y"))
    finally:
        os.chdir(cwd)
        niqe_mod.compute_feature = inner
    rows = np.array(rows, dtype=np.float64)
    half = rows.shape[0] // 2
    return score, [rows[:half], rows[half:]]


def main():
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import niqe_ref as R
    niqe_mod = import_reference()
    params = dict(np.load(os.path.join(REF, "basicsr", "metrics", "niqe_pris_params.npz")))
    for seed in range(20260, 20270):
        frames = make_frames(seed)
        out, n_alpha, bad_alpha, bad_nan, feat_dev, score_dev = {}, 0, 0, 0, 0.0, 0.0
        for k, frame in enumerate(frames):
            score, feats = reference_run(niqe_mod, frame)
            ours_score, ours = R.niqe_ref(frame, params, bgr=True)
            ref = np.concatenate(feats, axis=1)
            cols = [c + 18 * s for s in (0, 1) for c in ALPHA_COLS]
            bad_nan += int((np.isnan(ref) != np.isnan(ours)).sum())
            n_alpha += ref[:, cols].size
            bad_alpha += int((ref[:, cols] != ours[:, cols]).sum())
            with np.errstate(invalid="ignore"):
                feat_dev = max(feat_dev, float(np.nanmax(np.abs(ours - ref) / (np.abs(ref) + 1e-3))))
            score_dev = max(score_dev, abs(ours_score - score))
            out[f"f{k}_bgr"], out[f"f{k}_feat1"], out[f"f{k}_feat2"], out[f"f{k}_score"] = frame, feats[0], feats[1], score
            print(f"seed {seed} f{k} {frame.shape[0]}x{frame.shape[1]}: reference {score:.6f}, restatement {ours_score:.6f}, "
                  f"NaN rows {int(np.isnan(ref).any(axis=1).sum())} of {ref.shape[0]}")
        print(f"seed {seed}: {bad_alpha} of {n_alpha} alphas differ, {bad_nan} NaN mismatches, largest feature deviation "
              f"{feat_dev:.3e} relative to |ref| + 1e-3, largest score deviation {score_dev:.3e}")
        if bad_alpha == 0 and bad_nan == 0:
            break
        print(f"seed {seed} refused: the restatement and the reference differ on an alpha or a NaN; next seed")
    else:
        raise SystemExit("no seed gave a fixture on which every alpha agrees")
    out["n_frames"] = np.int64(len(frames))
    dst = os.path.join(REPO, "tests", "golden")
    np.savez_compressed(os.path.join(dst, "niqe.npz"), **out)
    shutil.copyfile(os.path.join(REF, "basicsr", "metrics", "niqe_pris_params.npz"), os.path.join(dst, "niqe_pris_params.npz"))
    print(f"wrote {dst}/niqe.npz ({os.path.getsize(os.path.join(dst, 'niqe.npz'))} bytes) and niqe_pris_params.npz")


if __name__ == "__main__":
    main()
