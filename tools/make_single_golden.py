#!/usr/bin/env python3
"""Generate tests/golden/single_*.npz: GoProSingleImageEventDataset.__getitem__ (data/Single_image_npy_dataset.py:136-201)
run with THE REFERENCE's own functions.

Test infrastructure in the pattern of tools/make_sample_golden.py, whose reference import (REFID_REFERENCE, the ``np.int``
shim, the ``sys.modules`` stubs and the closed forms standing in for cv2) is used as it is.  Imported from the reference,
unedited: ``events_to_voxel_grid`` and ``voxel_norm`` (data/event_util.py:6-66, 141-160), ``triple_random_crop`` and
``augment`` (data/transforms.py:88-242), ``img2tensor`` (utils/img_util.py:9-33).  Restated here: imfrombytes' ``/ 255.``,
the float32 event rows, and the order of the calls in __getitem__ (:170-187), with ``random.seed(k)`` set before the crop.

Per case: the raw frames (blur, sharp) and events, the config, the seeds, and per seed the reference's PRE-NORM voxel (after
crop and augment), its NORMALISED voxel, lq and gt, and ``d_ref``: the largest distance of the reference's normalised
voxel from the float64 normalisation of its own pre-norm voxel, in units of the tests' bound B (measured against float64,
never against the code under test).

Asserted here, on the CPU: every event lies inside the frame with a non-negative normalised time, and for every element
the reference's ``voxel != 0`` mask equals "the element has contributions and their exact (float64) sum is non-zero" --
zero disagreements.  Run:  REFID_REFERENCE=<reference checkout> python tools/make_single_golden.py"""
import os
import random
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tools"), os.path.join(REPO, "tests")]
import single_assembly_ref as S  # noqa: E402  (float64 helpers and the bound B only)
from make_sample_golden import import_reference, make_events, pick_seeds  # noqa: E402
from refid_amd.data import draw_augmentation  # noqa: E402  (only to CHOOSE seeds and to locate the crop for the assertions)


def getitem(eu, tr, iu, frames_u8, events, bins, gt_size, use_hflip, use_rot, seed):
    img_lq, img_gt = (f.astype(np.float32) / 255. for f in frames_u8)         # img_util.py:147
    h_lq, w_lq, _ = img_lq.shape
    voxel = eu.events_to_voxel_grid(events.copy(), num_bins=bins, width=w_lq, height=h_lq, return_format="HWC")   # :170
    random.seed(seed)
    if gt_size is not None:                                                    # :175-176
        img_gt, img_lq, voxel = tr.triple_random_crop(img_gt, img_lq, voxel, gt_size, 1, "fixture")
    res = iu.img2tensor(tr.augment([img_gt, img_lq, voxel], use_hflip, use_rot))   # :177-185
    gt, lq, pre = res
    normed = eu.voxel_norm(pre)                                                # :187
    return lq.numpy(), pre.numpy().copy(), normed.numpy(), gt.numpy()


ALL = [(h, v, r) for h in (False, True) for v in (False, True) for r in (False, True)]
CASES = [
    # name, bins, (H, W), gt_size, (t0, t1), combos wanted, corner crop wanted, first seed tried
    ("single_bins6", 6, (48, 64), 32, (1.6e9, 1.6e9 + 2.0e5), ALL, True, 0),
    ("single_bins2", 2, (40, 56), 24, (3.0, 3.25), [(True, False, True), (False, True, False)], False, 400),
]


def main():
    out_dir = os.path.join(REPO, "tests", "golden")
    eu, tr, iu = import_reference()
    for ci, (name, bins, (H, W), gt_size, (t0, t1), combos, corner, start) in enumerate(CASES):
        rng = np.random.Generator(np.random.PCG64(2000 + ci))
        seeds = pick_seeds(H, W, gt_size, True, True, combos, corner, start)
        hot = []
        for k in seeds:
            top, left, hf, vf, rt = draw_augmentation(random.Random(k), H, W, gt_size, True, True)
            hot.append((top + gt_size // 2, left + gt_size // 3 + len(hot) % 8))
        frames = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
        events = make_events(rng, H, W, t0, t1, 2500, hot[:3], 400)
        ts = (np.float32(bins - 1) * (events[:, 0] - events[0, 0])) / np.float32(events[-1, 0] - events[0, 0])
        assert np.all(ts >= 0) and np.all((events[:, 1] >= 0) & (events[:, 1] < W) & (events[:, 2] >= 0) & (events[:, 2] < H))
        rec = {"frames": frames, "events": events, "seeds": np.array(seeds),
               "config": np.array([bins, gt_size, 1, 1])}
        d_all = []
        for k in seeds:
            lq, pre, normed, gt = getitem(eu, tr, iu, list(frames), events, bins, gt_size, True, True, k)
            top, left, hf, vf, rt = draw_augmentation(random.Random(k), H, W, gt_size, True, True)
            e, cnt, mass = S.float64_sums(events, bins, H, W, top, left, gt_size, gt_size, hf, vf, rt)
            disagree = int(np.count_nonzero((pre != 0) != ((cnt > 0) & (e != 0))))
            assert disagree == 0, (name, k, disagree)
            x64, mu, sigma = S.float64_norm(pre)
            b = S.bound(pre, mu, sigma, pre.size)
            nz = pre != 0
            d_ref = float((np.abs(normed.astype(np.float64) - x64)[nz] / b[nz]).max())
            assert np.all(normed[~nz] == 0)
            d_all.append(d_ref)
            rec[f"s{k}/lq"], rec[f"s{k}/pre"], rec[f"s{k}/voxel"], rec[f"s{k}/gt"] = lq, pre, normed, gt
            rec[f"s{k}/d_ref"] = np.float64(d_ref)
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **rec)
        print(f"{name}: seeds {seeds}, {len(events)} events, voxel {pre.shape}, non-zero {int(nz.sum())}, "
              f"d_ref max {max(d_all):.2f}, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
