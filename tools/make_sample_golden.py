#!/usr/bin/env python3
"""Generate tests/golden/sample_*.npz: the recurrent datasets' __getitem__ run with THE REFERENCE's own functions.

Test infrastructure, run once on a CPU where a checkout of the reference is available (its path in REFID_REFERENCE);
the fixtures are data and are all the tests need.  Imported from the reference, unedited:
``events_to_voxel_grid`` (data/event_util.py:6-66), ``triple_random_crop`` and ``augment`` (data/transforms.py:88-242) and
``img2tensor`` (utils/img_util.py:9-33), with the ``np.int`` alias shim and the ``sys.modules`` stubs that
oracle/make_golden.py uses.  cv2 is not installed: ``cv2.flip(img, 1)`` / ``cv2.flip(img, 0)`` are stood in for by their
closed forms, reversal of the column / row axis, and ``cv2.cvtColor(img, COLOR_BGR2RGB)`` by reversal of the channel axis.

Only the glue between those calls is restated here: imfrombytes' ``astype(float32) / 255.`` (img_util.py:147), the
float32 event rows (image_npy_dataset.py:155-163), and the stacking / slicing of image_npy_dataset.py:188-232
(blur layout, return_deblur_voxel) and image_sharp_npy_dataset.py:180-225 (sharp layout), with ``random.seed(k)`` set
before the crop so that refid_amd.data.draw_augmentation(random.Random(k), ...) must reproduce the draws.

Every event lies inside the frame and has a non-negative normalised time, so the reference's flat index neither wraps
nor spills.  Stored per case: the inputs, the seeds, per seed the outputs lq / voxel / gt, and the un-augmented
full-frame voxel.  Run:  REFID_REFERENCE=<reference checkout> python tools/make_sample_golden.py"""
import importlib
import os
import random
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFID_REFERENCE")
sys.path.insert(0, REPO)
from refid_amd.data import draw_augmentation  # noqa: E402  (only to CHOOSE seeds; the fixtures come from the reference)


def import_reference():
    if not REF or not os.path.isdir(os.path.join(REF, "basicsr")):
        raise SystemExit("set REFID_REFERENCE to a checkout of the reference (the directory that holds basicsr/)")
    sys.dont_write_bytecode = True
    if not hasattr(np, "int"):
        np.int = int                                   # event_util.py:39,44 use the removed alias

    def pkg(name, path):
        mod = types.ModuleType(name)
        mod.__path__ = [path]
        sys.modules[name] = mod
        return mod

    pkg("basicsr", f"{REF}/basicsr")
    pkg("basicsr.data", f"{REF}/basicsr/data")
    utils = pkg("basicsr.utils", f"{REF}/basicsr/utils")
    utils.Timer = utils.CudaTimer = object
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_BGR2RGB = 4

    def flip(img, code):
        assert code in (0, 1)
        return np.ascontiguousarray(img[:, ::-1] if code == 1 else img[::-1])

    def cvt_color(img, code):
        assert code == cv2.COLOR_BGR2RGB and img.shape[2] == 3
        return np.ascontiguousarray(img[:, :, ::-1])

    cv2.flip, cv2.cvtColor = flip, cvt_color
    sys.modules["cv2"] = cv2
    tv, tvu = types.ModuleType("torchvision"), types.ModuleType("torchvision.utils")
    tvu.make_grid = None
    tv.utils = tvu
    sys.modules["torchvision"], sys.modules["torchvision.utils"] = tv, tvu
    eu = importlib.import_module("basicsr.data.event_util")
    tr = importlib.import_module("basicsr.data.transforms")
    iu = importlib.import_module("basicsr.utils.img_util")
    return eu, tr, iu


def getitem(eu, tr, iu, frames_u8, events, m, n, layout, gt_size, use_hflip, use_rot, seed):
    bins = 2 * m + n + 1 if layout == "blur" else n + 1
    imgs = [f.astype(np.float32) / 255. for f in frames_u8]                    # img_util.py:147
    img_lqs, img_gts = imgs[:2], imgs[2:]
    h_lq, w_lq, _ = img_lqs[0].shape
    voxel = eu.events_to_voxel_grid(events.copy(), num_bins=bins, width=w_lq, height=h_lq, return_format="HWC")
    full = np.ascontiguousarray(voxel.transpose(2, 0, 1))
    voxels = [voxel]
    random.seed(seed)
    if gt_size is not None:                                                    # image_npy_dataset.py:188-189
        img_gts, img_lqs, voxels = tr.triple_random_crop(img_gts, img_lqs, voxels, gt_size, 1, "fixture")
    num_lq, num_gt = len(img_lqs), len(img_gts)                                # :192-204
    img_lqs.extend(img_gts)
    img_lqs.extend(voxels) if isinstance(voxels, list) else img_lqs.append(voxels)
    res = iu.img2tensor(tr.augment(img_lqs, use_hflip, use_rot))
    lqs = torch.stack(res[:num_lq], dim=0)
    gts = torch.stack(res[num_lq:num_lq + num_gt], dim=0)
    voxels_list = res[num_lq + num_gt:]
    if layout == "blur":                                                       # :211-221
        lqs = torch.cat((lqs[0], voxels_list[0][1:m], lqs[1], voxels_list[0][m + 2 + n:]), dim=0)
    v = torch.stack(voxels_list, dim=0).squeeze(0)                             # :223-232
    v = torch.stack([v[i:i + 2] for i in range(v.shape[0] - 1)], dim=0)
    return lqs.numpy(), v.numpy(), gts.numpy(), full


def pick_seeds(H, W, gt_size, use_hflip, use_rot, want_combos, want_corner, start):
    """Smallest seeds from `start` on that realise each wanted (hflip, vflip, rot90) and, if asked, a corner crop."""
    seeds, left, corner = [], set(want_combos), want_corner
    k = start
    while left or corner:
        top, lft, hf, vf, rt = draw_augmentation(random.Random(k), H, W, gt_size, use_hflip, use_rot)
        at_corner = gt_size is not None and top in (0, H - gt_size) and lft in (0, W - gt_size)
        if (hf, vf, rt) in left or (corner and at_corner):
            seeds.append(k)
            left.discard((hf, vf, rt))
            corner = corner and not at_corner
        k += 1
    return seeds


def make_events(rng, H, W, t0, t1, n_background, hot_pixels, n_hot):
    """float32 rows [t, x, y, p] sorted by time; `n_hot` events on each hot pixel, half of them inside 4 % of the span."""
    t, x, y = [rng.uniform(t0, t1, n_background)], [rng.integers(0, W, n_background)], [rng.integers(0, H, n_background)]
    for (hy, hx) in hot_pixels:
        a = rng.uniform(t0 + 0.40 * (t1 - t0), t0 + 0.44 * (t1 - t0), n_hot // 2)
        t += [a, rng.uniform(t0, t1, n_hot - n_hot // 2)]
        x.append(np.full(n_hot, hx))
        y.append(np.full(n_hot, hy))
    edge = 40                                                                  # last row / last column of the frame
    t.append(rng.uniform(t0, t1, 2 * edge))
    x += [np.full(edge, W - 1), rng.integers(0, W, edge)]
    y += [rng.integers(0, H, edge), np.full(edge, H - 1)]
    t, x, y = np.concatenate(t), np.concatenate(x), np.concatenate(y)
    p = rng.integers(0, 2, t.size)
    p[x == hot_pixels[0][1]] = np.where(rng.random(int((x == hot_pixels[0][1]).sum())) < 0.9, 1, 0)   # a net-positive column
    ev = np.stack([t, x, y, p], axis=1).astype(np.float32)                     # image_npy_dataset.py:155-163
    return np.ascontiguousarray(ev[np.argsort(ev[:, 0], kind="stable")])


CASES = [
    # name, layout, m, n, (H, W), gt_size, use_hflip, use_rot, (t0, t1), combos wanted, corner crop wanted, first seed tried
    ("sample_blur_m3", "blur", 3, 1, (40, 56), 16, True, True, (1.6e9, 1.6e9 + 2.0e5),       # microseconds: coarse fp32 ts
     [(False, False, False), (True, False, True), (False, True, True)], True, 0),
    ("sample_blur_m11", "blur", 11, 1, (24, 32), 16, True, True, (0.0, 0.5),                   # fine fp32 ts
     [(True, True, True), (False, True, False), (True, False, False)], False, 100),
    ("sample_sharp_n7", "sharp", 1, 7, (24, 32), 16, True, True, (10.0, 10.3),
     [(True, True, False), (False, False, True)], False, 200),
    ("sample_whole_frame", "blur", 3, 1, (24, 40), None, True, False, (2.0, 2.05),
     [(True, False, False)], False, 300),
]


def main():
    out_dir = os.path.join(REPO, "tests", "golden")
    eu, tr, iu = import_reference()
    seen = set()
    for ci, (name, layout, m, n, (H, W), gt_size, use_hflip, use_rot, (t0, t1), combos, corner, start) in enumerate(CASES):
        rng = np.random.Generator(np.random.PCG64(1000 + ci))
        bins = 2 * m + n + 1 if layout == "blur" else n + 1
        seeds = pick_seeds(H, W, gt_size, use_hflip, use_rot, combos, corner, start)
        hot = []
        for k in seeds:                                                        # one hot pixel at the centre of every crop
            top, left, hf, vf, rt = draw_augmentation(random.Random(k), H, W, gt_size, use_hflip, use_rot)
            seen.add((hf, vf, rt))
            ps = (H, W) if gt_size is None else (gt_size, gt_size)
            hot.append((top + ps[0] // 2, left + ps[1] // 3 + len(hot)))
        frames = rng.integers(0, 256, (bins + 1, H, W, 3), dtype=np.uint8)     # blur0, blur1, gt0: all 256 levels
        for f in range(3, bins + 1):                                           # later frames: four levels each (small files)
            frames[f] = rng.integers(0, 256, 4, dtype=np.uint8)[rng.integers(0, 4, (H, W, 3))]
        events = make_events(rng, H, W, t0, t1, 2000, hot, 2200)
        rec = {"frames": frames, "events": events, "seeds": np.array(seeds), "layout": np.array(layout),
               "config": np.array([m, n, -1 if gt_size is None else gt_size, int(use_hflip), int(use_rot)]),
               "hot_pixels": np.array(hot)}
        for k in seeds:
            lq, vox, gt, full = getitem(eu, tr, iu, list(frames), events, m, n, layout, gt_size, use_hflip, use_rot, k)
            rec[f"s{k}/lq"], rec[f"s{k}/voxel"], rec[f"s{k}/gt"] = lq, vox, gt
        rec["voxel_full"] = full
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **rec)
        print(f"{name}: seeds {seeds}, {len(events)} events, lq {lq.shape} voxel {vox.shape} gt {gt.shape}, "
              f"{os.path.getsize(path) / 1024:.0f} KiB")
    assert len(seen) == 8, f"flip / flip / transpose combinations covered: {sorted(seen)}"


if __name__ == "__main__":
    main()
