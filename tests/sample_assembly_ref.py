"""numpy restatement of the batch-assembly kernels (refid_amd/csrc/sample.hip), shared by test_sample_assembly_host.py
and test_hip_sample_assembly.py: the fp32 time normalisation of the reference (data/event_util.py:37 on float32 rows), the
64-bit fixed-point accumulation (32 fractional bits), the one-rounding conversion, the crop / flip / flip / transpose of
transforms.py:114-129, BGR -> RGB with a true /255, and the lq / voxel / gt layouts of image_npy_dataset.py:211-232 and
image_sharp_npy_dataset.py:194-225.  Everything is integer arithmetic or a single correctly rounded fp32 operation, so
the device must reproduce it bit for bit."""
import os

import numpy as np

ONE = np.int64(1) << np.int64(32)
FIXTURES = ("sample_blur_m3", "sample_blur_m11", "sample_sharp_n7", "sample_whole_frame")


def num_bins(m, n, layout):
    return 2 * m + n + 1 if layout == "blur" else n + 1


def load_fixture(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    m, n, gt_size, use_hflip, use_rot = (int(v) for v in z["config"])
    cfg = dict(m=m, n=n, layout=str(z["layout"]), gt_size=None if gt_size < 0 else gt_size, use_hflip=bool(use_hflip),
               use_rot=bool(use_rot), seeds=[int(s) for s in z["seeds"]])
    return z, cfg


def event_terms(events, first, last, bins, height, width, top, left, ch, cw, hflip, vflip, rot90):
    """Per-event quantities of the scatter kernel: keep (bool), ti, flat output index, q, sign.  `events` is (N,4) float32."""
    ev = np.asarray(events, dtype=np.float32).reshape(-1, 4)
    first, last = np.float32(first), np.float32(last)
    dT = np.float32(last - first)
    if dT == 0:
        dT = np.float32(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        ts = (np.float32(bins - 1) * (ev[:, 0] - first)) / dT                 # three fp32 roundings, this order
        assert ts.dtype == np.float32
        keep = (ts >= 0) & (ts < np.float32(bins))
        keep &= (ev[:, 1] > -1) & (ev[:, 1] < np.float32(width)) & (ev[:, 2] > -1) & (ev[:, 2] < np.float32(height))
        ts = np.where(keep, ts, np.float32(0))
        x = np.where(keep, ev[:, 1], np.float32(0)).astype(np.int64)          # truncation
        y = np.where(keep, ev[:, 2], np.float32(0)).astype(np.int64)
    cy, cx = y - top, x - left
    keep &= (cy >= 0) & (cy < ch) & (cx >= 0) & (cx < cw)
    ti = ts.astype(np.int64)
    dts = ts - ti.astype(np.float32)                                          # exact
    assert dts.dtype == np.float32
    q = (dts * np.float32(4294967296.0)).astype(np.int64)                     # exact product, truncated
    if hflip:
        cx = cw - 1 - cx
    if vflip:
        cy = ch - 1 - cy
    ow = ch if rot90 else cw
    idx = cx * ow + cy if rot90 else cy * ow + cx
    sign = np.where(ev[:, 3] > 0, 1, -1).astype(np.int64)
    return keep, ti, idx, q, sign


def accumulate(events, first, last, bins, height, width, top, left, ch, cw, hflip, vflip, rot90):
    """int64 [bins, oh, ow] fixed-point sums."""
    assert not rot90 or ch == cw
    keep, ti, idx, q, sign = event_terms(events, first, last, bins, height, width, top, left, ch, cw, hflip, vflip, rot90)
    acc = np.zeros((bins, ch * cw), dtype=np.int64)
    np.add.at(acc, (ti[keep], idx[keep]), (sign * (ONE - q))[keep])
    right = keep & (ti + 1 < bins)
    np.add.at(acc, (ti[right] + 1, idx[right]), (sign * q)[right])
    return acc.reshape(bins, ch, cw)


def fixed_to_float(acc):
    """int64 -> fp32 with one rounding (RNE), then the exact scaling by 2^-32."""
    return acc.astype(np.float32) * np.float32(2.0 ** -32)


def frames_to_chw(frames, y0, x0, top, left, ch, cw, hflip, vflip, rot90):
    """(F, Hwin, Wwin, 3) u8 BGR -> (F, 3, oh, ow) float32 RGB in [0, 1]."""
    f = np.asarray(frames)[:, top - y0:top - y0 + ch, left - x0:left - x0 + cw, :]
    if hflip:
        f = f[:, :, ::-1]
    if vflip:
        f = f[:, ::-1]
    if rot90:
        f = f.transpose(0, 2, 1, 3)
    f = f[..., ::-1].astype(np.float32) / np.float32(255.0)                   # one correctly rounded division
    return np.ascontiguousarray(f.transpose(0, 3, 1, 2))


def assemble_sample(sample, m, n, layout, gt_size):
    """One raw sample (the DeviceBatchAssembler contract, numpy arrays) -> (lq, voxel, gt) float32."""
    bins = num_bins(m, n, layout)
    ev = np.asarray(sample["events"], dtype=np.float32).reshape(-1, 4)
    fr = np.asarray(sample["frames"])
    y0, x0 = sample.get("origin", (0, 0))
    H, W = sample.get("frame_hw", (y0 + fr.shape[1], x0 + fr.shape[2]))
    ch, cw = (H, W) if gt_size is None else (gt_size, gt_size)
    first, last = sample.get("first_stamp"), sample.get("last_stamp")
    if first is None or last is None:
        first, last = (ev[0, 0], ev[-1, 0]) if len(ev) else (0.0, 0.0)
    aug = [sample.get(k, 0) for k in ("top", "left", "hflip", "vflip", "rot90")]
    vox = fixed_to_float(accumulate(ev, first, last, bins, H, W, aug[0], aug[1], ch, cw, *aug[2:]))
    img = frames_to_chw(fr, y0, x0, aug[0], aug[1], ch, cw, *aug[2:])
    voxel = np.stack([vox[:-1], vox[1:]], axis=1)                              # (bins-1, 2, h, w)
    gt = img[2:]
    if layout == "blur":
        lq = np.concatenate([img[0], vox[1:m], img[1], vox[m + 2 + n:]], axis=0)
    else:
        lq = img[:2]
    return np.ascontiguousarray(lq), np.ascontiguousarray(voxel), np.ascontiguousarray(gt)


def assemble_batch(samples, m, n, layout, gt_size):
    outs = [assemble_sample(s, m, n, layout, gt_size) for s in samples]
    return tuple(np.stack([o[k] for o in outs]) for k in range(3))


def image_channels(lq, m, layout):
    """The channels of one sample's lq that hold image data (the rest are voxel bins)."""
    if layout == "sharp":
        return lq.reshape(6, *lq.shape[-2:])
    return np.concatenate([lq[0:3], lq[3 + m - 1:6 + m - 1]], axis=0)


def voxel_channels(lq, m, layout):
    if layout == "sharp":
        return lq[:0].reshape(0, *lq.shape[-2:])
    return np.concatenate([lq[3:3 + m - 1], lq[6 + m - 1:]], axis=0)
