"""numpy restatement of the pair-assembly kernels (refid_amd/csrc/sequence.hip), built on the functions of
sample_assembly_ref.py: the same event arithmetic with no crop and no flips, then np.pad -- zeros for voxel channels,
mode="edge" for image channels.  Shared by test_sequence_host.py and test_hip_sequence.py."""
import numpy as np

import sample_assembly_ref as R


def round_up(v, multiple):
    return (v + multiple - 1) // multiple * multiple


def assemble_pair(frames, events, pair, m, n, layout, out_h, out_w, bgr):
    """One pair (left, right, row0, row1, first_stamp, last_stamp) of a sequence -> (lq, voxel) float32 at (out_h, out_w)."""
    left, right, row0, row1, first, last = pair
    bins = R.num_bins(m, n, layout)
    frames = np.asarray(frames)
    H, W = frames.shape[1:3]
    ev = np.asarray(events, dtype=np.float32).reshape(-1, 4)[row0:row1]
    vox = R.fixed_to_float(R.accumulate(ev, first, last, bins, H, W, 0, 0, H, W, False, False, False))
    two = frames[[left, right]]
    if not bgr:
        two = two[..., ::-1]                                                   # frames_to_chw swaps BGR -> RGB
    img = R.frames_to_chw(two, 0, 0, 0, 0, H, W, False, False, False)
    ph, pw = out_h - H, out_w - W
    vox = np.pad(vox, ((0, 0), (0, ph), (0, pw)))
    img = np.pad(img, ((0, 0), (0, 0), (0, ph), (0, pw)), mode="edge")
    voxel = np.stack([vox[:-1], vox[1:]], axis=1)                              # (bins-1, 2, h, w)
    if layout == "blur":
        lq = np.concatenate([img[0], vox[1:m], img[1], vox[m + 2 + n:]], axis=0)
    else:
        lq = img
    return np.ascontiguousarray(lq), np.ascontiguousarray(voxel)


def assemble_pairs(frames, events, pairs, m, n, layout, multiple=8, bgr=False):
    H, W = np.asarray(frames).shape[1:3]
    oh, ow = round_up(H, multiple), round_up(W, multiple)
    outs = [assemble_pair(frames, events, p, m, n, layout, oh, ow, bgr) for p in pairs]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
