"""numpy restatement of the single-image item assembly of a resident sequence (refid_amd/csrc/sequence.hip:
refid_seq_assemble_single), built on single_assembly_ref.assemble_sample: per item the blurry frame `left` and the stream
rows [row0, row1) at a whole-frame crop without flips -- the statistics of voxel_norm over the UNPADDED sample -- then
np.pad: mode="edge" for lq, zeros for voxel.  Shared by test_sequence_single_host.py and test_hip_sequence_single.py."""
import os

import numpy as np

import single_assembly_ref as A
from sequence_ref import round_up

FIXTURE = "seq_single_whole"


def load_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, FIXTURE + ".npz"))
    return z, int(z["config"][0])


def assemble_item(frames, events, item, bins, out_h, out_w, norm=True, bgr=False):
    """One item (left, right, row0, row1, first_stamp, last_stamp) -> (lq, voxel, pre-norm voxel); lq and voxel at
    (out_h, out_w), the pre-norm voxel unpadded."""
    left, _, row0, row1, first, last = item
    f = np.asarray(frames)[left]
    if not bgr:
        f = f[..., ::-1]                                                       # assemble_sample swaps BGR -> RGB
    H, W = f.shape[:2]
    ev = np.asarray(events, dtype=np.float32).reshape(-1, 4)[row0:row1]
    sample = dict(frames=np.stack([f, f]), events=ev, first_stamp=np.float32(first), last_stamp=np.float32(last))
    lq, voxel, _, pre = A.assemble_sample(sample, bins, None, norm)
    ph, pw = out_h - H, out_w - W
    lq = np.pad(lq, ((0, 0), (0, ph), (0, pw)), mode="edge")
    voxel = np.pad(voxel, ((0, 0), (0, ph), (0, pw)))
    return np.ascontiguousarray(lq), np.ascontiguousarray(voxel), pre


def assemble_items(frames, events, items, bins, multiple=4, norm=True, bgr=False):
    H, W = np.asarray(frames).shape[1:3]
    oh, ow = round_up(H, multiple), round_up(W, multiple)
    outs = [assemble_item(frames, events, it, bins, oh, ow, norm, bgr) for it in items]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
