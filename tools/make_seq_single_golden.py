#!/usr/bin/env python3
"""Generate tests/golden/seq_single_whole.npz: a sequence of blurry frames with ONE event stream, and per frame what
GoProSingleImageEventDataset.__getitem__ (data/Single_image_npy_dataset.py:136-201) gives for it at gt_size=None without
flips, run with THE REFERENCE's own functions.

Test infrastructure in the pattern of tools/make_single_golden.py: ``getitem`` is imported from there, the reference import
and the event generator from tools/make_sample_golden.py.  The sequence: 3 frames 26x38 (no multiple of 4 on either side:
the test-time assembler pads them), about 3000 events sorted by time, three exposure windows of which the first two
overlap.  Each item's events are the stream rows of its window (``refid_amd.sequence.pair_windows``), so the reference's
first / last stamps are those of ``make_pairs(..., stamps='events')``.

Per item k: ``i{k}/lq``, the pre-norm voxel ``i{k}/pre``, the normalised voxel ``i{k}/voxel`` and ``i{k}/d_ref``: the
largest distance of the reference's normalised voxel from the float64 normalisation of its own pre-norm voxel, in units of
the tests' bound B (single_assembly_ref.bound), measured against float64, never against the code under test.

Asserted here, on the CPU: every event lies inside the frame with a non-negative normalised time, and for every element the
reference's ``pre != 0`` mask equals "the element has contributions and their exact (float64) sum is non-zero" -- zero
disagreements.  The event generator's seed is the first from SEED0 on for which both hold; it is stored in the file.
Run:  REFID_REFERENCE=<reference checkout> python tools/make_seq_single_golden.py"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tools"), os.path.join(REPO, "tests")]
import single_assembly_ref as S  # noqa: E402  (float64 helpers and the bound B only)
from make_sample_golden import import_reference, make_events  # noqa: E402
from make_single_golden import getitem  # noqa: E402
from refid_amd.sequence import pair_windows  # noqa: E402  (only to CUT the stream into the items' rows)

BINS, H, W = 6, 26, 38
T0, T1 = 2.0, 2.5
WINDOWS = [(2.02, 2.20), (2.15, 2.36), (2.38, 2.49)]           # [start, end): the first two overlap
HOT = [(13, 12), (7, 30)]
SEED0 = 3000


def items_of(events):
    rows = pair_windows(events[:, 0], [w[0] for w in WINDOWS], [w[1] for w in WINDOWS])
    return [events[r0:r1] for r0, r1 in rows.tolist()], rows


def acceptable(events):
    """The generator's two CPU assertions as a predicate, for the seed search (event side only: frame and time)."""
    for ev in items_of(events)[0]:
        if len(ev) < 2 or ev[-1, 0] == ev[0, 0]:
            return False
        ts = (np.float32(BINS - 1) * (ev[:, 0] - ev[0, 0])) / np.float32(ev[-1, 0] - ev[0, 0])
        if not (np.all(ts >= 0) and np.all((ev[:, 1] >= 0) & (ev[:, 1] < W) & (ev[:, 2] >= 0) & (ev[:, 2] < H))):
            return False
    return True


def main():
    eu, tr, iu = import_reference()
    for seed in range(SEED0, SEED0 + 64):
        rng = np.random.Generator(np.random.PCG64(seed))
        frames = rng.integers(0, 256, (len(WINDOWS), H, W, 3), dtype=np.uint8)
        events = make_events(rng, H, W, T0, T1, 2300, HOT, 300)
        if not acceptable(events):
            continue
        evs, rows = items_of(events)
        rec = {"frames": frames, "events": events, "windows": np.array(WINDOWS, dtype=np.float64), "rows": rows,
               "config": np.array([BINS]), "seed": np.array(seed)}
        d_all, disagree = [], 0
        for k, ev in enumerate(evs):
            lq, pre, normed, _ = getitem(eu, tr, iu, [frames[k], frames[k]], ev, BINS, None, False, False, 0)
            e, cnt, mass = S.float64_sums(ev, BINS, H, W, 0, 0, H, W, False, False, False)
            disagree += int(np.count_nonzero((pre != 0) != ((cnt > 0) & (e != 0))))
            x64, mu, sigma = S.float64_norm(pre)
            b = S.bound(pre, mu, sigma, pre.size)
            nz = pre != 0
            d_ref = float((np.abs(normed.astype(np.float64) - x64)[nz] / b[nz]).max())
            assert np.all(normed[~nz] == 0)
            d_all.append(d_ref)
            rec[f"i{k}/lq"], rec[f"i{k}/pre"], rec[f"i{k}/voxel"], rec[f"i{k}/d_ref"] = lq, pre, normed, np.float64(d_ref)
        if disagree:
            print(f"seed {seed}: {disagree} mask disagreements, trying the next")
            continue
        assert acceptable(events) and disagree == 0
        assert rows[0, 1] > rows[1, 0], "windows 0 and 1 must share rows"
        path = os.path.join(REPO, "tests", "golden", "seq_single_whole.npz")
        np.savez_compressed(path, **rec)
        print(f"seq_single_whole: seed {seed}, {len(events)} events, rows {rows.tolist()}, voxel {pre.shape}, "
              f"d_ref max {max(d_all):.2f}, {os.path.getsize(path) / 1024:.0f} KiB")
        return
    raise SystemExit("no seed in range satisfies the assertions")


if __name__ == "__main__":
    main()
