"""A restatement of csrc/blur_synth.hip in plain numpy and Python ints ("Blur synthesis" in include/refid_hip.h): the two
averaging formulas, the response table and the reference's window indexing, written independently of refid_amd.blur_synth.
The device is compared with this bit for bit."""
import numpy as np

MAX_COUNT = 64
LINEAR_ONE = 1 << 24


def gamma_table(gamma):
    """uint32 [256]: 2^24 (c / 255)^gamma rounded to the nearest integer (half to even), entry by entry in Python floats."""
    return np.array([int(round(16777216.0 * (c / 255.0) ** float(gamma))) for c in range(256)], dtype=np.uint32)


def thresholds(table):
    """Python ints thr[0..255]: thr[c] = (L[c-1] + L[c] + 1) >> 1, thr[0] = 0 (never read by the count below)."""
    L = [int(v) for v in table]
    return [0] + [(L[c - 1] + L[c] + 1) >> 1 for c in range(1, 256)]


def check_table(table):
    L = [int(v) for v in np.asarray(table).reshape(-1)]
    assert len(L) == 256
    assert all(L[c] > L[c - 1] for c in range(1, 256)), "the table is not strictly increasing"
    assert 0 <= L[0] and L[255] <= LINEAR_ONE


def blur_window(stack, to_linear=None):
    """One blurry frame from ``stack`` uint8 (count, ...): int64 sums, integer division, and in response mode the number of
    thresholds at or below the mean level."""
    stack = np.asarray(stack)
    assert stack.dtype == np.uint8 and 1 <= stack.shape[0] <= MAX_COUNT
    count = int(stack.shape[0])
    if to_linear is None:
        total = stack.astype(np.int64).sum(axis=0)
        return ((total + count // 2) // count).astype(np.uint8)
    check_table(to_linear)
    L = np.asarray(to_linear, dtype=np.int64).reshape(-1)
    total = L[stack].sum(axis=0)
    assert int(total.max()) + count // 2 < 2 ** 31
    v = (total + count // 2) // count
    thr = np.array(thresholds(to_linear)[1:], dtype=np.int64)                    # thr[1..255], ascending
    return np.searchsorted(thr, v, side="right").astype(np.uint8)               # #{c in 1..255 : thr[c] <= v}


def blur_byte(codes, to_linear=None):
    """The same for one byte position, in Python ints only (no numpy arithmetic): ``codes`` is a sequence of count codes."""
    codes = [int(c) for c in codes]
    count = len(codes)
    assert 1 <= count <= MAX_COUNT
    if to_linear is None:
        return (sum(codes) + count // 2) // count
    L = [int(v) for v in to_linear]
    v = (sum(L[c] for c in codes) + count // 2) // count
    thr = thresholds(to_linear)
    return sum(1 for c in range(1, 256) if thr[c] <= v)


def blur_synth(frames, windows, to_linear=None):
    """uint8 (K, H, W, 3) of frames uint8 (N, H, W, 3) and windows (K, 2) rows [first, count]."""
    frames = np.asarray(frames)
    out = []
    for first, count in np.asarray(windows).reshape(-1, 2).tolist():
        assert 1 <= count <= MAX_COUNT and 0 <= first and first + count <= frames.shape[0]
        out.append(blur_window(frames[first:first + count], to_linear))
    return np.stack(out, axis=0)


def blur_windows(n_frames, m, n):
    """([[first, count]] , [first]) by the reference's indexing (basicsr/data/image_npy_dataset.py:75-86): blurry frame i
    is made of the sharp frames [i (m + n), i (m + n) + m); as many as fit into n_frames."""
    rows, i = [], 0
    while i * (m + n) + m <= n_frames:
        rows.append([i * (m + n), m])
        i += 1
    if not rows:
        raise ValueError(f"{n_frames} frames do not hold one window of {m}")
    return np.array(rows, dtype=np.int32), [r[0] for r in rows]


def exposures(stamps, windows):
    return np.array([[float(stamps[f]), float(stamps[f + c - 1])] for f, c in np.asarray(windows).tolist()], dtype=np.float64)
