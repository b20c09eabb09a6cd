"""Blurry key frames from high-frame-rate video: averages of consecutive sharp frames on the GPU (csrc/blur_synth.hip; the
contract is "Blur synthesis" in include/refid_hip.h, tests/blur_ref.py restates it).

The reference reads GoPro's ``blur/`` PNGs, which are such averages, and its dataset code fixes which sharp frames belong
to which blurry frame (basicsr/data/image_npy_dataset.py:75-86): with P = m + n, blurry frame i is made of the sharp
frames [iP, iP + m), and pair i has the ground truth [iP, (i+1)P + m), 2m + n frames.  ``blur_windows`` follows that
indexing.  Two modes: the plain mean of the codes (``blur/``), or the mean in linear light through a 256-entry response
table (``blur_gamma/``), looked up back to the nearest code.  The arithmetic is integer, so the frames are reproducible to
the bit.

Not modelled: exposures that start or end between two frames, temporal upsampling before averaging, noise, saturation,
16-bit frames.  There is no host fallback."""
import numpy as np

from . import _lib
from ._lib import RefidHipError

LINEAR_ONE = 1 << 24         # the level of code 255 in a response table


def gamma_table(gamma):
    """uint32 [256]: rint(2^24 (c / 255)^gamma) in float64, c = 0 .. 255, for ``gamma`` in [1, 3].  1.0 is legal and is not
    the plain mode: the levels are averaged at 24 bits and rounded to a code once."""
    try:
        g = float(gamma)
    except (TypeError, ValueError):
        raise RefidHipError(f"gamma_table: gamma {gamma!r} is not a number") from None
    if not 1.0 <= g <= 3.0:
        raise RefidHipError(f"gamma_table: gamma {g} must be 1 .. 3")
    c = np.arange(256, dtype=np.float64)
    return np.rint(float(LINEAR_ONE) * (c / 255.0) ** g).astype(np.uint32)


def blur_windows(n_frames, m, n):
    """(windows int32 (K, 2) rows [first, count], key_first int64 (K,)) of ``n_frames`` sharp frames: blurry frame i
    averages the m frames from i (m + n) on, K = (n_frames - m) // (m + n) + 1; RefidHipError when not even one fits."""
    n_frames, m, n = int(n_frames), int(m), int(n)
    if not 1 <= m <= _lib.BLUR_MAX_COUNT:
        raise RefidHipError(f"blur_windows: m {m} must be 1 .. {_lib.BLUR_MAX_COUNT} frames per blurry frame")
    if n < 0:
        raise RefidHipError(f"blur_windows: n {n} must not be negative")
    if n_frames < m:
        raise RefidHipError(f"blur_windows: {n_frames} frames do not hold one blurry frame of m = {m}")
    k = (n_frames - m) // (m + n) + 1
    first = np.arange(k, dtype=np.int64) * (m + n)
    windows = np.stack([first, np.full((k,), m, dtype=np.int64)], axis=1).astype(np.int32)
    return windows, first


def synthesize(frames_u8, m, n, gamma=None):
    """(keys uint8 (K, H, W, 3) on the device, windows) of the resident frames uint8 (N, H, W, 3): the blurry key frames of
    ``blur_windows(N, m, n)``; ``gamma`` None averages the codes, a number in [1, 3] the levels of ``gamma_table(gamma)``.
    Does not synchronise."""
    from . import ops
    if not hasattr(frames_u8, "shape") or len(frames_u8.shape) != 4:
        raise RefidHipError("synthesize: frames must be a uint8 (N, H, W, 3) CUDA tensor (no CPU fallback)")
    windows, _ = blur_windows(int(frames_u8.shape[0]), m, n)
    table = None if gamma is None else gamma_table(gamma)
    return ops.blur_synth(frames_u8, windows, to_linear=table), windows


def exposures(stamps, windows):
    """float64 (K, 2) rows [start, end] of the windows: the stamps of the first and of the last averaged frame.  With
    count = 1, start == end, and ``sequence.exposure_windows`` yields the sharp layout's windows."""
    stamps = np.asarray(stamps, dtype=np.float64).reshape(-1)
    windows = np.asarray(windows, dtype=np.int64).reshape(-1, 2)
    first, last = windows[:, 0], windows[:, 0] + windows[:, 1] - 1
    if windows.shape[0] and (int(first.min()) < 0 or int(windows[:, 1].min()) < 1 or int(last.max()) >= stamps.shape[0]):
        raise RefidHipError(f"exposures: a window lies outside the {stamps.shape[0]} stamps")
    return np.stack([stamps[first], stamps[last]], axis=1)
