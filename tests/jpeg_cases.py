"""The frames that test_jpeg_ref_host.py and test_hip_jpeg.py share, and their expected JFIF files from tests/jpeg_ref.py:
built once per case, read-only.  A case is (height, width, quality, subsampling, restart_mcus) over the six families."""
import functools

import numpy as np

import jpeg_ref as J
from test_hip_png_filter import _frame

SHAPES = [(1, 1), (8, 8), (16, 16), (7, 9), (17, 35), (33, 65), (5, 131)]
FAMILIES = ("flat", "waves", "noise", "blocks", "saturated", "lone63")
QUALITIES = [1, 50, 90, 100]
SUBSAMPLINGS = ["420", "444"]
RESTARTS = [1, 2, 3, None]


def _family(family, h, w, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    if family == "flat":
        return np.broadcast_to(np.array([200, 31, 97], dtype=np.uint8), (h, w, 3)).copy()
    if family in ("waves", "noise", "blocks"):
        return _frame(family, h, w, rng)
    if family == "saturated":
        # per 8x8 block, by (row + column) % 3: all 0, all 255 (DC differences up to category 11), or a 0 | 255 step
        # across the block (an AC coefficient of category 10 at quality 100)
        kind = (yy // 8 + xx // 8) % 3
        v = np.where(kind == 0, 0, np.where(kind == 1, 255, 255 * ((xx % 8) >= 4)))
        return np.repeat(v[:, :, None], 3, axis=2).astype(np.uint8)
    # lone63: grey, every 8x8 block the highest-frequency basis function alone: 62 zeros in front of coefficient 63,
    # so three ZRL and no EOB (where the block lies inside the frame)
    c = np.cos((2 * (np.arange(h + 8) % 8) + 1) * 7 * np.pi / 16)[:h, None] * np.cos((2 * (np.arange(w + 8) % 8) + 1) * 7 * np.pi / 16)[None, :w]
    v = np.rint(128 + 120 * c).astype(np.int64)
    return np.repeat(v[:, :, None], 3, axis=2).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def frames_of(h, w):
    """uint8 (6, H, W, 3), one frame per family."""
    rng = np.random.Generator(np.random.PCG64(1000 * h + w))
    frames = np.stack([_family(f, h, w, rng) for f in FAMILIES])
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def coefficients(h, w, quality, subsampling):
    """Per family the quantised zig-zag coefficients (MCUs, blocks per MCU, 64)."""
    ss = J.SUBSAMPLINGS[subsampling]
    return [J.quantise(J.dct_scaled(J.mcu_blocks(f, ss)), quality, ss) for f in frames_of(h, w)]


@functools.lru_cache(maxsize=None)
def expected(h, w, quality, subsampling, restart_mcus):
    """([file bytes per family], [info dict per family]) from the restatement."""
    outs, infos = [], []
    for zz in coefficients(h, w, quality, subsampling):
        info = {}
        outs.append(J.encode_coefficients(zz, h, w, quality, J.SUBSAMPLINGS[subsampling], restart_mcus, info))
        infos.append(info)
    return outs, infos
