"""The forward half of the PNG filters, for tests and tools/bench_png_decode.py: what an adaptive encoder (libpng's
heuristic) writes, so that the decoders meet Sub / Up / Average / Paeth rows.  Forward filtering reads original pixels
only -- a = the byte bpp to the left, b = the byte above, c = the byte above-left, 0 outside the image -- so all of it is
vectorised numpy.  The file is written through refid_amd.png's own chunk writer."""
import os
import struct
import zlib

import numpy as np

from refid_amd import png


def _planes(img):
    """(x, a, b, c) as int32 (H, stride) of a uint8 image (H, W, 3) or (H, W), and bpp."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3)) and img.size, (img.dtype, img.shape)
    bpp = 3 if img.ndim == 3 else 1
    x = img.reshape(img.shape[0], -1).astype(np.int32)
    a, b, c = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp]
    b[1:] = x[:-1]
    c[1:, bpp:] = x[:-1, :-bpp]
    return x, a, b, c, bpp


def _all_filtered(img):
    """uint8 (5, H, stride): every row filtered with each of the five types."""
    x, a, b, c, _ = _planes(img)
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]).astype(np.uint8)         # the cast wraps modulo 256


def apply_filters(img, types):
    """The inflate input of a PNG of ``img`` whose row y uses filter ``types[y]`` (0..4): uint8 (H, 1 + stride)."""
    types = np.asarray(types, dtype=np.int64).reshape(-1)
    cand = _all_filtered(img)
    assert types.shape == (cand.shape[1],) and types.min() >= 0 and types.max() <= 4, types
    rows = np.empty((cand.shape[1], 1 + cand.shape[2]), dtype=np.uint8)
    rows[:, 0] = types
    rows[:, 1:] = cand[types, np.arange(cand.shape[1])]
    return rows


def adaptive_types(img):
    """libpng's heuristic: per row the type whose filtered bytes, read as signed, have the least sum of absolute values
    (the lowest type on a tie)."""
    cand = _all_filtered(img).view(np.int8).astype(np.int32)
    return np.argmin(np.abs(cand).sum(axis=2), axis=0)


def encode_filtered(img, types, level=1):
    img = np.asarray(img)
    h, w = img.shape[:2]
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2 if img.ndim == 3 else 0, 0, 0, 0)
    data = zlib.compress(apply_filters(img, types).tobytes(), level)
    return png.SIGNATURE + png._chunk(b"IHDR", ihdr) + png._chunk(b"IDAT", data) + png._chunk(b"IEND", b"")


def write_filtered_png(path, img, types, level=1):
    """As png.write_png, with filter ``types[y]`` on row y."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(encode_filtered(img, types, level))
    return path
