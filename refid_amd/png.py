"""A PNG writer (and a reader for its own files) on the standard library alone: the validation image dumps of the
reference go through cv2.imwrite (utils/img_util.py:152-170), and cv2 is not a dependency here.

8-bit RGB (H, W, 3) or 8-bit grey (H, W); signature, IHDR, one IDAT, IEND; filter type 0 on every row; one
``zlib.compress``.  Level 1 by default: validation writes thousands of 720p frames and the encoder runs on the host."""
import os
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def encode_png(img, level=1):
    img = np.asarray(img)
    if img.dtype != np.uint8 or not (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3)) or img.size == 0:
        raise ValueError(f"write_png: uint8 (H, W, 3) RGB or (H, W) grey expected, got {img.dtype} {img.shape}")
    h, w = img.shape[:2]
    rows = np.zeros((h, 1 + w * (img.size // (h * w))), dtype=np.uint8)        # column 0: filter type 0 (None)
    rows[:, 1:] = img.reshape(h, -1)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2 if img.ndim == 3 else 0, 0, 0, 0)
    return SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _chunk(b"IEND", b"")


def write_png(path, img, level=1):
    """img: uint8 numpy array, (H, W, 3) in RGB order or (H, W).  Creates the parent directory, as imwrite does."""
    data = encode_png(img, level)
    parent = os.path.dirname(os.path.abspath(path))
    os.makedirs(parent, exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)
    return path


def read_chunks(data):
    """[(tag, payload)] of a PNG byte string; raises ValueError on a bad signature, length or CRC."""
    if data[:8] != SIGNATURE:
        raise ValueError("read_png: not a PNG signature")
    out, pos = [], 8
    while pos < len(data):
        if pos + 12 > len(data):
            raise ValueError("read_png: truncated chunk")
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        tag, payload = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        if len(payload) != n or pos + 12 + n > len(data):
            raise ValueError("read_png: truncated chunk")
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        if crc != (zlib.crc32(tag + payload) & 0xffffffff):
            raise ValueError(f"read_png: CRC mismatch in {tag!r}")
        out.append((tag, payload))
        pos += 12 + n
    return out


def read_png(path):
    """Decodes what write_png writes (8-bit RGB / grey, no interlace, filter 0 only) into a uint8 array."""
    with open(path, "rb") as f:
        chunks = read_chunks(f.read())
    if not chunks or chunks[0][0] != b"IHDR" or chunks[-1][0] != b"IEND":
        raise ValueError("read_png: IHDR / IEND missing")
    w, h, depth, colour, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    if depth != 8 or colour not in (0, 2) or comp or flt or lace:
        raise ValueError("read_png: only 8-bit RGB / grey, non-interlaced files are supported")
    ch = 3 if colour == 2 else 1
    raw = zlib.decompress(b"".join(p for t, p in chunks if t == b"IDAT"))
    if len(raw) != h * (1 + w * ch):
        raise ValueError("read_png: image data has the wrong length")
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(h, 1 + w * ch)
    if rows[:, 0].any():
        raise ValueError("read_png: only filter type 0 is supported")
    img = rows[:, 1:].reshape(h, w, ch) if ch == 3 else rows[:, 1:]
    return np.ascontiguousarray(img)
