"""A PNG writer and a reader for 8-bit RGB / grey files on the standard library alone: the validation image dumps of the
reference go through cv2.imwrite (utils/img_util.py:152-170), and cv2 is not a dependency here.  ``read_png`` decodes on
the host; ``read_filtered`` stops after inflate and leaves the per-row filters to the GPU (csrc/png.hip).

8-bit RGB (H, W, 3) or 8-bit grey (H, W); signature, IHDR, one IDAT, IEND; filter type 0 on every row; one
``zlib.compress``.  Level 1 by default: validation writes thousands of 720p frames and the encoder runs on the host.
``encode_png_rows`` / ``write_png_rows`` take rows the GPU has already filtered (``ops.png_filter``, csrc/png_filter.hip);
``wrap_zlib_stream`` / ``write_png_stream`` take the finished zlib stream of such rows (``ops.png_deflate``,
csrc/png_deflate.hip) and only add the chunk framing and the CRC."""
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


def encode_png_rows(rows, width, height, level=1, strategy=zlib.Z_HUFFMAN_ONLY):
    """The PNG (8-bit RGB) of rows that are ALREADY filtered: uint8, ``height`` rows of 1 + 3*``width`` bytes, the filter type
    (0..4) first in every row -- the output of ``ops.png_filter`` (csrc/png_filter.hip).  Signature, IHDR, one IDAT, IEND;
    the IDAT is one zlib stream from ``zlib.compressobj(level, DEFLATED, 15, 8, strategy)``.  Filtered rows are mostly small
    residuals, which Huffman codes already capture: Z_HUFFMAN_ONLY (the default) and Z_RLE skip the string matcher, where
    a deflate at level 1 spends its time.  Z_HUFFMAN_ONLY was the faster and the smaller of the two on every measured set
    (tools/bench_png_encode.py); it spends at least one bit per byte, so frames with large flat areas
    (long runs of zero residuals) come out smaller with ``strategy=zlib.Z_RLE``.  Every strategy gives a stream any
    inflate reads."""
    rows = np.asarray(rows)
    width, height = int(width), int(height)
    if rows.dtype != np.uint8 or width < 1 or height < 1 or rows.size != height * (1 + 3 * width):
        raise ValueError(f"write_png_rows: uint8 rows of {height}*(1 + 3*{width}) bytes expected, got {rows.dtype} {rows.shape}")
    deflate = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    data = deflate.compress(np.ascontiguousarray(rows).reshape(-1).data) + deflate.flush()
    ihdr = struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0)
    return SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", data) + _chunk(b"IEND", b"")


def write_png_rows(path, rows, width, height, level=1, strategy=zlib.Z_HUFFMAN_ONLY):
    """As ``write_png``, for rows that are already filtered (``encode_png_rows``)."""
    data = encode_png_rows(rows, width, height, level, strategy)
    parent = os.path.dirname(os.path.abspath(path))
    os.makedirs(parent, exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)
    return path


def wrap_zlib_stream(stream_bytes, width, height):
    """The PNG (8-bit RGB) whose image data is the finished zlib stream ``stream_bytes`` (bytes, or a uint8 array) of
    ``height`` filtered rows of 1 + 3*``width`` bytes -- a stream of ``ops.png_deflate`` (csrc/png_deflate.hip), cut to its
    length.  Signature, IHDR, one IDAT, IEND; the IDAT's CRC-32 is taken here, on the host, over the compressed bytes.
    The stream is not inflated: what it holds is the caller's business."""
    data = stream_bytes.tobytes() if isinstance(stream_bytes, np.ndarray) else bytes(stream_bytes)
    width, height = int(width), int(height)
    if width < 1 or height < 1 or len(data) < 2 + 5 + 4 or data[:2] != b"\x78\x01":
        raise ValueError(f"write_png_stream: a zlib stream (78 01 ...) for {height} rows of 1 + 3*{width} bytes expected, got "
                         f"{len(data)} bytes starting {data[:2].hex()}")
    ihdr = struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0)
    return SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", data) + _chunk(b"IEND", b"")


def write_png_stream(path, stream_bytes, width, height):
    """As ``write_png``, for image data that is already a zlib stream (``wrap_zlib_stream``)."""
    data = wrap_zlib_stream(stream_bytes, width, height)
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


def _unfilter(rows, bpp):
    """Undoes the per-row PNG filters (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth) of ``rows`` (h, 1 + stride) uint8; returns
    (h, stride).  Sub is a running sum along the row and Up adds the finished row above: both vectorised.  Average and
    Paeth depend on the byte just reconstructed, so they walk the row byte by byte: this is the host reference of
    csrc/png.hip, which decodes the command lines' frame directories on the GPU (``read_filtered``,
    ``sequence.load_png_frames``); frames written by this package use filter 0 and never get here."""
    h, stride = rows.shape[0], rows.shape[1] - 1
    out = np.zeros((h, stride), dtype=np.uint8)
    zero = np.zeros(stride, dtype=np.uint8)
    for y in range(h):
        ft, cur = int(rows[y, 0]), rows[y, 1:]
        up = out[y - 1] if y else zero
        if ft == 0:
            out[y] = cur
        elif ft == 1:                                       # x + left: a cumulative sum per byte lane, modulo 256
            lanes = cur.reshape(-1, bpp).astype(np.uint32)
            out[y] = (np.cumsum(lanes, axis=0) & 0xff).astype(np.uint8).reshape(-1)
        elif ft == 2:
            out[y] = cur + up                               # uint8 arithmetic wraps modulo 256
        elif ft in (3, 4):
            line, above, rec = cur.tolist(), up.tolist(), [0] * stride
            for i in range(stride):
                a = rec[i - bpp] if i >= bpp else 0
                b = above[i]
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    c = above[i - bpp] if i >= bpp else 0
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                rec[i] = (line[i] + pred) & 0xff
            out[y] = rec
        else:
            raise ValueError(f"read_png: unknown filter type {ft} in row {y}")
    return out


def _inflate(path):
    """(width, height, channels, rows) of an 8-bit RGB / grey, non-interlaced PNG: ``rows`` is the inflate output as uint8
    (H, 1 + W*channels), filter byte first, not unfiltered (a read-only view of the inflated bytes).  What ``read_png``
    and ``read_filtered`` share: signature, CRCs, IHDR and the length of the image data."""
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
    return w, h, ch, np.frombuffer(raw, dtype=np.uint8).reshape(h, 1 + w * ch)


def read_header(path):
    """(width, height, channels) as ``_inflate`` gives them, from the 33 bytes of the signature and IHDR alone: what
    ``sequence.load_png_frames`` sizes its staging by before any file is inflated.  A file whose head does not parse that way
    goes through ``read_filtered``, whose ValueError says what is wrong with it."""
    with open(path, "rb") as f:
        head = f.read(33)
    try:
        (tag, ihdr), = read_chunks(head)
        w, h, depth, colour, comp, flt, lace = struct.unpack(">IIBBBBB", ihdr)
        if tag != b"IHDR" or depth != 8 or colour not in (0, 2) or comp or flt or lace:
            raise ValueError
    except (ValueError, struct.error):
        return read_filtered(path)[:3]
    return w, h, 3 if colour == 2 else 1


def read_png(path):
    """Decodes an 8-bit RGB / grey, non-interlaced PNG (all five filter types) into a uint8 array (H, W, 3) / (H, W)."""
    w, h, ch, rows = _inflate(path)
    data = _unfilter(rows, ch) if rows[:, 0].any() else rows[:, 1:]
    img = data.reshape(h, w, ch) if ch == 3 else data
    return np.ascontiguousarray(img)


def check_filters(filters):
    """Raises ``_unfilter``'s ValueError for the first filter byte above 4 of ``filters`` (..., H); returns them."""
    filters = np.asarray(filters)
    bad = np.flatnonzero(filters.reshape(-1) > 4)
    if bad.size:
        raise ValueError(f"read_png: unknown filter type {int(filters.reshape(-1)[bad[0]])} in row {int(bad[0]) % filters.shape[-1]}")
    return filters


def read_filtered(path):
    """(width, height, channels, rows) with ``rows`` the inflate output, uint8 (H, 1 + W*channels), still filtered: the
    input of ``ops.png_unfilter`` (csrc/png.hip).  The file checks are ``read_png``'s; the filter bytes are checked here,
    on the host, so that the kernel never sees one above 4."""
    w, h, ch, rows = _inflate(path)
    check_filters(rows[:, 0])
    return w, h, ch, rows


def find_bands(filters, min_rows=64):
    """The band table of ``refid_png_unfilter`` for the filter bytes ``filters`` (N, H): int32 (n_bands, 3) rows
    [frame, row0, row1).  A row of type 0 (None) or 1 (Sub) does not read the row above, so a band may start there; one
    does where the band before has at least ``min_rows`` rows (64: a full wave of the kernel's four; shorter bands leave
    lanes idle, longer ones leave workgroups idle; 1: every independent run its own band)."""
    filters = np.asarray(filters)
    filters = check_filters(filters.reshape(-1, filters.shape[-1]))
    h, out = filters.shape[1], []
    for f, column in enumerate(filters):
        starts = np.flatnonzero(column <= 1)
        row0 = 0
        while True:
            k = np.searchsorted(starts, row0 + max(int(min_rows), 1))
            row1 = int(starts[k]) if k < starts.size else h
            out.append((f, row0, row1))
            if row1 == h:
                break
            row0 = row1
    return np.asarray(out, dtype=np.int32).reshape(-1, 3)
