"""Motion-JPEG in an AVI 1.0 container, written with the standard library: every frame is an independent baseline JPEG
file (``ops.jpeg_encode``, csrc/jpeg.hip), the container a few RIFF headers.

    RIFF 'AVI '
      LIST 'hdrl'
        'avih'  the main header: microseconds per frame, frame count, one stream, width, height; flag AVIF_HASINDEX
        LIST 'strl'
          'strh'  'vids' / 'MJPG', scale and rate = the frame rate as a fraction (rate / scale frames per second), length
          'strf'  BITMAPINFOHEADER: width, height, one plane, 24 bit, compression 'MJPG'
      LIST 'movi'
        '00dc' chunks, one JPEG file each, padded to an even length (the chunk's size field is the unpadded length)
      'idx1'  per frame: '00dc', AVIIF_KEYFRAME, the chunk's offset counted from the 'movi' fourcc, its unpadded length

The file is written as the frames arrive; the sizes and frame counts are patched at ``close``.  AVI 1.0 only (no OpenDML):
a RIFF size is 32 bits, so before a file would pass ``max_bytes`` the writer closes it and continues in
``stem.part002.avi`` and so on.  ``read_mjpeg_avi`` reads one such file back.  No player or ffmpeg has opened these files
where they were developed: the independent readers are PIL for the frames and ``read_mjpeg_avi`` for the container."""
import os
import struct
from fractions import Fraction

MAX_BYTES = 2 ** 31 - 2 ** 24          # safely under 2 GiB: readers that take RIFF sizes as signed still cope
AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10
_HDRL_BYTES = 4 + (8 + 56) + (8 + 4 + (8 + 56) + (8 + 40))     # 'hdrl', avih, LIST strl: 'strl', strh, strf
_MOVI_AT = 12 + 8 + _HDRL_BYTES        # file offset of the 'movi' LIST chunk
_FIRST_CHUNK = _MOVI_AT + 12


def fps_fraction(fps):
    """(rate, scale): ``fps`` as a fraction of two positive integers below 2^31; a float is taken to the nearest
    fraction with a denominator up to 1 001 000 (30000/1001 and its like are exact)."""
    if isinstance(fps, bool) or not isinstance(fps, (int, float, Fraction)):
        raise ValueError(f"fps {fps!r} is not a number")
    if not fps == fps or fps <= 0 or fps >= 2 ** 31:                  # (NaN, too)
        raise ValueError(f"fps {fps!r} is not positive and below 2^31")
    f = Fraction(fps).limit_denominator(1001000)
    if f <= 0:
        raise ValueError(f"fps {fps!r} is too small")
    return f.numerator, f.denominator


def _headers(width, height, rate, scale, frames, movi_bytes, riff_bytes, largest):
    """The bytes in front of the first '00dc' chunk."""
    usec = (1000000 * scale + rate // 2) // rate
    per_sec = (largest * rate + scale - 1) // scale
    avih = struct.pack("<14I", usec, min(per_sec, 2 ** 32 - 1), 0, AVIF_HASINDEX, frames, 0, 1, largest, width, height, 0, 0, 0, 0)
    strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, scale, rate, 0, frames, largest, 0xffffffff, 0, 0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", 3 * width * height, 0, 0, 0, 0)
    strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
    hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
    assert len(hdrl) == _HDRL_BYTES
    return (b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl +
            b"LIST" + struct.pack("<I", movi_bytes) + b"movi")


def part_path(path, part):
    """``path`` for part 1, ``stem.part002.avi`` and so on for the parts after it."""
    if part == 1:
        return path
    stem, ext = os.path.splitext(path)
    return f"{stem}.part{part:03d}{ext}"


class MjpegAviWriter:
    """``add(jpeg_bytes)`` appends a frame, ``close()`` finishes the file; ``paths`` lists the files written so far."""

    def __init__(self, path, width, height, fps, max_bytes=MAX_BYTES):
        if not (isinstance(width, int) and isinstance(height, int) and 1 <= width <= 65535 and 1 <= height <= 65535):
            raise ValueError(f"width {width!r} and height {height!r} must be integers 1 .. 65535")
        if not isinstance(max_bytes, int) or not _FIRST_CHUNK + 8 <= max_bytes <= 2 ** 32 - 1:
            raise ValueError(f"max_bytes {max_bytes!r} is not an integer {_FIRST_CHUNK + 8} .. 2^32 - 1")
        self.path, self.width, self.height, self.max_bytes = str(path), width, height, max_bytes
        self.rate, self.scale = fps_fraction(fps)
        self.paths, self.frames = [], 0
        self._file = None
        folder = os.path.dirname(self.path)
        if folder:
            os.makedirs(folder, exist_ok=True)
        self._open()

    def _open(self):
        self.paths.append(part_path(self.path, len(self.paths) + 1))
        self._file = open(self.paths[-1], "wb")
        self._index, self._at, self._largest = [], _FIRST_CHUNK, 0
        self._file.write(_headers(self.width, self.height, self.rate, self.scale, 0, 4, 0, 0))

    def _finish(self):
        f, n = self._file, len(self._index)
        f.write(b"idx1" + struct.pack("<I", 16 * n))
        f.write(b"".join(b"00dc" + struct.pack("<III", AVIIF_KEYFRAME, off, size) for off, size in self._index))
        total = self._at + 8 + 16 * n
        f.seek(0)
        f.write(_headers(self.width, self.height, self.rate, self.scale, n, self._at - _MOVI_AT - 8, total - 8, self._largest))
        f.close()
        self._file = None

    def add(self, jpeg_bytes):
        if self._file is None:
            raise ValueError("MjpegAviWriter: the writer is closed")
        data = bytes(jpeg_bytes)
        padded = len(data) + (len(data) & 1)
        grown = lambda: self._at + 8 + padded + 8 + 16 * (len(self._index) + 1)      # noqa: E731  the file's size with this frame
        if self._index and grown() > self.max_bytes:
            self._finish()
            self._open()
        if grown() > 2 ** 32 - 1:
            raise ValueError(f"MjpegAviWriter: a frame of {len(data)} bytes does not fit an AVI 1.0 file")
        self._file.write(b"00dc" + struct.pack("<I", len(data)) + data + b"\0" * (padded - len(data)))
        self._index.append((self._at - _MOVI_AT - 8, len(data)))
        self._at += 8 + padded
        self._largest = max(self._largest, len(data))
        self.frames += 1

    def close(self):
        """Writes the index and patches the sizes; the paths of all parts are in ``paths``.  Closing twice is harmless."""
        if self._file is not None:
            self._finish()
        return self.paths

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def read_mjpeg_avi(path):
    """(header dict, [frame bytes]) of one file ``MjpegAviWriter`` wrote (any AVI with one MJPG stream laid out the same
    way): width, height, frames (avih), length (strh), rate, scale, fps (a Fraction), usec_per_frame, handler, compression,
    index: [(offset from the 'movi' fourcc, length)].  The frames come from walking 'movi'; the index is checked against it
    by the caller if they care."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError(f"{path}: not a RIFF AVI file")
    riff_end = 8 + struct.unpack_from("<I", data, 4)[0]
    if riff_end > len(data):
        raise ValueError(f"{path}: the RIFF size {riff_end - 8} passes the end of the file")
    head, frames = {"riff_bytes": riff_end - 8}, []

    def walk(lo, hi, inside):
        at = lo
        while at + 8 <= hi:
            four, size = data[at:at + 4], struct.unpack_from("<I", data, at + 4)[0]
            body = at + 8
            if body + size > hi:
                raise ValueError(f"{path}: chunk {four!r} at {at} passes the end of {inside!r}")
            if four == b"LIST":
                kind = data[body:body + 4]
                if kind == b"movi":
                    head["movi_at"] = body
                walk(body + 4, body + size, kind)
            elif four == b"avih":
                v = struct.unpack_from("<14I", data, body)
                head.update(usec_per_frame=v[0], flags=v[3], frames=v[4], streams=v[6], width=v[8], height=v[9])
            elif four == b"strh":
                head.update(stream_type=data[body:body + 4], handler=data[body + 4:body + 8])
                v = struct.unpack_from("<IIII", data, body + 20)
                head.update(scale=v[0], rate=v[1], length=v[3], fps=Fraction(v[1], v[0]))
            elif four == b"strf":
                v = struct.unpack_from("<IiiHH4s", data, body)
                head.update(bitmap_width=v[1], bitmap_height=v[2], bit_count=v[4], compression=v[5])
            elif four == b"idx1":
                head["index"] = [struct.unpack_from("<II", data, body + 16 * k + 8) for k in range(size // 16)]
                head["index_ids"] = [data[body + 16 * k:body + 16 * k + 4] for k in range(size // 16)]
                head["index_flags"] = [struct.unpack_from("<I", data, body + 16 * k + 4)[0] for k in range(size // 16)]
            elif inside == b"movi" and four == b"00dc":
                frames.append(data[body:body + size])
            at = body + size + (size & 1)
    walk(12, riff_end, b"AVI ")
    for key in ("width", "rate", "compression", "movi_at"):
        if key not in head:
            raise ValueError(f"{path}: no {'movi list' if key == 'movi_at' else key} found")
    return head, frames
