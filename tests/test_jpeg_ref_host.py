"""CPU-only: pins tests/jpeg_ref.py, the numpy restatement of csrc/jpeg.hip's stream, before the GPU is compared with it
byte for byte (tests/test_hip_jpeg.py) -- against PIL's decoder and encoder, a float64 DCT and a marker walker -- and
refid_amd/video.py's container against its own reader and the byte layout."""
import io
import json
import os
import struct
from fractions import Fraction

import numpy as np
import pytest

import jpeg_cases as K
import jpeg_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIL_SUBSAMPLING = {"444": 0, "420": 2}


def _pil(data):
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def _pil_encode(frame, quality, subsampling):
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, "JPEG", quality=quality, subsampling=PIL_SUBSAMPLING[subsampling], optimize=False)
    return buf.getvalue()


def walk_markers(data):
    """[(marker, payload)] of the segments in front of the scan, the entropy-coded segments, the RSTm numbers between
    them, and what follows the scan."""
    assert data[:2] == b"\xff\xd8"
    at, segments = 2, []
    while True:
        assert data[at] == 0xff, at
        marker, size = data[at + 1], struct.unpack_from(">H", data, at + 2)[0]
        segments.append((marker, data[at + 4:at + 2 + size]))
        at += 2 + size
        if marker == 0xda:
            break
    scans, restarts, start = [], [], at
    while True:
        at = data.index(b"\xff", at)
        if data[at + 1] == 0x00:
            at += 2
        elif 0xd0 <= data[at + 1] <= 0xd7:
            scans.append(data[start:at])
            restarts.append(data[at + 1] - 0xd0)
            at = start = at + 2
        else:
            scans.append(data[start:at])
            return segments, scans, restarts, data[at:]


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_case_loads_in_pil_with_pils_tables_and_the_markers_in_place(shape):
    h, w = shape
    for quality in K.QUALITIES:
        for subsampling in K.SUBSAMPLINGS:
            ss = J.SUBSAMPLINGS[subsampling]
            theirs = _pil(_pil_encode(K.frames_of(h, w)[0], quality, subsampling))
            for restart in K.RESTARTS:
                m, rows, cols, bpm, interval, segs = J.geometry(h, w, ss, restart)
                for family, data in zip(K.FAMILIES, K.expected(h, w, quality, subsampling, restart)[0]):
                    what = (h, w, quality, subsampling, restart, family)
                    im = _pil(data)
                    assert im.mode == "RGB" and im.size == (w, h), what
                    assert {k: list(v) for k, v in im.quantization.items()} == {k: list(v) for k, v in theirs.quantization.items()}, what
                    assert len(data) <= J.bound(h, w, ss, restart), what
                    segments, scans, restarts, tail = walk_markers(data)
                    assert [s[0] for s in segments] == [0xe0, 0xdb, 0xc0, 0xc4, 0xc4, 0xc4, 0xc4, 0xdd, 0xda], what
                    assert data[:J.HEADER_BYTES] == J.header(h, w, quality, ss, restart), what
                    assert J.HEADER_BYTES + sum(map(len, scans)) + 2 * (segs - 1) + 2 == len(data), what
                    assert struct.unpack(">H", segments[7][1])[0] == interval == (cols if restart is None else restart), what
                    assert len(scans) == segs and restarts == [k % 8 for k in range(segs - 1)], what
                    assert tail == b"\xff\xd9", what                  # no marker behind the last segment but EOI
                    sof = segments[2][1]
                    assert sof[:6] == bytes([8]) + struct.pack(">HH", h, w) + bytes([3]), what
                    assert sof[6:] == bytes([1, 0x22 if subsampling == "420" else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]), what


def test_the_huffman_tables_are_the_ones_pil_writes():
    """PIL (libjpeg) writes the Annex K tables K.3 .. K.6 when it does not optimise: ours are the same bytes."""
    ours = [s[1] for s in walk_markers(K.expected(16, 16, 90, "420", None)[0][0])[0] if s[0] == 0xc4]
    theirs = b"".join(s[1] for s in walk_markers(_pil_encode(K.frames_of(16, 16)[1], 90, "420"))[0] if s[0] == 0xc4)
    tables, at = {}, 0
    while at < len(theirs):                                            # libjpeg may put several tables into one DHT segment
        n = sum(theirs[at + 1:at + 17])
        tables[theirs[at]] = theirs[at:at + 17 + n]
        at += 17 + n
    assert [t[0] for t in ours] == [0x00, 0x10, 0x01, 0x11] and all(tables[t[0]] == t for t in ours)


def test_the_integer_dct_is_within_one_of_a_float64_dct():
    k = np.arange(8)
    basis = np.where(k[:, None] == 0, np.sqrt(0.125), 0.5) * np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16)
    worst = 0.0
    for h, w in K.SHAPES:
        for subsampling in K.SUBSAMPLINGS:
            for frame in K.frames_of(h, w):
                blocks = J.mcu_blocks(frame, J.SUBSAMPLINGS[subsampling])
                exact = np.einsum("vy,...yx,ux->...vu", basis, blocks.astype(np.float64) - 128.0, basis)
                worst = max(worst, float(np.abs(J.dct_scaled(blocks) / float(1 << 20) - exact).max()))
    print(f"largest deviation of the unquantised coefficients from the float64 orthonormal DCT: {worst:.6f}")
    assert worst <= 1.0


def _psnr(a, b):
    mse = float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean())
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def test_psnr_is_within_a_tenth_of_a_decibel_of_pils_own_encode():
    """PSNR against the source of our file decoded by PIL >= that of PIL's own encode (same quality and subsampling, not
    optimised) decoded by PIL, minus 0.1 dB -- per shape from 16x16 up, family, quality and subsampling.  The two encoders
    differ only in sub-quantisation-step roundings.  Flat frames, where both may be infinite, compare pixels instead."""
    record, short = [], []
    for h, w in [s for s in K.SHAPES if s[0] >= 16 and s[1] >= 16]:
        for quality in K.QUALITIES:
            for subsampling in K.SUBSAMPLINGS:
                ours_all = K.expected(h, w, quality, subsampling, None)[0]
                for family, frame, data in zip(K.FAMILIES, K.frames_of(h, w), ours_all):
                    ours = np.asarray(_pil(data))
                    theirs = np.asarray(_pil(_pil_encode(frame, quality, subsampling)))
                    a, b = _psnr(ours, frame), _psnr(theirs, frame)
                    record.append(dict(shape=f"{h}x{w}", family=family, quality=quality, subsampling=subsampling,
                                       ours_db=None if np.isinf(a) else round(a, 4), pil_db=None if np.isinf(b) else round(b, 4)))
                    if family == "flat":
                        assert np.array_equal(ours, theirs), (h, w, family, quality, subsampling)
                    elif not a >= b - 0.1:
                        short.append((h, w, family, quality, subsampling, round(a, 4), round(b, 4)))
    with open(os.path.join(ROOT, "profiles", "jpeg_ref_psnr.json"), "w") as f:
        json.dump(dict(note="PSNR (dB) against the source, decoded by PIL: tests/jpeg_ref.py's file and PIL's own encode at the same "
                            "quality and subsampling, optimize=False; null = identical to the source", cases=record), f, indent=1)
        f.write("\n")
    assert not short, short


def test_the_cases_reach_the_corners_of_the_coder():
    infos = [(h, w, q, s, r, f, i, d) for h, w in K.SHAPES for q in K.QUALITIES for s in K.SUBSAMPLINGS for r in K.RESTARTS
             for f, i, d in zip(K.FAMILIES, K.expected(h, w, q, s, r)[1], K.expected(h, w, q, s, r)[0])]
    assert any(i.get("stuffed", 0) > 0 and b"\xff\x00" in d[J.HEADER_BYTES:] for *_, i, d in infos)
    assert any(i.get("zrl", 0) > 0 for *_, i, d in infos)
    assert any(i.get("no_eob", 0) > 0 for *_, i, d in infos)
    assert max(i["dc_category"] for *_, i, d in infos) >= 10
    assert max(i.get("ac_category", 0) for *_, i, d in infos) == 10
    lone = [i for h, w, q, s, r, f, i, d in infos if f == "lone63" and (h, w) == (16, 16) and q == 50 and s == "444" and r is None][0]
    assert lone["zrl"] == 3 * 4 and lone["no_eob"] == 4                # Y of four blocks: 62 zeros, then coefficient 63
    long = [d for h, w, q, s, r, f, i, d in infos if (h, w, q, s, r, f) == (33, 65, 100, "444", None, "noise")][0]
    assert J.default_pitch(33, 65) < len(long) <= J.bound(33, 65, J.J444, None)
    assert J.geometry(33, 65, J.J420, 1)[5] > 8 and J.geometry(33, 65, J.J444, 1)[5] > 8


def _jpegs(n, size=lambda k: 40 + 7 * k):
    return [bytes([0xff, 0xd8]) + bytes((k * 31 + j) % 251 for j in range(size(k) - 4)) + bytes([0xff, 0xd9]) for k in range(n)]


def test_avi_round_trip_and_layout(tmp_path):
    from refid_amd.video import AVIIF_KEYFRAME, MjpegAviWriter, read_mjpeg_avi
    frames = _jpegs(7)                                                 # odd and even lengths
    path = tmp_path / "sub" / "clip.avi"
    writer = MjpegAviWriter(str(path), 50, 37, 30000 / 1001)
    for f in frames:
        writer.add(f)
    assert writer.close() == [str(path)] and writer.close() == [str(path)] and writer.frames == 7
    with pytest.raises(ValueError, match="closed"):
        writer.add(frames[0])
    head, got = read_mjpeg_avi(str(path))
    assert got == frames
    data = path.read_bytes()
    assert head["riff_bytes"] == len(data) - 8 and data[8:12] == b"AVI "
    assert (head["width"], head["height"], head["frames"], head["length"], head["streams"]) == (50, 37, 7, 7, 1)
    assert (head["bitmap_width"], head["bitmap_height"], head["bit_count"]) == (50, 37, 24)
    assert head["stream_type"] == b"vids" and head["handler"] == b"MJPG" and head["compression"] == b"MJPG"
    assert (head["rate"], head["scale"]) == (30000, 1001) and head["fps"] == Fraction(30000, 1001) and head["usec_per_frame"] == 33367
    assert head["flags"] & 0x10 and head["index_ids"] == [b"00dc"] * 7 and head["index_flags"] == [AVIIF_KEYFRAME] * 7
    movi = head["movi_at"]
    assert data[movi:movi + 4] == b"movi" and data[movi - 8:movi - 4] == b"LIST"
    at = 4
    for (off, size), f in zip(head["index"], frames):
        assert (off, size) == (at, len(f))
        assert data[movi + off:movi + off + 4] == b"00dc" and struct.unpack_from("<I", data, movi + off + 4)[0] == len(f)
        assert data[movi + off + 8:movi + off + 8 + size] == f
        at += 8 + len(f) + (len(f) & 1)                                # chunks start at even offsets
        assert at % 2 == 0
    assert struct.unpack_from("<I", data, movi - 4)[0] == at and data[movi + at:movi + at + 4] == b"idx1"
    assert len(data) == movi + at + 8 + 16 * 7


def test_avi_parts_and_zero_frames(tmp_path):
    from refid_amd.video import MjpegAviWriter, part_path, read_mjpeg_avi
    frames = _jpegs(10, size=lambda k: 100)
    path = str(tmp_path / "clip.avi")
    with MjpegAviWriter(path, 8, 8, 25, max_bytes=700) as writer:        # headers 224 + 3 chunks of 108 + index 8 + 48 = 604
        for f in frames:
            writer.add(f)
    assert writer.paths == [part_path(path, k) for k in (1, 2, 3, 4)] and writer.paths[1].endswith("clip.part002.avi")
    got = []
    for k, p in enumerate(writer.paths):
        head, part = read_mjpeg_avi(p)
        assert os.path.getsize(p) <= 700 and head["frames"] == head["length"] == len(part) == (3 if k < 3 else 1)
        assert (head["rate"], head["scale"]) == (25, 1) and len(head["index"]) == len(part)
        got += part
    assert got == frames
    with MjpegAviWriter(path, 8, 8, 25, max_bytes=300) as writer:        # a frame larger than max_bytes still gets a file of its own
        writer.add(frames[0])
        writer.add(frames[1])
    assert [read_mjpeg_avi(p)[1] for p in writer.paths] == [[frames[0]], [frames[1]]]
    empty = str(tmp_path / "empty.avi")
    MjpegAviWriter(empty, 640, 480, 30).close()
    head, none = read_mjpeg_avi(empty)
    assert none == [] and head["frames"] == 0 and head["length"] == 0 and head["index"] == [] and head["width"] == 640
    assert head["riff_bytes"] == os.path.getsize(empty) - 8
    for bad in (dict(fps=0), dict(fps=-1), dict(fps="fast"), dict(fps=float("nan")), dict(width=0), dict(height=70000), dict(max_bytes=10)):
        with pytest.raises(ValueError):
            MjpegAviWriter(**dict(dict(path=empty, width=8, height=8, fps=30), **bad))
    with pytest.raises(ValueError, match="RIFF AVI"):
        (tmp_path / "x.avi").write_bytes(b"not a video")
        read_mjpeg_avi(str(tmp_path / "x.avi"))
