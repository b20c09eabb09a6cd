"""CPU-only: refid_amd.png writes PNGs that its own reader -- and PIL, where it is installed -- decode to the same pixels."""
import os
import struct
import zlib

import numpy as np
import pytest

from refid_amd.png import SIGNATURE, read_chunks, read_png, write_png


def _img(shape, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, shape, dtype=np.uint8)


SHAPES = [(1, 1, 3), (17, 35, 3), (720, 1280, 3), (5, 7)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_round_trip(tmp_path, shape):
    x = _img(shape, 1)
    if x.ndim == 3 and x.shape[0] == 720:
        x[100:600] = x[99]                                  # (a photograph compresses; pure noise would only test zlib's stored blocks)
    path = write_png(str(tmp_path / "a.png"), x)
    y = read_png(path)
    assert y.dtype == np.uint8 and y.shape == x.shape and np.array_equal(x, y)


def test_chunk_layout_and_crcs(tmp_path):
    x = _img((17, 35, 3), 2)
    data = open(write_png(str(tmp_path / "a.png"), x), "rb").read()
    assert data[:8] == SIGNATURE
    chunks = read_chunks(data)                              # verifies every CRC
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert struct.unpack(">IIBBBBB", chunks[0][1]) == (35, 17, 8, 2, 0, 0, 0)
    pos = 8                                                 # and independently of read_chunks
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(data[pos + 4:pos + 8 + n]) & 0xffffffff
        pos += 12 + n
    assert pos == len(data)
    raw = zlib.decompress(chunks[1][1])
    assert len(raw) == 17 * (1 + 35 * 3) and not any(raw[r * 106] for r in range(17))      # filter type 0 on every row
    bad = bytearray(data)
    bad[40] ^= 1
    with pytest.raises(ValueError, match="CRC"):
        read_chunks(bytes(bad))


@pytest.mark.parametrize("shape", [(17, 35, 3), (5, 7)], ids=["rgb", "grey"])
def test_pil_decodes_the_same_pixels(tmp_path, shape):
    Image = pytest.importorskip("PIL.Image")
    x = _img(shape, 3)
    path = write_png(str(tmp_path / "a.png"), x)
    with Image.open(path) as im:
        assert im.mode == ("RGB" if x.ndim == 3 else "L")
        assert np.array_equal(np.asarray(im), x)


def test_parent_directory_is_created_and_bad_input_rejected(tmp_path):
    path = str(tmp_path / "a" / "b" / "c.png")
    write_png(path, _img((2, 3, 3), 4))
    assert os.path.isfile(path)
    for bad in (np.zeros((2, 3, 4), np.uint8), np.zeros((2, 3, 3), np.float32), np.zeros((0, 3, 3), np.uint8)):
        with pytest.raises(ValueError):
            write_png(str(tmp_path / "bad.png"), bad)
    assert not os.path.exists(tmp_path / "bad.png")


def test_level_changes_the_size_not_the_pixels(tmp_path):
    x = np.tile(np.arange(64, dtype=np.uint8).reshape(1, 64, 1), (48, 1, 3))
    a, b = write_png(str(tmp_path / "1.png"), x, level=1), write_png(str(tmp_path / "9.png"), x, level=9)
    assert np.array_equal(read_png(a), read_png(b)) and os.path.getsize(b) <= os.path.getsize(a)
