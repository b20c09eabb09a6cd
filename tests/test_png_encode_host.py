"""CPU-only: png.encode_png_rows / write_png_rows, the host half of the filtered PNG route -- rows filtered by
tests/png_filter_ref.py (pinned to read_png and PIL by test_png_filter_ref_host.py) go through every deflate strategy and
decode to the image with the project's reader and with PIL; encode_png keeps its bytes; wrong row counts are rejected."""
import io
import struct
import zlib

import numpy as np
import pytest

import png_filter_ref as R
from refid_amd import png

STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "rle": zlib.Z_RLE, "huffman": zlib.Z_HUFFMAN_ONLY}


def _image(h, w, seed):
    """Smooth content, an edge and a little noise: the adaptive choice uses several filter types."""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:h, 0:w]
    base = 120 + 60 * np.sin(xx / 5.0) + 40 * np.cos(yy / 3.0) + 50 * (xx > w // 2)
    img = base[:, :, None] + np.array([0.0, 15.0, -20.0]) + rng.normal(0, 2.0, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (17, 35), (40, 56)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("strategy", sorted(STRATEGIES))
def test_filtered_rows_decode_to_the_image(tmp_path, shape, strategy):
    h, w = shape
    img = _image(h, w, 3)
    types = R.adaptive_types(img)
    if h >= 17:
        assert len(set(types.tolist())) >= 2
    rows = R.apply_filters(img, types)
    data = png.encode_png_rows(rows, w, h, strategy=STRATEGIES[strategy])
    chunks = png.read_chunks(data)
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert chunks[0][1] == struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)
    assert zlib.decompress(chunks[1][1]) == rows.tobytes()
    path = png.write_png_rows(str(tmp_path / "sub" / "a.png"), rows, w, h, strategy=STRATEGIES[strategy])
    assert open(path, "rb").read() == data
    got = png.read_png(path)
    assert got.dtype == np.uint8 and got.shape == img.shape and np.array_equal(got, img)
    _, _, ch, back = png.read_filtered(path)
    assert ch == 3 and np.array_equal(back, rows)
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(io.BytesIO(data)) as pil:
        assert pil.mode == "RGB" and np.array_equal(np.asarray(pil), img)


def test_the_default_strategy_and_rows_flat_or_batched():
    """Level 1 and Z_HUFFMAN_ONLY: the strategy that tools/bench_png_encode.py measured faster and smaller than Z_RLE."""
    img = _image(9, 11, 4)
    rows = R.apply_filters(img, R.adaptive_types(img))
    want = png.encode_png_rows(rows, 11, 9, 1, zlib.Z_HUFFMAN_ONLY)
    flat = np.zeros((9, 1 + 3 * 11), dtype=np.uint8)              # runs: where the two strategies differ
    assert png.encode_png_rows(flat, 11, 9) == png.encode_png_rows(flat, 11, 9, 1, zlib.Z_HUFFMAN_ONLY)
    assert png.encode_png_rows(flat, 11, 9) != png.encode_png_rows(flat, 11, 9, 1, zlib.Z_RLE)
    assert png.encode_png_rows(rows, 11, 9) == want
    assert png.encode_png_rows(rows.reshape(-1), 11, 9) == want
    assert png.encode_png_rows(rows[::1][None], 11, 9) == want


def test_encode_png_keeps_its_bytes():
    """encode_png / write_png: filter 0 on every row, one zlib.compress at the given level -- stated here from scratch."""
    for img in (_image(17, 35, 5), _image(5, 4, 6)[:, :, 0]):
        h, w = img.shape[:2]
        rows0 = np.zeros((h, 1 + img.size // h), dtype=np.uint8)
        rows0[:, 1:] = img.reshape(h, -1)
        for level in (1, 6):
            chunk = lambda tag, d: struct.pack(">I", len(d)) + tag + d + struct.pack(">I", zlib.crc32(tag + d) & 0xffffffff)   # noqa: E731
            want = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if img.ndim == 3 else 0, 0, 0, 0)) +
                    chunk(b"IDAT", zlib.compress(rows0.tobytes(), level)) + chunk(b"IEND", b""))
            assert png.encode_png(img, level) == want
    assert png.encode_png(_image(17, 35, 5)) == png.encode_png(_image(17, 35, 5), 1)


def test_rows_of_the_wrong_length_are_rejected():
    rows = R.apply_filters(_image(4, 5, 7), np.zeros(4, dtype=np.int64))
    for bad, w, h in ((rows[:, :-1], 5, 4), (rows[:-1], 5, 4), (rows, 4, 5), (rows, 5, 0), (rows, 0, 4), (rows.astype(np.int32), 5, 4)):
        with pytest.raises(ValueError, match="write_png_rows"):
            png.encode_png_rows(bad, w, h)


def test_the_command_lines_take_the_flag_then_the_yaml_key(tmp_path):
    """--png-filter, else val.png_filter of --opt, else none; a bad value of the key ends the command line by name."""
    import argparse
    from refid_amd import deblur, interpolate
    from test_sequence_host import TEST_YAML
    assert deblur.png_filter_setting is interpolate.png_filter_setting
    keyed, bad, plain = tmp_path / "k.yml", tmp_path / "b.yml", tmp_path / "p.yml"
    keyed.write_text(TEST_YAML + "\nval:\n  png_filter: adaptive\n")
    bad.write_text(TEST_YAML + "\nval:\n  png_filter: best\n")
    plain.write_text(TEST_YAML)
    setting = lambda flag, opt: interpolate.png_filter_setting(argparse.Namespace(png_filter=flag, opt=opt and str(opt)))   # noqa: E731
    assert setting(None, None) == "none" and setting(None, plain) == "none" and setting(None, keyed) == "adaptive"
    assert setting("none", keyed) == "none" and setting("adaptive", plain) == "adaptive"
    with pytest.raises(SystemExit, match="val.png_filter: 'best'"):
        setting(None, bad)
