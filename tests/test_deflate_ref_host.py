"""CPU-only: tests/deflate_ref.py (the stream format of refid_png_deflate) pinned to zlib's inflate, to the project's PNG
reader and to PIL before the GPU test compares the kernel with it byte for byte.  Every comparison is exact equality."""
import io
import zlib

import numpy as np
import pytest

import deflate_cases as K
import deflate_ref as D
from refid_amd import png

# Size of the restatement's stream over zlib's own Huffman-only deflate (level 1) on the adaptive rows of 256x256 frames of
# the nine families, at the default block size: the ratios measured with this file on the CPU, each
# with the 0.01 that zlib builds may differ by in their block boundaries.
SIZE_BARS = {"zeros": 1.0346, "all255": 1.0340, "noise": 0.9999, "hramp": 1.0338, "vramp": 1.0331, "diagonal": 1.0146,
             "waves": 1.0145, "checker": 1.0229, "blocks": 1.0090}


@pytest.mark.parametrize("block_bytes", K.BLOCKS)
@pytest.mark.parametrize("case", K.CASES)
def test_zlib_inflates_every_stream_and_the_segments_add_up(case, block_bytes):
    data = K.streams(case)
    outs, infos = K.expected(case, block_bytes)
    for k, (stream, info) in enumerate(zip(outs, infos)):
        raw = data[k].tobytes()
        assert zlib.decompress(stream) == raw, k
        inflater = zlib.decompressobj()
        assert inflater.decompress(stream) == raw and inflater.eof and inflater.unused_data == b"", k
        assert stream[:2] == b"\x78\x01" and stream[-9:-4] == b"\x01\x00\x00\xff\xff"
        assert int.from_bytes(stream[-4:], "big") == zlib.adler32(raw) == D.adler32(data[k]), k
        assert len(info) == D.n_blocks(len(raw), block_bytes)
        assert sum(r["bytes"] for r in info) == len(raw)
        assert 2 + sum(r["length"] for r in info) + 9 == len(stream) <= D.bound(len(raw), block_bytes)
        at = 2
        for r in info:
            # every segment starts at a byte and ends with the empty stored block's 00 00 FF FF (dynamic) or with its bytes
            assert r["offset"] == at
            seg = stream[at:at + r["length"]]
            if r["stored"]:
                n = r["bytes"]
                assert seg[:5] == bytes([0, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255]) and len(seg) == n + 5
            else:
                assert seg[-4:] == b"\x00\x00\xff\xff" and len(seg) == r["dynamic_bytes"] < r["bytes"] + 5
                assert r["kraft"] == 1 << D.MAX_BITS and r["max_length"] <= D.MAX_BITS
            at += r["length"]


def test_a_segment_inflates_on_its_own():
    """Segments are independent: a raw inflate of one segment plus the terminator gives that block's bytes."""
    data = K.streams("17x35")[6]
    info = []
    stream = D.deflate(data, 257, info)
    for j, r in enumerate(info):
        seg = stream[r["offset"]:r["offset"] + r["length"]] + b"\x01\x00\x00\xff\xff"
        assert zlib.decompressobj(-15).decompress(seg) == data[257 * j:257 * j + 257].tobytes(), j


def test_header_fields_are_parsed_back():
    data = K.streams("65x33")[K.FAMILIES.index("waves")]
    info = []
    stream = D.deflate(data, 4096, info)
    seen = 0
    for j, r in enumerate(info):
        if r["stored"]:
            continue
        seen += 1
        block = data[4096 * j:4096 * j + 4096]
        freq = np.bincount(block, minlength=257)
        freq[256] = 1
        hlit, hdist, hclen, cl, lengths = D.parse_dynamic_header(stream[r["offset"]:r["offset"] + r["length"]])
        assert (hlit, hdist, hclen) == (0, 0, 15)
        assert cl == [4] * 16 + [0, 0, 0]
        assert len(lengths) == 258 and lengths[257] == 0
        assert lengths[:257] == D.code_lengths(freq).tolist()
        assert all((n > 0) == (f > 0) for n, f in zip(lengths[:257], freq))
    assert seen >= 2
    assert D.HEADER_BITS == 1106


def test_the_code_is_the_documented_one_on_small_examples():
    """Worked by hand: two symbols get one bit each; 1, 1, 2, 4 gives 3, 3, 2, 1 (ties: lower symbol first in the sort, and
    the canonical numbering gives the lower symbol the lower code); a chain past 15 is repaired to a complete code."""
    f = np.zeros(257, dtype=np.int64)
    f[0], f[256] = 9, 1
    assert D.code_lengths(f)[[0, 256]].tolist() == [1, 1] and D.canonical_codes(D.code_lengths(f))[[0, 256]].tolist() == [0, 1]
    f = np.zeros(257, dtype=np.int64)
    f[10], f[20], f[30], f[256] = 4, 2, 1, 1
    lengths = D.code_lengths(f)
    assert lengths[[10, 20, 30, 256]].tolist() == [1, 2, 3, 3]
    assert D.canonical_codes(lengths)[[10, 20, 30, 256]].tolist() == [0b0, 0b10, 0b110, 0b111]
    f = np.zeros(257, dtype=np.int64)
    fib = [1, 2]
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    f[:17], f[256] = fib, 1
    info = {}
    lengths = D.code_lengths(f, info)
    assert info["overflow"] > 0 and lengths.max() == 15 and int((1 << (15 - lengths[lengths > 0])).sum()) == 1 << 15
    assert (np.diff(lengths[:17]) <= 0).all()                   # the more frequent, the shorter


def test_the_inputs_reach_every_path():
    """From the restatement's own counters, over the cases and block sizes the GPU test runs."""
    seen = dict(stored=0, dynamic=0, repaired=0, two_symbols=0, all_symbols=0, one_byte=0, one_block=0, short_last=0, mid_row=0)
    for case in K.CASES:
        data = K.streams(case)
        pitch = 1 + 3 * int(case.split("x")[1]) if "x" in case else None
        for block_bytes in K.BLOCKS:
            for info in K.expected(case, block_bytes)[1]:
                seen["one_block"] += len(info) == 1
                seen["short_last"] += len(info) > 1 and info[-1]["bytes"] < block_bytes
                if pitch and len(info) > 1:
                    seen["mid_row"] += any((j * block_bytes) % pitch for j in range(1, len(info)))
                for r in info:
                    seen["stored"] += r["stored"]
                    seen["dynamic"] += not r["stored"]
                    seen["one_byte"] += r["bytes"] == 1
                    if not r.get("short"):
                        seen["repaired"] += r["overflow"] > 0 and not r["stored"]
                        seen["two_symbols"] += r["symbols"] == 2 and r["max_length"] == 1 and not r["stored"]
                        seen["all_symbols"] += r["symbols"] == 257 and not r["stored"]
        assert data.shape[1] >= 1
    print(seen)
    assert all(v >= 1 for v in seen.values()), seen


@pytest.mark.parametrize("shape", [(1, 1), (17, 35), (65, 33)], ids=lambda s: "x".join(map(str, s)))
def test_the_wrapped_png_decodes_to_the_frame(tmp_path, shape):
    h, w = shape
    frames = K.frames_of(h, w)
    for k, stream in enumerate(K.expected(f"{h}x{w}", D.DEFAULT_BLOCK_BYTES)[0]):
        data = png.wrap_zlib_stream(stream, w, h)
        assert data == png.wrap_zlib_stream(np.frombuffer(stream, dtype=np.uint8), w, h)
        assert [t for t, _ in png.read_chunks(data)] == [b"IHDR", b"IDAT", b"IEND"] and png.read_chunks(data)[1][1] == stream
        path = png.write_png_stream(str(tmp_path / "sub" / f"{k}.png"), stream, w, h)
        assert open(path, "rb").read() == data
        assert np.array_equal(png.read_png(path), frames[k]), K.FAMILIES[k]
        try:
            from PIL import Image
        except ImportError:
            continue
        with Image.open(io.BytesIO(data)) as pil:
            assert pil.mode == "RGB" and np.array_equal(np.asarray(pil), frames[k]), K.FAMILIES[k]
    for bad in (b"", b"\x78\x9c" + bytes(20), stream[:5]):
        with pytest.raises(ValueError, match="write_png_stream"):
            png.wrap_zlib_stream(bad, w, h)
    with pytest.raises(ValueError, match="write_png_stream"):
        png.wrap_zlib_stream(stream, 0, h)


def test_the_existing_encoders_keep_their_bytes():
    img = K.frames_of(17, 35)[6]
    rows = K.adaptive_rows(img)
    chunk = png._chunk
    ihdr = chunk(b"IHDR", (35).to_bytes(4, "big") + (17).to_bytes(4, "big") + bytes([8, 2, 0, 0, 0]))
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
    idat = c.compress(rows.tobytes()) + c.flush()
    assert png.encode_png_rows(rows, 35, 17) == png.SIGNATURE + ihdr + chunk(b"IDAT", idat) + chunk(b"IEND", b"")
    rows0 = np.zeros_like(rows)
    rows0[:, 1:] = img.reshape(17, -1)
    assert png.encode_png(img) == png.SIGNATURE + ihdr + chunk(b"IDAT", zlib.compress(rows0.tobytes(), 1)) + chunk(b"IEND", b"")


@pytest.mark.parametrize("family", K.FAMILIES)
def test_size_against_zlib_huffman_only(family):
    rng = np.random.Generator(np.random.PCG64(7))
    img = K._frame(family, 256, 256, rng)
    rows = K.adaptive_rows(img)
    stream = D.deflate(rows, D.DEFAULT_BLOCK_BYTES)
    assert zlib.decompress(stream) == rows.tobytes()
    ratio = len(stream) / len(D.zlib_huffman_only(rows))
    print(family, f"{ratio:.4f}")
    assert ratio <= SIZE_BARS[family] + 0.01, (family, ratio)


def test_the_command_lines_take_the_flag_then_the_yaml_key(tmp_path):
    """--png-deflate, else val.png_deflate of --opt, else host; a bad value of the key ends the command line by name."""
    import argparse
    from refid_amd import deblur, interpolate, validation
    from test_sequence_host import TEST_YAML
    assert deblur.png_deflate_setting is interpolate.png_deflate_setting
    assert validation.PNG_DEFLATES == ("host", "device") and validation.PNG_FILTERS == ("none", "adaptive")
    keyed, bad, plain = tmp_path / "k.yml", tmp_path / "b.yml", tmp_path / "p.yml"
    keyed.write_text(TEST_YAML + "\nval:\n  png_deflate: device\n")
    bad.write_text(TEST_YAML + "\nval:\n  png_deflate: gpu\n")
    plain.write_text(TEST_YAML)
    setting = lambda flag, opt: interpolate.png_deflate_setting(argparse.Namespace(png_deflate=flag, opt=opt and str(opt)))   # noqa: E731
    assert setting(None, None) == "host" and setting(None, plain) == "host" and setting(None, keyed) == "device"
    assert setting("host", keyed) == "host" and setting("device", plain) == "device"
    with pytest.raises(SystemExit, match="val.png_deflate: 'gpu'"):
        setting(None, bad)
    ap = interpolate.parser("x", "doc", "o", "f", "s")
    common = ["--frames", "f", "--events", "e", "--stamps", "s", "--out", "o"]
    assert ap.parse_args(common).png_deflate is None and ap.parse_args([*common, "--png-deflate", "device"]).png_deflate == "device"
    with pytest.raises(SystemExit):
        ap.parse_args([*common, "--png-deflate", "gpu"])
    assert validation.check_png_deflate(None) == "host" and validation.check_png_deflate("device") == "device"
