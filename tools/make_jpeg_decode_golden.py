"""Writes tests/golden/jpeg_decode_cases.npz: a dozen small JPEG files made by PIL (libjpeg-turbo) together with the pixels
PIL decodes from them, so that the GPU tests of JPEG decode are pinned to libjpeg without needing PIL.  Every sampling,
optimised Huffman tables, restart markers, a file with its DHT segments stripped (decoded with the Annex K tables, as
Motion-JPEG cameras write them) and widths 3 .. 5 (the narrow-chroma rule).  Seeded: a rerun with the same PIL gives the
same file.

    python tools/make_jpeg_decode_golden.py
"""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "jpeg_decode_cases.npz")
PIL_SUBSAMPLING = {"444": 0, "422": 1, "420": 2}

# (name, height, width, family, sampling, save options, strip DHT)
CASES = [
    ("s420_17x35_q90", 17, 35, "noise", "420", dict(quality=90), False),
    ("s420_33x65_q30_rst3", 33, 65, "smooth", "420", dict(quality=30, restart_marker_blocks=3), False),
    ("s420_37x53_opt", 37, 53, "smooth", "420", dict(quality=75, optimize=True), False),
    ("s420_16x16_nodht", 16, 16, "noise", "420", dict(quality=90), True),
    ("s420_5x3", 5, 3, "noise", "420", dict(quality=90), False),
    ("s420_9x4", 9, 4, "noise", "420", dict(quality=90), False),
    ("s420_8x5", 8, 5, "noise", "420", dict(quality=90), False),
    ("s422_17x35_q90", 17, 35, "noise", "422", dict(quality=90), False),
    ("s422_7x9_rst1", 7, 9, "smooth", "422", dict(quality=90, restart_marker_blocks=1), False),
    ("s422_9x4_opt", 9, 4, "noise", "422", dict(quality=100, optimize=True), False),
    ("s444_16x16_q100", 16, 16, "noise", "444", dict(quality=100), False),
    ("s444_5x3_opt", 5, 3, "smooth", "444", dict(quality=30, optimize=True), False),
    ("grey_17x35_q90", 17, 35, "noise", "grey", dict(quality=90), False),
    ("grey_20x6_opt_rst1", 20, 6, "smooth", "grey", dict(quality=75, optimize=True, restart_marker_blocks=1), False),
]


def image(height, width, family, seed):
    if family == "noise":
        return np.random.default_rng(seed).integers(0, 256, (height, width, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:height, 0:width]
    return np.stack([(yy * 7 + xx * 3) % 256, (xx * 5 + 40) % 256, (yy * 2 + xx * 2 + 90) % 256], axis=-1).astype(np.uint8)


def strip_dht(data):
    """The file without its DHT segments (walks the markers up to SOS)."""
    out, pos = bytearray(data[:2]), 2
    while True:
        assert data[pos] == 0xff
        marker, length = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        if marker != 0xc4:
            out += data[pos:pos + 2 + length]
        pos += 2 + length
        if marker == 0xda:
            return bytes(out + data[pos:])


def pil_encode(img, sampling, **options):
    from PIL import Image
    buf = io.BytesIO()
    if sampling == "grey":
        Image.fromarray(img).convert("L").save(buf, "JPEG", **options)
    else:
        Image.fromarray(img).save(buf, "JPEG", subsampling=PIL_SUBSAMPLING[sampling], **options)
    return buf.getvalue()


def pil_decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im.convert("RGB"))


def main():
    arrays = {}
    for k, (name, h, w, family, sampling, options, no_dht) in enumerate(CASES):
        data = pil_encode(image(h, w, family, 100 + k), sampling, **options)
        if no_dht:
            data = strip_dht(data)
        arrays[name + ".jpg"] = np.frombuffer(data, dtype=np.uint8)
        arrays[name + ".rgb"] = pil_decode(data)
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    print(f"{OUT}: {len(CASES)} cases, {size} bytes")
    assert size < 64 * 1024, size
    return 0


if __name__ == "__main__":
    sys.exit(main())
