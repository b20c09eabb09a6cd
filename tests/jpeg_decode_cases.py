"""What the JPEG decode tests share: the golden cases (PIL-made files with PIL's pixels), seeded frames, a marker-level
editor and a builder of hand-made files for the refusals, and synthetic coefficients for the pixel stage."""
import functools
import os

import numpy as np

import jpeg_decode_ref as R
import jpeg_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_decode_cases.npz")
SAMPLINGS = ("grey", "444", "422", "420")
CODES = {"grey": R.GREY, "444": R.S444, "422": R.S422, "420": R.S420}


@functools.lru_cache(maxsize=None)
def golden():
    """{name: (file bytes, uint8 (H, W, 3) pixels as PIL decodes them)}."""
    with np.load(GOLDEN) as z:
        names = sorted(k[:-4] for k in z.files if k.endswith(".jpg"))
        return {n: (z[n + ".jpg"].tobytes(), z[n + ".rgb"]) for n in names}


def image(height, width, family, seed=0):
    if family == "noise":
        return np.random.default_rng(seed).integers(0, 256, (height, width, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:height, 0:width]
    return np.stack([(yy * 7 + xx * 3) % 256, (xx * 5 + 40) % 256, (yy * 2 + xx * 2 + 90) % 256], axis=-1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def own_files():
    """Files of tests/jpeg_ref.py's encoder (what csrc/jpeg.hip writes): 4:4:4 and 4:2:0, restart intervals None / 1 / 3."""
    return {f"own_{'444' if ss == J.J444 else '420'}_{h}x{w}_r{r}": J.encode(image(h, w, "noise", 7), 90, ss, r)
            for h, w in ((17, 35), (16, 16), (5, 3)) for ss in (J.J444, J.J420) for r in (None, 1, 3)}


# ---- a marker-level editor ---------------------------------------------------------------------------------------------

def split(data):
    """([(marker, payload)] up to and including SOS, the bytes behind the SOS segment) of a well-formed file."""
    segs, pos = [], 2
    while True:
        assert data[pos] == 0xff, pos
        marker, length = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        segs.append((marker, bytes(data[pos + 4:pos + 2 + length])))
        pos += 2 + length
        if marker == 0xda:
            return segs, bytes(data[pos:])


def join(segs, tail):
    out = bytearray(b"\xff\xd8")
    for marker, payload in segs:
        out += bytes([0xff, marker, (len(payload) + 2) >> 8, (len(payload) + 2) & 255]) + payload
    return bytes(out) + tail


def edit(data, marker, change, new_marker=None):
    """The file with ``change(payload)`` in place of the payload of every segment ``marker`` (and the marker renamed)."""
    segs, tail = split(data)
    return join([((new_marker or m) if m == marker else m, change(p) if m == marker else p) for m, p in segs], tail)


def strip_dht(data):
    segs, tail = split(data)
    return join([s for s in segs if s[0] != 0xc4], tail)


def put(payload, at, values):
    out = bytearray(payload)
    out[at:at + len(values)] = bytes(values)
    return bytes(out)


# ---- hand-made files ---------------------------------------------------------------------------------------------------

def pack_bits(bits):
    """A string of '0' / '1' -> entropy-coded bytes: padded with 1-bits, FF stuffed."""
    bits += "1" * (-len(bits) % 8)
    raw = bytes(int(bits[k:k + 8], 2) for k in range(0, len(bits), 8))
    return raw.replace(b"\xff", b"\xff\x00")


def dht(tc, th, symbols_by_length):
    """A DHT payload: {code length: [symbols]}."""
    counts = [len(symbols_by_length.get(k, [])) for k in range(1, 17)]
    return bytes([(tc << 4) | th]) + bytes(counts) + bytes(s for k in range(1, 17) for s in symbols_by_length.get(k, []))


def grey_file(height, width, dc_symbols, ac_symbols, bits, extra=()):
    """A one-component baseline file whose DC / AC tables hold ``dc_symbols`` / ``ac_symbols`` ({length: [symbols]}) and whose
    entropy-coded data is the bit string ``bits``."""
    segs = [(0xdb, bytes([0]) + bytes([1] * 64)), (0xc0, bytes([8, height >> 8, height & 255, width >> 8, width & 255, 1, 1, 0x11, 0])),
            (0xc4, dht(0, 0, dc_symbols)), (0xc4, dht(1, 0, ac_symbols)), *extra, (0xda, bytes([1, 1, 0x00, 0, 63, 0]))]
    return join(segs, pack_bits(bits) + b"\xff\xd9")


# ---- synthetic coefficients for the pixel stage ------------------------------------------------------------------------

FAMILIES = ("noise", "smooth", "zeros", "white", "extreme")


def coefficients(height, width, sampling, family, seed=0):
    """(coefs int16 (total_blocks, 64), quant uint16 (components, 64)) of one frame.  'noise' / 'smooth': a frame through
    tests/jpeg_ref.py's forward DCT, laid out per component plane; 'zeros' / 'white': all-0 / all-255 frames; 'extreme':
    coefficients of +-2047 (and a few smaller) with quantisers of 255: the clamp and the int32 wrap-around."""
    code = CODES[sampling]
    _, _, comps = R.geometry(height, width, code)
    total = sum(a * b for a, b in comps)
    rng = np.random.default_rng(seed)
    if family == "extreme":
        coefs = rng.choice(np.array([-2047, 2047, -2047, 2047, 0, 1, -1000], dtype=np.int16), size=(total, 64))
        return coefs, np.full((len(comps), 64), 255, dtype=np.uint16)
    if family in ("zeros", "white"):
        frame = np.full((height, width, 3), 0 if family == "zeros" else 255, dtype=np.uint8)
    else:
        frame = image(height, width, family, seed)
    hs, vs = R.LUMA_FACTORS[code]
    ycc = J.ycc(np.pad(frame, ((0, comps[0][0] * 8 - height), (0, comps[0][1] * 8 - width), (0, 0)), mode="edge"))
    quant = np.stack([J.quant_tables(90)[0 if c == 0 else 1] for c in range(len(comps))]).astype(np.uint16)
    out = []
    for c, (bh, bw) in enumerate(comps):
        plane = ycc[c]
        if c and (hs, vs) != (1, 1):
            plane = plane.reshape(bh * 8, vs, bw * 8, hs).sum(axis=(1, 3)) // (hs * vs)
        blocks = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(bh * bw, 8, 8)
        scaled = J.dct_scaled(blocks).reshape(-1, 64)
        q = quant[c].astype(np.int64)
        out.append(np.sign(scaled) * (((np.abs(scaled) + (q << 19)) >> 20) // q))
    return np.concatenate(out).astype(np.int16), quant
