"""numpy restatement of the baseline JPEG stream of include/refid_hip.h (csrc/jpeg.hip): header, colour conversion, chroma
averaging, the integer DCT, quantisation, entropy coding, byte stuffing, restart markers, and the size functions.  Written
for clarity, not speed; integers only.  tests/test_jpeg_ref_host.py pins it against PIL and a float64 DCT before the GPU is
compared with it byte for byte."""
import math

import numpy as np

J444, J420 = 0, 1                      # == REFID_JPEG_444 / REFID_JPEG_420
SUBSAMPLINGS = {"444": J444, "420": J420}
HEADER_BYTES = 625                     # == REFID_JPEG_HEADER_BYTES
BLOCK_BITS = 1660                      # == REFID_JPEG_BLOCK_BITS: 11 + 11 for DC, 63 * (16 + 10) for AC
RECORD_BYTES = 16                      # scratch per segment in front of its parked bits

# ITU-T T.81 Annex K, tables K.1 and K.2, in natural (row-major) order
QUANT_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    dtype=np.int64)
QUANT_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32,
    dtype=np.int64)
# natural index of the k-th coefficient in zig-zag order
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# Annex K tables K.3 .. K.6: (counts of codes of length 1 .. 16, symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")))
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], list(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))
DHT_TABLES = ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA))      # (Tc << 4 | Th, table) in file order


def _round_half_away(x):
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


# T[u][k] = round(2^14 a(u) cos((2k+1) u pi / 16)), a(0) = sqrt(1/8), a(u) = 1/2
DCT_T = np.array([[_round_half_away(16384 * (math.sqrt(0.125) if u == 0 else 0.5) * math.cos((2 * k + 1) * u * math.pi / 16))
                   for k in range(8)] for u in range(8)], dtype=np.int64)
# what csrc/jpeg.hip holds: 8192 cos(n pi / 16) for n = 0 .. 8, rounded (and 5793 for the row u = 0)
DCT_COS = [8192, 8035, 7568, 6811, 5793, 4551, 3135, 1598, 0]


def _dct_entry(u, k):
    """T[u][k] from the nine constants, as the kernel folds the angle: cos is even, cos(pi - x) = -cos(x)."""
    if u == 0:
        return 5793
    n = (2 * k + 1) * u % 32
    n = 32 - n if n > 16 else n
    return DCT_COS[n] if n <= 8 else -DCT_COS[16 - n]


assert all(int(DCT_T[u][k]) == _dct_entry(u, k) for u in range(8) for k in range(8))


def huffman_codes(table):
    """{symbol: (code, length)} of a (counts, symbols) table: canonical codes, T.81 Annex C."""
    counts, symbols = table
    out, code, i = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[symbols[i]] = (code, length)
            code += 1
            i += 1
        code <<= 1
    return out


DC_CODES = (huffman_codes(DC_LUMA), huffman_codes(DC_CHROMA))
AC_CODES = (huffman_codes(AC_LUMA), huffman_codes(AC_CHROMA))


def quant_tables(quality):
    """int64 (2, 64), natural order: the Annex K tables scaled as libjpeg's jpeg_set_quality does."""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.stack([np.clip((base * s + 50) // 100, 1, 255) for base in (QUANT_LUMA, QUANT_CHROMA)])


def geometry(height, width, subsampling, restart_mcus=None):
    """(mcu size in pixels, MCU rows, MCU columns, blocks per MCU, MCUs per segment, segments)."""
    m = 16 if subsampling == J420 else 8
    rows, cols = -(-height // m), -(-width // m)
    restart = cols if not restart_mcus else restart_mcus
    return m, rows, cols, 6 if subsampling == J420 else 3, restart, -(-rows * cols // restart)


def _segment_blocks(height, width, subsampling, restart_mcus):
    m, rows, cols, bpm, restart, segs = geometry(height, width, subsampling, restart_mcus)
    return [min(restart, rows * cols - s * restart) * bpm for s in range(segs)]


def header_bytes():
    return HEADER_BYTES


def bound(height, width, subsampling, restart_mcus=None):
    blocks = _segment_blocks(height, width, subsampling, restart_mcus)
    return HEADER_BYTES + sum(2 * (-(-BLOCK_BITS * b // 8)) for b in blocks) + 2 * (len(blocks) - 1) + 2


def segment_stride(height, width, subsampling, restart_mcus=None):
    m, rows, cols, bpm, restart, segs = geometry(height, width, subsampling, restart_mcus)
    return (-(-BLOCK_BITS * min(restart, rows * cols) * bpm // 8) + 3) // 4 * 4      # room for the largest segment


def work_bytes(n_frames, height, width, subsampling, restart_mcus=None):
    segs = geometry(height, width, subsampling, restart_mcus)[5]
    return n_frames * segs * (RECORD_BYTES + segment_stride(height, width, subsampling, restart_mcus))


def default_pitch(height, width):
    return (HEADER_BYTES + 3 * height * width + 3) // 4 * 4


def header(height, width, quality, subsampling, restart_mcus=None):
    """The bytes in front of the first entropy-coded segment."""
    be16 = lambda v: bytes([v >> 8, v & 255])                                       # noqa: E731
    q = quant_tables(quality)
    out = b"\xff\xd8"
    out += b"\xff\xe0" + be16(16) + b"JFIF\x00" + bytes([1, 1, 0]) + be16(1) + be16(1) + bytes([0, 0])
    out += b"\xff\xdb" + be16(2 + 2 * 65) + b"".join(bytes([t]) + bytes(int(v) for v in q[t][ZIGZAG]) for t in (0, 1))
    hv = 0x22 if subsampling == J420 else 0x11
    out += b"\xff\xc0" + be16(17) + bytes([8]) + be16(height) + be16(width) + bytes([3, 1, hv, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc_th, (counts, symbols) in DHT_TABLES:
        out += b"\xff\xc4" + be16(2 + 1 + 16 + len(symbols)) + bytes([tc_th]) + bytes(counts) + bytes(symbols)
    out += b"\xff\xdd" + be16(4) + be16(geometry(height, width, subsampling, restart_mcus)[4])
    out += b"\xff\xda" + be16(12) + bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert len(out) == HEADER_BYTES
    return out


def ycc(frame):
    """int64 (3, H, W): Y, Cb, Cr of a uint8 (H, W, 3) RGB frame."""
    r, g, b = (frame[..., c].astype(np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16
    return np.stack([y, cb, cr])


def mcu_blocks(frame, subsampling):
    """int64 (MCUs, blocks per MCU, 8, 8): the samples (0 .. 255) of every block in stream order."""
    h, w = frame.shape[:2]
    m, rows, cols, bpm, _, _ = geometry(h, w, subsampling)
    planes = ycc(np.pad(frame, ((0, rows * m - h), (0, cols * m - w), (0, 0)), mode="edge"))
    if subsampling == J444:
        blocks = planes.reshape(3, rows, 8, cols, 8).transpose(1, 3, 0, 2, 4)
        return np.ascontiguousarray(blocks).reshape(rows * cols, 3, 8, 8)
    y = planes[0].reshape(rows, 2, 8, cols, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(rows * cols, 4, 8, 8)
    c = planes[1:].reshape(2, rows, 8, 2, cols, 8, 2)
    c = (c[:, :, :, 0, :, :, 0] + c[:, :, :, 0, :, :, 1] + c[:, :, :, 1, :, :, 0] + c[:, :, :, 1, :, :, 1] + 2) >> 2
    c = c.transpose(1, 3, 0, 2, 4).reshape(rows * cols, 2, 8, 8)
    return np.concatenate([y, c], axis=1)


def dct_scaled(samples):
    """int64 (..., 8, 8) [v][u]: 2^20 times the orthonormal DCT of the level-shifted (..., 8, 8) samples [y][x].  The DC term is
    exact (sum / 8), so that a flat block quantises as its mean does, ties included."""
    s = samples.astype(np.int64) - 128
    r = (np.einsum("...yk,uk->...yu", s, DCT_T) + 128) >> 8
    f = np.einsum("...ku,vk->...vu", r, DCT_T)
    f[..., 0, 0] = s.sum(axis=(-1, -2)) << 17
    return f


def quantise(scaled, quality, subsampling):
    """int64 (MCUs, blocks per MCU, 64) in zig-zag order."""
    q = quant_tables(quality)
    table = q[[0, 0, 0, 0, 1, 1] if subsampling == J420 else [0, 1, 1]].reshape(1, -1, 8, 8)
    out = np.sign(scaled) * (((np.abs(scaled) + (table << 19)) >> 20) // table)
    return out.reshape(out.shape[0], out.shape[1], 64)[..., ZIGZAG]


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, n):
        assert 0 <= value < (1 << n)
        self.acc, self.n = (self.acc << n) | value, self.n + n

    def bytes(self):
        pad = -self.n % 8
        return ((self.acc << pad) | ((1 << pad) - 1)).to_bytes((self.n + pad) // 8, "big")


def _category(v):
    cat = int(abs(v)).bit_length()
    return cat, (v if v >= 0 else v + (1 << cat) - 1)


def encode_block(bits, zz, pred, table, info):
    """One block's codes; zz: 64 quantised coefficients in zig-zag order; returns the new predictor."""
    dc = int(zz[0])
    cat, extra = _category(dc - pred)
    code, length = DC_CODES[table][cat]
    bits.put((code << cat) | extra, length + cat)
    info["dc_category"] = max(info.get("dc_category", 0), cat)
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bits.put(*AC_CODES[table][0xf0])
            info["zrl"] = info.get("zrl", 0) + 1
            run -= 16
        cat, extra = _category(v)
        code, length = AC_CODES[table][(run << 4) | cat]
        bits.put((code << cat) | extra, length + cat)
        info["ac_category"] = max(info.get("ac_category", 0), cat)
        run = 0
    if run:
        bits.put(*AC_CODES[table][0x00])
    else:
        info["no_eob"] = info.get("no_eob", 0) + 1
    return dc


def encode_coefficients(zz, height, width, quality, subsampling, restart_mcus=None, info=None):
    """bytes: the JFIF file of the quantised zig-zag coefficients (MCUs, blocks per MCU, 64)."""
    info = {} if info is None else info
    m, rows, cols, bpm, restart, segs = geometry(height, width, subsampling, restart_mcus)
    comp = [0, 0, 0, 0, 1, 2] if subsampling == J420 else [0, 1, 2]
    out = bytearray(header(height, width, quality, subsampling, restart_mcus))
    info["segments"] = segs
    for s in range(segs):
        if s:
            out += bytes([0xff, 0xd0 + (s - 1) % 8])
        bits, pred = _Bits(), [0, 0, 0]
        for mcu in range(s * restart, min((s + 1) * restart, rows * cols)):
            for j in range(bpm):
                pred[comp[j]] = encode_block(bits, zz[mcu, j], pred[comp[j]], 0 if comp[j] == 0 else 1, info)
        raw = bits.bytes()
        info["stuffed"] = info.get("stuffed", 0) + raw.count(b"\xff")
        out += raw.replace(b"\xff", b"\xff\x00")
    out += b"\xff\xd9"
    return bytes(out)


def encode(frame, quality=90, subsampling=J420, restart_mcus=None, info=None):
    """bytes: the JFIF file of a uint8 (H, W, 3) RGB frame."""
    h, w = frame.shape[:2]
    zz = quantise(dct_scaled(mcu_blocks(frame, subsampling)), quality, subsampling)
    return encode_coefficients(zz, h, w, quality, subsampling, restart_mcus, info)
