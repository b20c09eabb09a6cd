"""numpy restatement of the baseline JPEG decoder of include/refid_hip.h (csrc/jpeg_entropy.h, csrc/jpeg_decode.hip): marker
parser, Huffman decoder, and the pixel stage -- dequantisation, libjpeg's islow IDCT, fancy upsampling, table-based colour
conversion -- in 32-bit two's complement with wrap-around (int64 wrapped after every operation: what np.int32 holds).
Written for clarity, not speed: the shapes are tiny.  tests/test_jpeg_decode_ref_host.py pins it against PIL (libjpeg-turbo) byte for byte before the library and the GPU are
compared with it."""
import collections

import numpy as np

import jpeg_ref as J

GREY, S444, S422, S420 = 0, 1, 2, 3        # == REFID_JPEG_DEC_*
SAMPLING_NAMES = {GREY: "grey", S444: "444", S422: "422", S420: "420"}
LUMA_FACTORS = {GREY: (1, 1), S444: (1, 1), S422: (2, 1), S420: (2, 2)}       # (h, v)

Info = collections.namedtuple("Info", "height width components sampling blocks total_blocks restart_interval")


class Refused(ValueError):
    pass


def geometry(height, width, sampling):
    """(MCU rows, MCU columns, [(blocks high, blocks wide)] per component) of the planes padded to whole MCUs."""
    h, v = LUMA_FACTORS[sampling]
    rows, cols = -(-height // (8 * v)), -(-width // (8 * h))
    comps = [(rows * v, cols * h)] + ([(rows, cols)] * 2 if sampling != GREY else [])
    return rows, cols, comps


def blocks_of(height, width, sampling):
    comps = geometry(height, width, sampling)[2]
    blocks = [a * b for a, b in comps] + [0] * (3 - len(comps))
    return blocks, sum(blocks)


class _Huff:
    """Canonical codes (T.81 Annex C) of (counts per length 1 .. 16, symbols in code order): {(length, code): symbol}."""

    def __init__(self, counts, symbols):
        self.codes, code, k = {}, 0, 0
        for length in range(1, 17):
            if code + counts[length - 1] > (1 << length):
                raise Refused("DHT: more codes of a length than the length holds")
            for _ in range(counts[length - 1]):
                self.codes[(length, code)] = symbols[k]
                code, k = code + 1, k + 1
            code <<= 1


def parse(data):
    """The header up to SOS: a dict with height, width, comps [(id, h, v, tq, td, ta)], sampling, restart, quant {tq: int
    array (64,) natural order}, dc / ac {th: _Huff}, scan_at.  Raises Refused for what include/refid_hip.h lists."""
    data = bytes(data)
    if len(data) < 4 or data[:2] != b"\xff\xd8":
        raise Refused("no SOI marker")
    h = dict(quant={}, restart=0, adobe=None, comps=None,
             dc={0: _Huff(*J.DC_LUMA), 1: _Huff(*J.DC_CHROMA)}, ac={0: _Huff(*J.AC_LUMA), 1: _Huff(*J.AC_CHROMA)})
    pos = 2
    while True:
        if pos >= len(data):
            raise Refused("the file ends before SOS")
        if data[pos] != 0xff:
            raise Refused(f"a marker was expected at byte {pos}")
        while pos < len(data) and data[pos] == 0xff:
            pos += 1
        if pos >= len(data):
            raise Refused("the file ends before SOS")
        m = data[pos]
        pos += 1
        if m in (0xd8, 0x01) or 0xd0 <= m <= 0xd7:
            continue
        if m == 0x00:
            raise Refused("a marker was expected, found FF 00")
        if m == 0xd9:
            raise Refused("EOI before SOS")
        if pos + 2 > len(data):
            raise Refused("the file ends inside a segment")
        length = (data[pos] << 8) | data[pos + 1]
        if length < 2 or pos + length > len(data):
            raise Refused("a segment passes the end of the file")
        s = data[pos + 2:pos + length]
        pos += length
        if m == 0xc0:
            if h["comps"] is not None:
                raise Refused("a second SOF0")
            if len(s) < 6:
                raise Refused("SOF0 is too short")
            if s[0] != 8:
                raise Refused(f"sample precision {s[0]}")
            h["height"], h["width"], n = (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
            if h["height"] == 0 or h["width"] == 0:
                raise Refused("dimensions of 0")
            if n not in (1, 3):
                raise Refused(f"{n} components")
            if len(s) != 6 + 3 * n:
                raise Refused("SOF0 has the wrong length")
            comps = [[s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c], 0, 0] for c in range(n)]
            for c in comps:
                if not (1 <= c[1] <= 4 and 1 <= c[2] <= 4) or c[3] > 3:
                    raise Refused("a bad component")
            if n == 1:
                comps[0][1] = comps[0][2] = 1
                h["sampling"] = GREY
            else:
                if [c[0] for c in comps] == [ord("R"), ord("G"), ord("B")]:
                    raise Refused("an RGB-coded file (component ids R G B)")
                hv = [(c[1], c[2]) for c in comps]
                if hv[1:] != [(1, 1), (1, 1)] or hv[0] not in ((1, 1), (2, 1), (2, 2)):
                    raise Refused(f"sampling {hv}")
                h["sampling"] = {(1, 1): S444, (2, 1): S422, (2, 2): S420}[hv[0]]
            h["comps"] = comps
        elif 0xc1 <= m <= 0xcf and m not in (0xc4, 0xc8, 0xcc):
            raise Refused(f"SOF{m - 0xc0}: only baseline (SOF0)")
        elif m == 0xcc:
            raise Refused("arithmetic coding (DAC)")
        elif m == 0xdb:
            at = 0
            while at < len(s):
                pq, tq = s[at] >> 4, s[at] & 15
                if pq == 1:
                    raise Refused("a 16-bit quantisation table")
                if pq > 1 or tq > 3 or at + 65 > len(s):
                    raise Refused("a bad DQT")
                q = np.zeros(64, dtype=np.int64)
                q[J.ZIGZAG] = list(s[at + 1:at + 65])
                h["quant"][tq] = q
                at += 65
        elif m == 0xc4:
            at = 0
            while at < len(s):
                tc, th = s[at] >> 4, s[at] & 15
                if tc > 1 or th > 3 or at + 17 > len(s):
                    raise Refused("a bad DHT")
                counts = list(s[at + 1:at + 17])
                if sum(counts) > 256 or at + 17 + sum(counts) > len(s):
                    raise Refused("DHT passes the end of its segment")
                h["ac" if tc else "dc"][th] = _Huff(counts, list(s[at + 17:at + 17 + sum(counts)]))
                at += 17 + sum(counts)
        elif m == 0xdd:
            if len(s) != 2:
                raise Refused("a bad DRI")
            h["restart"] = (s[0] << 8) | s[1]
        elif m == 0xee:
            if len(s) >= 12 and s[:5] == b"Adobe":
                h["adobe"] = s[11]
        elif m == 0xda:
            comps = h["comps"]
            if comps is None:
                raise Refused("SOS before SOF0")
            if len(s) < 1 or s[0] != len(comps):
                raise Refused("a non-interleaved scan")
            if len(s) != 4 + 2 * len(comps):
                raise Refused("SOS has the wrong length")
            for c, comp in enumerate(comps):
                if s[1 + 2 * c] != comp[0]:
                    raise Refused("the scan's components are not the frame's")
                comp[4], comp[5] = s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15
                if comp[4] not in h["dc"] or comp[5] not in h["ac"]:
                    raise Refused("a Huffman table that is not defined")
                if comp[3] not in h["quant"]:
                    raise Refused("a quantisation table that is not defined")
            if tuple(s[1 + 2 * len(comps):]) != (0, 63, 0):
                raise Refused("a progressive scan")
            if len(comps) == 3 and h["adobe"] == 0:
                raise Refused("an RGB-coded file (Adobe transform 0)")
            h["scan_at"] = pos
            return h


def probe(data):
    h = parse(data)
    blocks, total = blocks_of(h["height"], h["width"], h["sampling"])
    return Info(h["height"], h["width"], len(h["comps"]), SAMPLING_NAMES[h["sampling"]], tuple(blocks), total, h["restart"])


class _Bits:
    """The bits of one entropy-coded segment: FF 00 is a data byte FF; the segment ends at FF followed by anything else."""

    def __init__(self, data, pos):
        self.data, self.pos, self.acc, self.n = data, pos, 0, 0

    def _more(self):
        d, p = self.data, self.pos
        if p >= len(d):
            return False
        b = d[p]
        if b == 0xff:
            if p + 1 >= len(d) or d[p + 1] != 0:
                return False
            p += 1
        self.pos, self.acc, self.n = p + 1, (self.acc << 8) | b, self.n + 8
        return True

    def get(self, k):
        while self.n < k:
            if not self._more():
                raise Refused("the entropy-coded data ends before the last MCU")
        self.n -= k
        v = (self.acc >> self.n) & ((1 << k) - 1)
        self.acc &= (1 << self.n) - 1
        return v

    def symbol(self, table, what):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.get(1)
            if (length, code) in table.codes:
                return table.codes[(length, code)]
        raise Refused(f"a Huffman code that is not in the {what} table")

    def restart(self, want):
        if self.n >= 8 or self._more():                     # (a byte that _more() can still take lies in front of the marker)
            raise Refused("bytes are left over in front of RST")
        d, p = self.data, self.pos
        while p < len(d) and d[p] == 0xff:
            p += 1
        if p >= len(d):
            raise Refused("the entropy-coded data ends before the last MCU")
        if d[p] != 0xd0 + want:
            raise Refused("a wrong RST number")
        self.pos, self.acc, self.n = p + 1, 0, 0


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def entropy_decode(data):
    """(Info, coefs int16 (total_blocks, 64), quant uint16 (components, 64)) in the layout of include/refid_hip.h."""
    data = bytes(data)
    h = parse(data)
    info = probe(data)
    rows, cols, planes = geometry(h["height"], h["width"], h["sampling"])
    comps = h["comps"]
    base = np.concatenate([[0], np.cumsum(info.blocks)])
    coefs = np.zeros((info.total_blocks, 64), dtype=np.int16)
    quant = np.stack([h["quant"][c[3]] for c in comps]).astype(np.uint16)
    bits, pred = _Bits(data, h["scan_at"]), [0] * len(comps)
    for m in range(rows * cols):
        if h["restart"] and m and m % h["restart"] == 0:
            bits.restart((m // h["restart"] - 1) & 7)
            pred = [0] * len(comps)
        my, mx = divmod(m, cols)
        for c, (_, ch, cv, _, td, ta) in enumerate(comps):
            for by in range(cv):
                for bx in range(ch):
                    blk = coefs[base[c] + (my * cv + by) * planes[c][1] + mx * ch + bx]
                    s = bits.symbol(h["dc"][td], "DC")
                    if s > 11:
                        raise Refused("a DC category above 11")
                    if s:
                        pred[c] += _extend(bits.get(s), s)
                    if not -32768 <= pred[c] <= 32767:
                        raise Refused("a DC value leaves int16")
                    blk[0] = pred[c]
                    i = 1
                    while i < 64:
                        rs = bits.symbol(h["ac"][ta], "AC")
                        run, s = rs >> 4, rs & 15
                        if s == 0:
                            if run != 15:
                                break
                            if i + 16 > 64:
                                raise Refused("a zero run past coefficient 63")
                            i += 16
                            continue
                        if s > 10:
                            raise Refused("an AC category above 10")
                        i += run
                        if i > 63:
                            raise Refused("a zero run past coefficient 63")
                        blk[J.ZIGZAG[i]] = _extend(bits.get(s), s)
                        i += 1
    return info, coefs, quant


# ---- the pixel stage -------------------------------------------------------------------------------------------------

def _wrap(x):
    """int64 -> the value a 32-bit two's complement register holds."""
    return ((np.asarray(x, dtype=np.int64) + (1 << 31)) % (1 << 32)) - (1 << 31)


def _idct8(v, shift):
    """libjpeg's jpeg_idct_islow on the last axis (8 values), every operation wrapped to int32; descaled by ``shift``."""
    w = _wrap
    i0, i1, i2, i3, i4, i5, i6, i7 = (v[..., k].astype(np.int64) for k in range(8))
    z1 = w(w(i2 + i6) * 4433)
    tmp2 = w(z1 + w(i6 * -15137))
    tmp3 = w(z1 + w(i2 * 6270))
    tmp0 = w(w(i0 + i4) << 13)
    tmp1 = w(w(i0 - i4) << 13)
    tmp10, tmp13, tmp11, tmp12 = w(tmp0 + tmp3), w(tmp0 - tmp3), w(tmp1 + tmp2), w(tmp1 - tmp2)
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = w(t0 + t3), w(t1 + t2), w(t0 + t2), w(t1 + t3)
    z5 = w(w(z3 + z4) * 9633)
    t0, t1, t2, t3 = w(t0 * 2446), w(t1 * 16819), w(t2 * 25172), w(t3 * 12299)
    z1, z2, z3, z4 = w(z1 * -7373), w(z2 * -20995), w(z3 * -16069), w(z4 * -3196)
    z3, z4 = w(z3 + z5), w(z4 + z5)
    t0, t1, t2, t3 = w(t0 + w(z1 + z3)), w(t1 + w(z2 + z4)), w(t2 + w(z2 + z3)), w(t3 + w(z1 + z4))
    half = 1 << (shift - 1)
    d = lambda x: w(x + half) >> shift                                              # noqa: E731  (arithmetic shift)
    return np.stack([d(w(tmp10 + t3)), d(w(tmp11 + t2)), d(w(tmp12 + t1)), d(w(tmp13 + t0)),
                     d(w(tmp13 - t0)), d(w(tmp12 - t1)), d(w(tmp11 - t2)), d(w(tmp10 - t3))], axis=-1)


def idct_blocks(coefs, q):
    """uint8-valued int64 (B, 8, 8) samples of int16 (B, 64) coefficients under the table q (64,), natural order."""
    x = _wrap(coefs.astype(np.int64) * np.asarray(q, dtype=np.int64)).reshape(-1, 8, 8)
    cols = _idct8(x.transpose(0, 2, 1), 11).transpose(0, 2, 1)                      # along each column first
    return np.clip(_idct8(cols, 18) + 128, 0, 255)


def planes_of(coefs, quant, height, width, sampling):
    """The component planes cropped to ceil(H v / vmax) x ceil(W h / hmax): [int64 (h_c, w_c)]."""
    hs, vs = LUMA_FACTORS[sampling]
    _, _, comps = geometry(height, width, sampling)
    out, at = [], 0
    for c, (bh, bw) in enumerate(comps):
        s = idct_blocks(coefs[at:at + bh * bw], quant[c]).reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
        at += bh * bw
        ph, pw = (height, width) if c == 0 else (-(-height // vs), -(-width // hs))
        out.append(s[:ph, :pw])
    return out


def _h2v1(s):
    """(rows, w) -> (rows, 2w): libjpeg's h2v1_fancy_upsample."""
    left, right = np.concatenate([s[:, :1], s[:, :-1]], axis=1), np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((s.shape[0], 2 * s.shape[1]), dtype=np.int64)
    out[:, 0::2] = (3 * s + left + 1) >> 2
    out[:, 1::2] = (3 * s + right + 2) >> 2
    out[:, 0], out[:, -1] = s[:, 0], s[:, -1]
    return out


def _h2v2(s):
    """(h, w) -> (2h, 2w): libjpeg's h2v2_fancy_upsample, the row above / below an edge row being the edge row."""
    above, below = np.concatenate([s[:1], s[:-1]]), np.concatenate([s[1:], s[-1:]])
    out = np.empty((2 * s.shape[0], 2 * s.shape[1]), dtype=np.int64)
    for v, far in ((0, above), (1, below)):
        t = 3 * s + far
        left, right = np.concatenate([t[:, :1], t[:, :-1]], axis=1), np.concatenate([t[:, 1:], t[:, -1:]], axis=1)
        row = np.empty((s.shape[0], 2 * s.shape[1]), dtype=np.int64)
        row[:, 0::2] = (3 * t + left + 8) >> 4
        row[:, 1::2] = (3 * t + right + 7) >> 4
        row[:, 0], row[:, -1] = (4 * t[:, 0] + 8) >> 4, (4 * t[:, -1] + 7) >> 4
        out[v::2] = row
    return out


def upsample(s, height, width, sampling):
    hs, vs = LUMA_FACTORS[sampling]
    if hs == 1:
        return s
    if s.shape[1] <= 2:                                                             # narrow planes: plain replication
        s = np.repeat(np.repeat(s, vs, axis=0), 2, axis=1)
    else:
        s = _h2v1(s) if vs == 1 else _h2v2(s)
    return s[:height, :width]


def _fix(x):
    return int(x * 65536 + 0.5)


def colour(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def pixels(coefs, quant, height, width, sampling):
    """uint8 (H, W, 3) of one frame's coefficients int16 (total_blocks, 64) and tables (components, 64)."""
    planes = planes_of(np.asarray(coefs), np.asarray(quant), height, width, sampling)
    if sampling == GREY:
        return np.repeat(planes[0][:, :, None], 3, axis=2).astype(np.uint8)
    return colour(planes[0], upsample(planes[1], height, width, sampling), upsample(planes[2], height, width, sampling))


def decode(data):
    """uint8 (H, W, 3) of a JPEG byte string."""
    info, coefs, quant = entropy_decode(data)
    return pixels(coefs, quant, info.height, info.width, {v: k for k, v in SAMPLING_NAMES.items()}[info.sampling])
