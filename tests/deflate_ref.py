"""The stream format of refid_png_deflate (csrc/png_deflate.hip), restated in numpy for the tests and tools: one zlib stream
per frame from its filtered rows, Huffman codes only (no matches), one code per block of ``block_bytes`` input bytes.

Stream:   78 01 | segment of block 0 | segment of block 1 | ... | 01 00 00 FF FF (final empty stored block) | Adler-32, big-endian
Every segment is byte-aligned, so the blocks are encoded independently and laid end to end.

Dynamic segment (RFC 1951 3.2.7), bits packed from the least significant bit of each byte:
  BFINAL 0, BTYPE 10 | HLIT 0 (257 literal/length codes), HDIST 0 (one distance code), HCLEN 15 (19 entries)
  | the 19 code-length-code lengths in the RFC's order: 0 for the symbols 16, 17, 18, 4 for 0..15 -- a complete fixed code
    in which the 4-bit code of a length IS that length, and no run-length symbol exists
  | 257 literal/length code lengths and one distance length of 0, each as that 4-bit code       (1106 header bits in all)
  | the block's bytes as canonical Huffman codes, most significant code bit first (RFC 1951 3.1.1) | the end-of-block code
  | an empty stored block: 000, padding to the next byte, 00 00 FF FF   (the sync marker; it byte-aligns the segment)
Stored segment: 00 | LEN, ~LEN little-endian | the bytes.  Used exactly when the dynamic segment would take >= len + 5 bytes.

The code of a block:
  - frequencies of its bytes, and 1 for end-of-block (symbol 256); at least two symbols always occur;
  - the symbols that occur, sorted by (frequency, symbol), are the leaves; n - 1 merges with two queues (leaves, merged
    nodes in order of creation), each taking the two least heads, the LEAF queue winning a tie;
  - depths from the root down, node by node in reverse order of creation, each one more than its parent's CLAMPED depth;
    a depth above 15 becomes 15 and counts as an overflow, for merged nodes too (zlib's gen_bitlen);
  - with overflows, zlib's repair on the 16 counts of leaves per length: while overflow > 0, the longest length below 15
    that has a leaf gives one leaf up as a parent of two at the next length, one of them taken from length 15;
  - the counts are dealt out longest first over the leaves in sorted order (the rarest symbol gets the longest code);
  - canonical code values (RFC 1951 3.2.2).  The code is complete: sum 2^-length == 1."""
import zlib

import numpy as np

MAX_BITS = 15
MAX_BLOCK = 65535
DEFAULT_BLOCK_BYTES = 32768          # == REFID_PNG_DEFLATE_BLOCK in include/refid_hip.h (the size table)
RECORD_BYTES = 1088                  # == REFID_PNG_DEFLATE_RECORD: scratch per block (segment length, Adler sums, 257 codes)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
HEADER_BITS = 3 + 5 + 5 + 4 + 19 * 3 + 258 * 4
ADLER = 65521


def n_blocks(stream_bytes, block_bytes):
    return -(-int(stream_bytes) // int(block_bytes))


def bound(stream_bytes, block_bytes):
    """The largest stream: every block stored."""
    return 2 + int(stream_bytes) + 5 * n_blocks(stream_bytes, block_bytes) + 9


def work_bytes(n_streams, stream_bytes, block_bytes):
    return int(n_streams) * n_blocks(stream_bytes, block_bytes) * RECORD_BYTES


def code_lengths(freq, info=None):
    """int (257,) code lengths of the frequencies ``freq`` (257,), by the construction of the module docstring."""
    freq = [int(v) for v in freq]
    leaves = sorted((f, s) for s, f in enumerate(freq) if f)
    n = len(leaves)
    assert n >= 2 and len(freq) == 257
    node_freq = [f for f, _ in leaves] + [0] * (n - 1)
    parent = [0] * (2 * n - 1)
    leaf, merged, nxt = 0, n, n
    for _ in range(n - 1):
        pick = []
        for _ in range(2):
            if leaf < n and (merged >= nxt or node_freq[leaf] <= node_freq[merged]):
                pick.append(leaf)
                leaf += 1
            else:
                pick.append(merged)
                merged += 1
        node_freq[nxt] = node_freq[pick[0]] + node_freq[pick[1]]
        parent[pick[0]] = parent[pick[1]] = nxt
        nxt += 1
    depth = [0] * (2 * n - 1)
    count = [0] * (MAX_BITS + 1)
    overflow = 0
    for i in range(2 * n - 3, -1, -1):
        d = depth[parent[i]] + 1
        if d > MAX_BITS:
            d, overflow = MAX_BITS, overflow + 1
        depth[i] = d
        if i < n:
            count[d] += 1
    if info is not None:
        info.update(symbols=n, overflow=overflow)
    while overflow > 0:
        bits = MAX_BITS - 1
        while count[bits] == 0:
            bits -= 1
        count[bits] -= 1
        count[bits + 1] += 2
        count[MAX_BITS] -= 1
        overflow -= 2
    lengths = np.zeros(257, dtype=np.int64)
    k = 0
    for bits in range(MAX_BITS, 0, -1):
        for _ in range(count[bits]):
            lengths[leaves[k][1]] = bits
            k += 1
    assert k == n and sum(c << (MAX_BITS - b) for b, c in enumerate(count) if b) == 1 << MAX_BITS, count
    return lengths


def canonical_codes(lengths):
    """int (257,) code values of RFC 1951 3.2.2 (most significant bit first) for the lengths."""
    lengths = np.asarray(lengths, dtype=np.int64)
    count = np.bincount(lengths, minlength=MAX_BITS + 2)
    count[0] = 0
    nxt, code = [0] * (MAX_BITS + 2), 0
    for bits in range(1, MAX_BITS + 1):
        code = (code + int(count[bits - 1])) << 1
        nxt[bits] = code
    codes = np.zeros(len(lengths), dtype=np.int64)
    for s, ln in enumerate(lengths.tolist()):
        if ln:
            codes[s] = nxt[ln]
            nxt[ln] += 1
    return codes


def _reverse(codes, lengths):
    out = np.zeros_like(codes)
    for j in range(MAX_BITS):
        out |= ((codes >> j) & 1) << np.maximum(lengths - 1 - j, 0)
    return np.where(lengths > 0, out, 0)


def _put(bits, pos, values, widths):
    """ORs ``values`` (least significant bit first, ``widths`` bits each) into the bit array at positions ``pos``."""
    values, widths, pos = np.asarray(values, dtype=np.int64), np.asarray(widths, dtype=np.int64), np.asarray(pos, dtype=np.int64)
    for j in range(int(widths.max(initial=0))):
        m = widths > j
        bits[pos[m] + j] |= ((values[m] >> j) & 1).astype(np.uint8)


def header_bits(lengths):
    """uint8 (1106,) bits of a dynamic segment's header for the 257 code lengths."""
    bits = np.zeros(HEADER_BITS, dtype=np.uint8)
    cl = [0 if s >= 16 else 4 for s in CL_ORDER]
    fields = [(0, 1), (2, 2), (0, 5), (0, 5), (15, 4)] + [(v, 3) for v in cl]
    # a 4-bit code-length code is the length itself, as a Huffman code: most significant bit first
    fields += [(int(f"{int(v):04b}"[::-1], 2), 4) for v in list(lengths) + [0]]
    pos = np.cumsum([0] + [w for _, w in fields[:-1]])
    _put(bits, pos, [v for v, _ in fields], [w for _, w in fields])
    assert pos[-1] + 4 == HEADER_BITS
    return bits


def encode_block(data, info=None):
    """bytes of the segment of one block ``data`` (uint8, 1 .. 65535 of them)."""
    data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    n = data.size
    assert 1 <= n <= MAX_BLOCK
    info = {} if info is None else info
    if (HEADER_BITS + n + 1 + 3 + 7) // 8 + 4 >= n + 5:
        # every code has at least one bit, so the dynamic segment cannot be shorter than this: stored whatever the code is
        # (blocks of up to 158 bytes; the code is not built, which keeps tests with tiny blocks quick)
        info.update(bytes=n, stored=True, short=True)
        return bytes([0, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255]) + data.tobytes()
    freq = np.bincount(data, minlength=257)
    freq[256] = 1
    lengths = code_lengths(freq, info)
    rev = _reverse(canonical_codes(lengths), lengths)
    body = int((freq * lengths).sum())
    total = HEADER_BITS + body + 3
    dyn_bytes = (total + 7) // 8 + 4
    info.update(bytes=n, max_length=int(lengths.max()), stored=dyn_bytes >= n + 5, dynamic_bytes=dyn_bytes,
                kraft=int((1 << (MAX_BITS - lengths[lengths > 0])).sum()))
    if info["stored"]:
        return bytes([0, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255]) + data.tobytes()
    bits = np.zeros(8 * (dyn_bytes - 4), dtype=np.uint8)
    bits[:HEADER_BITS] = header_bits(lengths)
    widths = lengths[data]
    pos = HEADER_BITS + np.concatenate(([0], np.cumsum(widths)))
    _put(bits, pos[:-1], rev[data], widths)
    _put(bits, pos[-1:], rev[256:257], lengths[256:257])
    return np.packbits(bits, bitorder="little").tobytes() + b"\x00\x00\xff\xff"


def deflate(rows, block_bytes=DEFAULT_BLOCK_BYTES, info=None):
    """The zlib stream (bytes) of the uint8 array ``rows`` (any shape, taken flat).  ``info``: a list that receives one dict
    per block (bytes, stored, symbols, overflow, max_length, dynamic_bytes, kraft, offset, length)."""
    data = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1)
    block_bytes = int(block_bytes)
    assert data.size >= 1 and 1 <= block_bytes <= MAX_BLOCK
    out = [b"\x78\x01"]
    offset = 2
    for start in range(0, data.size, block_bytes):
        rec = {}
        seg = encode_block(data[start:start + block_bytes], rec)
        rec.update(offset=offset, length=len(seg))
        offset += len(seg)
        out.append(seg)
        if info is not None:
            info.append(rec)
    out.append(b"\x01\x00\x00\xff\xff" + adler32(data).to_bytes(4, "big"))
    stream = b"".join(out)
    assert len(stream) <= bound(data.size, block_bytes)
    return stream


def adler32(data, block_bytes=4096):
    """Adler-32 the way the kernels take it: per block A = sum d_i and B = sum (len - i) d_i modulo 65521, then combined in
    block order: b += len * a + B, a += A."""
    data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    a, b = 1, 0
    for start in range(0, data.size, block_bytes):
        d = data[start:start + block_bytes].astype(np.int64)
        ln = d.size
        b = (b + ln * a + int((d * (ln - np.arange(ln))).sum())) % ADLER
        a = (a + int(d.sum())) % ADLER
    return (b << 16) | a


def parse_dynamic_header(segment):
    """(hlit, hdist, hclen, [19 code-length-code lengths by symbol], [258 lengths]) read back from a dynamic segment."""
    bits = np.unpackbits(np.frombuffer(segment[:(HEADER_BITS + 7) // 8], dtype=np.uint8), bitorder="little")
    take = lambda p, w: int((bits[p:p + w] << np.arange(w)).sum())          # noqa: E731
    assert take(0, 1) == 0 and take(1, 2) == 2
    hlit, hdist, hclen = take(3, 5), take(8, 5), take(13, 4)
    cl = [0] * 19
    for k in range(hclen + 4):
        cl[CL_ORDER[k]] = take(17 + 3 * k, 3)
    p = 17 + 3 * (hclen + 4)
    lengths = [int("".join(map(str, bits[p + 4 * k:p + 4 * k + 4])), 2) for k in range(hlit + 257 + hdist + 1)]
    return hlit, hdist, hclen, cl, lengths


def zlib_huffman_only(rows):
    """The stream zlib's own Huffman-only deflate (level 1) gives for the same bytes: the size yardstick."""
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
    return c.compress(np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1).data) + c.flush()
