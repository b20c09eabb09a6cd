// The host stage of JPEG decode: marker parser and Huffman decoder of baseline files (what is accepted and refused:
// include/refid_hip.h).  Plain C++17, no HIP include: csrc/jpeg_decode.hip exports it, tools/jpeg_entropy_check.cpp builds
// it alone under the host sanitizers.  Every read of the file goes through a bounds check; the only writes are the caller's
// coefs / quant / info and the error text.  No allocation, no static state that is written: safe from several threads.
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/refid_hip.h"
#include "jpeg_tables.h"

namespace refid_jpeg {

constexpr int ERR_BYTES = 256;

struct Huff {
    bool defined;
    int32_t mincode[17], maxcode[17], valptr[17];              // per code length 1 .. 16 (maxcode -1: no code of that length)
    uint8_t vals[256];
    uint16_t look[1024];                                       // the next 10 bits -> (length << 8) | symbol, 0 = a longer code
};

struct Component {
    int id, h, v, tq, td, ta;
};

struct Header {
    int height, width, ncomp, sampling, restart;
    int mcu_rows, mcu_cols;
    Component comp[3];
    bool have_sof, adobe, quant_defined[4];
    int adobe_transform;
    uint16_t quant[4][64];                                     // natural order
    Huff dc[4], ac[4];
    size_t scan_at;                                            // the first byte of the entropy-coded data
};

inline int fail(char* err, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    int n = snprintf(err, ERR_BYTES, "jpeg_decode: ");
    vsnprintf(err + n, ERR_BYTES - n, fmt, ap);
    va_end(ap);
    return 1;
}

// canonical codes (T.81 Annex C) of `counts` codes per length and their symbols; false: more codes of a length than fit
inline bool huff_build(Huff* t, const uint8_t* counts, const uint8_t* symbols, int n_symbols) {
    memset(t, 0, sizeof(*t));
    int32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        t->mincode[len] = code, t->valptr[len] = k;
        const int n = counts[len - 1];
        if (code + n > (1 << len)) return false;
        if (len <= 10)
            for (int j = 0; j < n; ++j) {
                const int first = (code + j) << (10 - len);
                for (int f = 0; f < (1 << (10 - len)); ++f) t->look[first + f] = (uint16_t)((len << 8) | symbols[k + j]);
            }
        code += n, k += n;
        t->maxcode[len] = n ? code - 1 : -1;
        code <<= 1;
    }
    if (k != n_symbols) return false;
    memcpy(t->vals, symbols, (size_t)n_symbols);
    t->defined = true;
    return true;
}

inline void header_init(Header* h) {
    memset(h, 0, sizeof(*h));
    static const uint8_t dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    for (int c = 0; c < 2; ++c) {                              // Annex K until a DHT says otherwise
        huff_build(&h->dc[c], JPEG_DC_BITS[c], dc_vals, 12);
        huff_build(&h->ac[c], JPEG_AC_BITS[c], JPEG_AC_VALS[c], 162);
    }
}

inline const char* sof_name(int m) {
    switch (m) {
        case 0xc1: return "extended sequential (SOF1)";
        case 0xc2: return "progressive (SOF2)";
        case 0xc3: return "lossless (SOF3)";
        case 0xc5: case 0xc6: case 0xc7: return "hierarchical (SOF5 .. SOF7)";
        case 0xc9: case 0xca: case 0xcb: case 0xcd: case 0xce: case 0xcf: return "arithmetic coding (SOF9 .. SOF15)";
        default: return "unknown";
    }
}

// Walks the markers up to and including SOS.  0, or 1 with the message in err.
inline int parse_header(const uint8_t* file, size_t len, Header* h, char* err) {
    header_init(h);
    if (!file || len < 4 || file[0] != 0xff || file[1] != 0xd8) return fail(err, "no SOI marker at the start of the file");
    size_t pos = 2;
    for (;;) {
        if (pos >= len) return fail(err, "the file ends before SOS");
        if (file[pos] != 0xff) return fail(err, "a marker was expected at byte %zu, found %02X", pos, file[pos]);
        while (pos < len && file[pos] == 0xff) ++pos;          // FF fill bytes
        if (pos >= len) return fail(err, "the file ends before SOS");
        const int m = file[pos++];
        if (m == 0xd8 || m == 0x01 || (m >= 0xd0 && m <= 0xd7)) continue;      // stand-alone markers
        if (m == 0x00) return fail(err, "a marker was expected at byte %zu, found FF 00", pos - 2);
        if (m == 0xd9) return fail(err, "EOI before SOS");
        if (pos + 2 > len) return fail(err, "the file ends inside segment %02X", m);
        const size_t L = ((size_t)file[pos] << 8) | file[pos + 1];
        if (L < 2 || pos + L > len) return fail(err, "segment %02X of %zu bytes passes the end of the file", m, L);
        const uint8_t* s = file + pos + 2;
        const size_t n = L - 2;
        pos += L;
        if (m == 0xc0) {
            if (h->have_sof) return fail(err, "a second SOF0");
            if (n < 6) return fail(err, "SOF0 of %zu bytes is too short", n);
            if (s[0] != 8) return fail(err, "sample precision %d: only 8-bit files are decoded", s[0]);
            h->height = (s[1] << 8) | s[2], h->width = (s[3] << 8) | s[4], h->ncomp = s[5];
            if (h->height == 0 || h->width == 0) return fail(err, "dimensions of 0: height %d, width %d", h->height, h->width);
            if (h->ncomp != 1 && h->ncomp != 3) return fail(err, "%d components: only 1 (grey) or 3 (YCbCr) are decoded", h->ncomp);
            if (n != 6 + 3 * (size_t)h->ncomp) return fail(err, "SOF0 of %zu bytes for %d components", n, h->ncomp);
            for (int c = 0; c < h->ncomp; ++c) {
                Component& k = h->comp[c];
                k.id = s[6 + 3 * c], k.h = s[7 + 3 * c] >> 4, k.v = s[7 + 3 * c] & 15, k.tq = s[8 + 3 * c];
                if (k.h < 1 || k.h > 4 || k.v < 1 || k.v > 4) return fail(err, "component %d has sampling factors %dx%d", c, k.h, k.v);
                if (k.tq > 3) return fail(err, "component %d names quantisation table %d", c, k.tq);
            }
            if (h->ncomp == 1) {
                h->sampling = REFID_JPEG_DEC_GREY;
                h->comp[0].h = h->comp[0].v = 1;               // a one-component scan is not interleaved: the factors mean nothing
            } else {
                const Component* k = h->comp;
                if (k[0].id == 'R' && k[1].id == 'G' && k[2].id == 'B') return fail(err, "an RGB-coded file (component ids R G B)");
                const int hv = k[0].h * 16 + k[0].v;
                if (k[1].h != 1 || k[1].v != 1 || k[2].h != 1 || k[2].v != 1 || (hv != 0x11 && hv != 0x21 && hv != 0x22))
                    return fail(err, "sampling %dx%d %dx%d %dx%d: only luma 1x1, 2x1 or 2x2 with 1x1 chroma is decoded", k[0].h, k[0].v,
                                k[1].h, k[1].v, k[2].h, k[2].v);
                h->sampling = hv == 0x11 ? REFID_JPEG_DEC_444 : hv == 0x21 ? REFID_JPEG_DEC_422 : REFID_JPEG_DEC_420;
            }
            h->mcu_rows = (h->height + 8 * h->comp[0].v - 1) / (8 * h->comp[0].v);
            h->mcu_cols = (h->width + 8 * h->comp[0].h - 1) / (8 * h->comp[0].h);
            h->have_sof = true;
        } else if ((m >= 0xc1 && m <= 0xcf && m != 0xc4 && m != 0xc8 && m != 0xcc)) {
            return fail(err, "a %s frame: only baseline (SOF0) is decoded", sof_name(m));
        } else if (m == 0xcc) {
            return fail(err, "arithmetic coding (DAC) is not decoded");
        } else if (m == 0xdb) {
            size_t at = 0;
            while (at < n) {
                const int pq = s[at] >> 4, tq = s[at] & 15;
                if (pq == 1) return fail(err, "a 16-bit quantisation table");
                if (pq > 1 || tq > 3) return fail(err, "DQT names precision %d, table %d", pq, tq);
                if (at + 65 > n) return fail(err, "DQT passes the end of its segment");
                for (int k = 0; k < 64; ++k) h->quant[tq][JPEG_ZIGZAG[k]] = s[at + 1 + k];
                h->quant_defined[tq] = true;
                at += 65;
            }
        } else if (m == 0xc4) {
            size_t at = 0;
            while (at < n) {
                const int tc = s[at] >> 4, th = s[at] & 15;
                if (tc > 1 || th > 3) return fail(err, "DHT names class %d, table %d", tc, th);
                if (at + 17 > n) return fail(err, "DHT passes the end of its segment");
                int count = 0;
                for (int k = 0; k < 16; ++k) count += s[at + 1 + k];
                if (count > 256 || at + 17 + (size_t)count > n) return fail(err, "DHT with %d symbols passes the end of its segment", count);
                if (!huff_build(tc ? &h->ac[th] : &h->dc[th], s + at + 1, s + at + 17, count))
                    return fail(err, "DHT class %d table %d has more codes of a length than the length holds", tc, th);
                at += 17 + (size_t)count;
            }
        } else if (m == 0xdd) {
            if (n != 2) return fail(err, "DRI of %zu bytes", n);
            h->restart = (s[0] << 8) | s[1];
        } else if (m == 0xee) {
            if (n >= 12 && memcmp(s, "Adobe", 5) == 0) h->adobe = true, h->adobe_transform = s[11];
        } else if (m == 0xda) {
            if (!h->have_sof) return fail(err, "SOS before SOF0");
            if (n < 1) return fail(err, "SOS of %zu bytes is too short", n);
            const int ns = s[0];
            if (ns != h->ncomp) return fail(err, "a non-interleaved scan: %d of the frame's %d components", ns, h->ncomp);
            if (n != 4 + 2 * (size_t)ns) return fail(err, "SOS of %zu bytes for %d components", n, ns);
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != h->comp[c].id) return fail(err, "the scan's component %d is not the frame's", c);
                h->comp[c].td = s[2 + 2 * c] >> 4, h->comp[c].ta = s[2 + 2 * c] & 15;
                if (h->comp[c].td > 3 || h->comp[c].ta > 3) return fail(err, "component %d names Huffman tables %d / %d", c, h->comp[c].td, h->comp[c].ta);
                if (!h->dc[h->comp[c].td].defined || !h->ac[h->comp[c].ta].defined)
                    return fail(err, "component %d names a Huffman table that is not defined", c);
                if (!h->quant_defined[h->comp[c].tq]) return fail(err, "quantisation table %d is not defined", h->comp[c].tq);
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0)
                return fail(err, "a progressive scan (Ss %d, Se %d, AhAl %02X): only Ss 0, Se 63, 00 is decoded", s[1 + 2 * ns], s[2 + 2 * ns], s[3 + 2 * ns]);
            if (h->ncomp == 3 && h->adobe && h->adobe_transform == 0) return fail(err, "an RGB-coded file (Adobe transform 0)");
            h->scan_at = pos;
            return 0;
        }
        // APPn, COM and everything else: skipped
    }
}

inline void fill_info(const Header& h, refid_jpeg_info* info) {
    memset(info, 0, sizeof(*info));
    info->height = h.height, info->width = h.width, info->components = h.ncomp, info->sampling = h.sampling;
    for (int c = 0; c < h.ncomp; ++c) {
        info->blocks[c] = h.mcu_rows * h.comp[c].v * h.mcu_cols * h.comp[c].h;     // (<= 8192 * 8192 * 4 / 4 ... < 2^31)
        info->total_blocks += info->blocks[c];
    }
    info->restart_interval = h.restart;
}

// The entropy-coded bytes as bits, MSB first: FF 00 is a data byte FF, FF and anything else ends the segment.  acc holds
// the next n bits in its top bits; below them it is zero, so a look-ahead past the data reads zeros but take() refuses.
struct Bits {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc;
    int n;
    void fill() {
        while (n <= 56 && p < end) {
            unsigned b = *p;
            if (b == 0xff) {
                if (p + 1 >= end || p[1] != 0) break;          // a marker (or the file's last byte): the segment's data ends here
                p += 2;
            } else {
                ++p;
            }
            acc |= (uint64_t)b << (56 - n);
            n += 8;
        }
    }
    unsigned peek(int k) const { return (unsigned)(acc >> (64 - k)); }          // k 1 .. 32
    bool take(int k) {
        if (k > n) return false;
        acc <<= k, n -= k;
        return true;
    }
};

enum { OK = 0, SHORT = 1, BADCODE = 2 };

inline int huff_decode(Bits& b, const Huff& t, int* sym) {
    if (b.n < 16) b.fill();
    const unsigned e = t.look[b.peek(10)];
    if (e) {
        *sym = (int)(e & 255);
        return b.take((int)(e >> 8)) ? OK : SHORT;
    }
    const int32_t code = (int32_t)b.peek(16);
    for (int len = 11; len <= 16; ++len) {
        const int32_t c = code >> (16 - len);
        if (t.maxcode[len] >= 0 && c >= t.mincode[len] && c <= t.maxcode[len]) {
            *sym = t.vals[t.valptr[len] + (c - t.mincode[len])];
            return b.take(len) ? OK : SHORT;
        }
    }
    return b.n < 16 ? SHORT : BADCODE;                           // (with fewer than 16 real bits the zeros behind them may be what failed)
}

// s more bits as the signed value of category s (T.81 F.2.2.1); s 1 .. 11
inline bool receive_extend(Bits& b, int s, int* v) {
    if (b.n < s) b.fill();
    const int raw = (int)b.peek(s);
    if (!b.take(s)) return false;
    *v = raw < (1 << (s - 1)) ? raw - (1 << s) + 1 : raw;
    return true;
}

// One file's coefficients and tables (the layout: include/refid_hip.h).  0, or 1 with the message in err.
inline int entropy_decode(const uint8_t* file, size_t len, const refid_jpeg_info* expect, int16_t* coefs, uint16_t* quant, char* err) {
    if (!expect || !coefs || !quant) return fail(err, "%s is null", !expect ? "expect" : !coefs ? "coefs" : "quant");
    Header h;
    if (parse_header(file, len, &h, err)) return 1;
    refid_jpeg_info info;
    fill_info(h, &info);
    if (memcmp(&info, expect, sizeof(info)) != 0)
        return fail(err, "the file is %dx%d, %d components, sampling %d, %d blocks, restart interval %d; expected %dx%d, %d, %d, %d, %d",
                    info.height, info.width, info.components, info.sampling, info.total_blocks, info.restart_interval, expect->height,
                    expect->width, expect->components, expect->sampling, expect->total_blocks, expect->restart_interval);
    for (int c = 0; c < h.ncomp; ++c) memcpy(quant + 64 * c, h.quant[h.comp[c].tq], 64 * sizeof(uint16_t));
    long long base[3] = {0, info.blocks[0], (long long)info.blocks[0] + info.blocks[1]};
    Bits b = {file + h.scan_at, file + len, 0, 0};
    int pred[3] = {0, 0, 0};
    const long long mcus = (long long)h.mcu_rows * h.mcu_cols;
    static const char* const SHORT_MSG = "the entropy-coded data ends before the last MCU (MCU %lld of %lld)";
    for (long long m = 0; m < mcus; ++m) {
        if (h.restart && m && m % h.restart == 0) {
            const int want = (int)((m / h.restart - 1) & 7);
            if (b.n >= 8) return fail(err, "bytes are left over in front of RST%d (MCU %lld)", want, m);
            b.fill();                                          // (stops at the marker; what it adds would be left-over bytes)
            if (b.n >= 8) return fail(err, "bytes are left over in front of RST%d (MCU %lld)", want, m);
            b.acc = 0, b.n = 0;
            const uint8_t* p = b.p;
            if (p >= b.end) return fail(err, SHORT_MSG, m, mcus);
            while (p < b.end && *p == 0xff) ++p;               // (*b.p is FF here: fill() stopped there)
            if (p >= b.end) return fail(err, SHORT_MSG, m, mcus);
            if (*p != 0xd0 + want) return fail(err, "a wrong RST number: found marker %02X, expected RST%d (MCU %lld)", *p, want, m);
            b.p = p + 1;
            pred[0] = pred[1] = pred[2] = 0;
        }
        const long long my = m / h.mcu_cols, mx = m % h.mcu_cols;
        for (int c = 0; c < h.ncomp; ++c) {
            const Component& k = h.comp[c];
            const Huff& dc = h.dc[k.td];
            const Huff& ac = h.ac[k.ta];
            for (int by = 0; by < k.v; ++by)
                for (int bx = 0; bx < k.h; ++bx) {
                    int16_t* blk = coefs + 64 * (base[c] + (my * k.v + by) * ((long long)h.mcu_cols * k.h) + mx * k.h + bx);
                    memset(blk, 0, 64 * sizeof(int16_t));
                    int s = 0, v = 0;
                    int rc = huff_decode(b, dc, &s);
                    if (rc == SHORT) return fail(err, SHORT_MSG, m, mcus);
                    if (rc == BADCODE) return fail(err, "a Huffman code that is not in the DC table (MCU %lld)", m);
                    if (s > 11) return fail(err, "a DC category of %d, above 11 (MCU %lld)", s, m);
                    if (s) {
                        if (!receive_extend(b, s, &v)) return fail(err, SHORT_MSG, m, mcus);
                        pred[c] += v;
                    }
                    if (pred[c] < -32768 || pred[c] > 32767) return fail(err, "a DC value of %d leaves int16 (MCU %lld)", pred[c], m);
                    blk[0] = (int16_t)pred[c];
                    for (int i = 1; i < 64;) {
                        rc = huff_decode(b, ac, &s);
                        if (rc == SHORT) return fail(err, SHORT_MSG, m, mcus);
                        if (rc == BADCODE) return fail(err, "a Huffman code that is not in the AC table (MCU %lld)", m);
                        const int run = s >> 4;
                        s &= 15;
                        if (s == 0) {
                            if (run != 15) break;              // EOB
                            if (i + 16 > 64) return fail(err, "a zero run past coefficient 63 (MCU %lld)", m);
                            i += 16;
                            continue;
                        }
                        if (s > 10) return fail(err, "an AC category of %d, above 10 (MCU %lld)", s, m);
                        i += run;
                        if (i > 63) return fail(err, "a zero run past coefficient 63 (MCU %lld)", m);
                        if (!receive_extend(b, s, &v)) return fail(err, SHORT_MSG, m, mcus);
                        blk[JPEG_ZIGZAG[i]] = (int16_t)v;
                        ++i;
                    }
                }
        }
    }
    return 0;
}

inline int probe(const uint8_t* file, size_t len, refid_jpeg_info* info, char* err) {
    if (!info) return fail(err, "info is null");
    Header h;
    if (parse_header(file, len, &h, err)) return 1;
    fill_info(h, info);
    return 0;
}

}  // namespace refid_jpeg
