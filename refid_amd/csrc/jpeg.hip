// Baseline JPEG frames for Motion-JPEG video: one JFIF file per frame, cut by restart markers into byte-aligned segments
// that are coded independently and laid end to end.  The stream is stated in include/refid_hip.h and restated in
// tests/jpeg_ref.py.
//
// Three launches that meet only at the kernel boundaries; no workgroup waits for another, nothing spins, every loop count
// is known before the loop starts.
//   jpeg_code_kernel     one workgroup per segment, one lane per 8x8 block, JPEG_BLOCKS blocks per pass.  A lane converts
//     its block's pixels (clamped coordinates: the replicated edge), averages chroma, runs the two integer DCT passes in
//     registers, quantises and leaves the 64 zig-zag coefficients in LDS.  The DC predictor is the DC of the lane 1, 3 or
//     6 places before (the last eight of a pass are carried to the next).  A first walk over the coefficients adds up the
//     block's bits, a workgroup prefix sum gives its bit position, a second walk puts the codes MSB first into the LDS
//     image of bit_image.h (writer, retire step and their barrier contract are stated there).  The sink byte-swaps a
//     complete word, counts its FF bytes and parks it in the segment's room in `work` (aligned dword stores).  The
//     segment's record gets its length before and after stuffing.
//   jpeg_offsets_kernel  one workgroup per frame.  Exclusive sum of the stuffed lengths (+2 for each RSTm) into the records
//     (the chunk walk of bit_image.h), then, if the file fits the pitch, the header (a kernel argument, built on the
//     host), EOI and lens; else lens = -need.
//   jpeg_place_kernel    one workgroup per segment.  RSTm, then the parked bytes with 00 after every FF: a lane takes 16
//     consecutive bytes, a workgroup prefix sum of 1 + (byte == FF) gives its place, bytes are stored one by one (out has
//     no alignment).  No global atomics, no read-modify-write of a global word; nothing outside the segment's bytes is
//     written.
// The scan is that of workgroup.h.
#include "common.h"
#include "bit_image.h"
#include "jpeg_tables.h"
#include <initializer_list>

namespace {

constexpr int JPEG_BLOCKS = 128;                               // threads of the code kernel = blocks per pass
constexpr int JPEG_THREADS = 256;                              // threads of the other two kernels
constexpr int JPEG_REC = 4;                                    // words of a segment's record in `work`
constexpr int JPEG_REC_RAW = 0, JPEG_REC_STUFFED = 1, JPEG_REC_OFF = 2, JPEG_REC_FITS = 3;
constexpr int JPEG_IMAGE = (31 + JPEG_BLOCKS * REFID_JPEG_BLOCK_BITS + 31) / 32 + 2;      // words: carried bits + a pass at its worst
constexpr int JPEG_PER_THREAD = 16;
constexpr int JPEG_PASS = JPEG_THREADS * JPEG_PER_THREAD;      // parked bytes per pass of the place kernel

// what the kernels look up: (length << 16) | code per symbol, canonical codes (T.81 Annex C); the zig-zag position of a
// natural index
struct JpegTables {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
    uint8_t zz_pos[64];
};
constexpr JpegTables jpeg_make_tables() {
    JpegTables t = {};
    for (int c = 0; c < 2; ++c) {
        uint32_t code = 0;
        int i = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int n = 0; n < JPEG_DC_BITS[c][len - 1]; ++n) t.dc[c][i++] = ((uint32_t)len << 16) | code++;    // (symbol i is category i)
            code <<= 1;
        }
        code = 0, i = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int n = 0; n < JPEG_AC_BITS[c][len - 1]; ++n) t.ac[c][JPEG_AC_VALS[c][i++]] = ((uint32_t)len << 16) | code++;
            code <<= 1;
        }
    }
    for (int k = 0; k < 64; ++k) t.zz_pos[JPEG_ZIGZAG[k]] = (uint8_t)k;
    return t;
}
__constant__ JpegTables jpeg_tables = jpeg_make_tables();

// T[u][k] = round(2^14 a(u) cos((2k+1) u pi / 16)) from 8192 cos(n pi / 16), n = 0 .. 8: cos is even, cos(pi - x) = -cos(x)
constexpr int jpeg_cos(int n) {
    return n == 0 ? 8192 : n == 1 ? 8035 : n == 2 ? 7568 : n == 3 ? 6811 : n == 4 ? 5793 : n == 5 ? 4551 : n == 6 ? 3135 : n == 7 ? 1598 : 0;
}
constexpr int jpeg_t(int u, int k) {
    if (u == 0) return 5793;
    int n = (2 * k + 1) * u % 32;
    n = n > 16 ? 32 - n : n;
    return n <= 8 ? jpeg_cos(n) : -jpeg_cos(16 - n);
}
template <int U>
__device__ __forceinline__ int jpeg_dot(const int* s) {
    constexpr int t0 = jpeg_t(U, 0), t1 = jpeg_t(U, 1), t2 = jpeg_t(U, 2), t3 = jpeg_t(U, 3), t4 = jpeg_t(U, 4), t5 = jpeg_t(U, 5),
                  t6 = jpeg_t(U, 6), t7 = jpeg_t(U, 7);
    return s[0] * t0 + s[1] * t1 + s[2] * t2 + s[3] * t3 + s[4] * t4 + s[5] * t5 + s[6] * t6 + s[7] * t7;
}
__device__ __forceinline__ void jpeg_dct8(const int* s, int* o) {
    o[0] = jpeg_dot<0>(s), o[1] = jpeg_dot<1>(s), o[2] = jpeg_dot<2>(s), o[3] = jpeg_dot<3>(s);
    o[4] = jpeg_dot<4>(s), o[5] = jpeg_dot<5>(s), o[6] = jpeg_dot<6>(s), o[7] = jpeg_dot<7>(s);
}

struct JpegGeom {
    int n_frames, height, width, subsampling;
    int mcu, rows, cols, bpm, restart, segs;                   // MCU size in pixels, MCU rows / columns, blocks per MCU, MCUs per segment
    int seg_stride;                                            // bytes of a segment's room in `work` (a multiple of 4)
    int out_pitch;
    long long bound;
};
struct JpegQuant { uint8_t q[2][64]; };                        // zig-zag order, as in DQT
struct JpegHeader { uint8_t b[(REFID_JPEG_HEADER_BYTES + 3) / 4 * 4]; };

constexpr RefidBitOrder JPEG_ORDER = REFID_BITS_MSB_FIRST;     // T.81: the most significant bit of a code comes first

__device__ __forceinline__ unsigned jpeg_category(int v) { return 32u - (unsigned)__clz(v < 0 ? -v : v); }    // (__clz(0) = 32)
__device__ __forceinline__ unsigned jpeg_ff_bytes(unsigned v) {
    return ((v & 0xffu) == 0xffu) + ((v & 0xff00u) == 0xff00u) + ((v & 0xff0000u) == 0xff0000u) + ((v >> 24) == 0xffu);
}

// One component of pixel (y, x) of the extended frame: the clamp replicates the last column and row
__device__ __forceinline__ int jpeg_component(const uint8_t* frame, int y, int x, int height, int width, int cr, int cg, int cb, int add) {
    const uint8_t* p = frame + ((long long)min(y, height - 1) * width + min(x, width - 1)) * 3;
    return (cr * (int)p[0] + cg * (int)p[1] + cb * (int)p[2] + add) >> 16;
}

__global__ __launch_bounds__(JPEG_BLOCKS) void jpeg_code_kernel(const uint8_t* __restrict__ frames, unsigned* __restrict__ work,
                                                                const JpegGeom g, const JpegQuant quant) {
    __shared__ short coef[64][JPEG_BLOCKS];
    __shared__ int dcs[8 + JPEG_BLOCKS];
    __shared__ unsigned image[JPEG_IMAGE];
    __shared__ unsigned hdc[2][16], hac[2][256], qt[2][64];
    __shared__ unsigned red[JPEG_BLOCKS / 64];
    const int tid = threadIdx.x;
    const int f = blockIdx.x / g.segs, s = blockIdx.x % g.segs;
    const int mcu0 = s * g.restart;                            // (< rows * cols <= 2^26)
    const int n_blocks = min(g.restart, g.rows * g.cols - mcu0) * g.bpm;
    const uint8_t* frame = frames + (long long)f * g.height * g.width * 3;
    unsigned* rec = work + (long long)blockIdx.x * JPEG_REC;
    unsigned* parked = work + (long long)g.n_frames * g.segs * JPEG_REC + (long long)blockIdx.x * (g.seg_stride / 4);

    for (int i = tid; i < 2 * 16; i += JPEG_BLOCKS) (&hdc[0][0])[i] = (&jpeg_tables.dc[0][0])[i];
    for (int i = tid; i < 2 * 256; i += JPEG_BLOCKS) (&hac[0][0])[i] = (&jpeg_tables.ac[0][0])[i];
    for (int i = tid; i < 2 * 64; i += JPEG_BLOCKS) (&qt[0][0])[i] = (&quant.q[0][0])[i];
    for (int i = tid; i < JPEG_IMAGE; i += JPEG_BLOCKS) image[i] = 0;
    if (tid < 8) dcs[tid] = 0;

    const bool s420 = g.subsampling == REFID_JPEG_420;
    unsigned cursor = 0;                                       // bits of the segment so far
    int w0 = 0;                                                // the word of the segment that image[0] stands for
    unsigned ff = 0;                                           // FF bytes among the words this thread parked
    const int passes = (n_blocks + JPEG_BLOCKS - 1) / JPEG_BLOCKS;
    for (int pass = 0; pass < passes; ++pass) {
        __syncthreads();                                       // the tables; the image, dcs[0..8) and coef of the pass before
        const int b = pass * JPEG_BLOCKS + tid;
        const bool active = b < n_blocks;
        const int j = b % g.bpm;
        const int comp = s420 ? max(j - 3, 0) : j;             // 0 Y, 1 Cb, 2 Cr
        const int tbl = comp ? 1 : 0;
        if (active) {
            const int mcu = mcu0 + b / g.bpm;
            const int my = mcu / g.cols, mx = mcu % g.cols;
            const int step = s420 && comp ? 2 : 1;             // pixels per sample
            const int y0 = my * g.mcu + (s420 && !comp ? 8 * (j >> 1) : 0), x0 = mx * g.mcu + (s420 && !comp ? 8 * (j & 1) : 0);
            const int cr = comp == 0 ? 19595 : comp == 1 ? -11059 : 32768;
            const int cg = comp == 0 ? 38470 : comp == 1 ? -21709 : -27439;
            const int cb = comp == 0 ? 7471 : comp == 1 ? 32768 : -5329;
            const int add = comp == 0 ? 32768 : 8421375;
            int r[64];
            int sum = 0;
#pragma unroll
            for (int y = 0; y < 8; ++y) {
                int smp[8];
#pragma unroll
                for (int x = 0; x < 8; ++x) {
                    const int py = y0 + y * step, px = x0 + x * step;
                    int v = jpeg_component(frame, py, px, g.height, g.width, cr, cg, cb, add);
                    if (step == 2) {
                        v += jpeg_component(frame, py, px + 1, g.height, g.width, cr, cg, cb, add);
                        v += jpeg_component(frame, py + 1, px, g.height, g.width, cr, cg, cb, add);
                        v += jpeg_component(frame, py + 1, px + 1, g.height, g.width, cr, cg, cb, add);
                        v = (v + 2) >> 2;
                    }
                    smp[x] = v - 128;
                    sum += smp[x];
                }
                int o[8];
                jpeg_dct8(smp, o);
#pragma unroll
                for (int u = 0; u < 8; ++u) r[y * 8 + u] = (o[u] + 128) >> 8;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                int col[8], o[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) col[k] = r[k * 8 + u];
                jpeg_dct8(col, o);
                if (u == 0) o[0] = sum * 131072;                   // the exact DC term, 2^20 * sum / 8
#pragma unroll
                for (int v = 0; v < 8; ++v) {
                    const int zz = jpeg_tables.zz_pos[v * 8 + u];
                    const unsigned q = qt[tbl][zz];
                    const unsigned a = (unsigned)(o[v] < 0 ? -o[v] : o[v]);
                    const int level = (int)(((a + (q << 19)) >> 20) / q);
                    coef[zz][tid] = (short)(o[v] < 0 ? -level : level);
                }
            }
            dcs[8 + tid] = coef[0][tid];
        }
        __syncthreads();
        // the block's bits
        const int back = s420 ? (comp ? 6 : (j ? 1 : 3)) : 3;  // the block before of the same component
        const int diff = active ? (int)coef[0][tid] - (b >= back ? dcs[8 + tid - back] : 0) : 0;
        const unsigned dc_cat = jpeg_category(diff);
        const unsigned zrl = hac[tbl][0xf0], eob = hac[tbl][0x00];
        unsigned bits = 0;
        if (active) {
            bits = (hdc[tbl][dc_cat] >> 16) + dc_cat;
            unsigned run = 0;
            for (int k = 1; k < 64; ++k) {
                const int v = coef[k][tid];
                if (v == 0) {
                    ++run;
                } else {
                    const unsigned cat = jpeg_category(v);
                    bits += (run >> 4) * (zrl >> 16) + (hac[tbl][((run & 15u) << 4) | cat] >> 16) + cat;
                    run = 0;
                }
            }
            if (run) bits += eob >> 16;
        }
        unsigned total = 0;
        const unsigned at = cursor + refid_block_scan<JPEG_BLOCKS / 64>(bits, red, &total) - 32u * (unsigned)w0;    // bit position in the image
        if (tid >= JPEG_BLOCKS - 8) dcs[tid - (JPEG_BLOCKS - 8)] = dcs[8 + tid];       // (dcs[0..8) was last read before the scan's barriers)
        if (active) {
            RefidBitWriter<JPEG_ORDER> p(at);                  // (a code and its value bits: at most 16 + 11 bits a put)
            const unsigned e = hdc[tbl][dc_cat];
            p.put(image, ((e & 0xffffu) << dc_cat) | ((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << dc_cat) - 1u)), (e >> 16) + dc_cat);
            unsigned run = 0;
            for (int k = 1; k < 64; ++k) {
                const int v = coef[k][tid];
                if (v == 0) {
                    ++run;
                } else {
                    for (; run > 15u; run -= 16u) p.put(image, zrl & 0xffffu, zrl >> 16);
                    const unsigned cat = jpeg_category(v);
                    const unsigned c = hac[tbl][(run << 4) | cat];
                    p.put(image, ((c & 0xffffu) << cat) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u)), (c >> 16) + cat);
                    run = 0;
                }
            }
            if (run) p.put(image, eob & 0xffffu, eob >> 16);
            p.flush(image);
        }
        cursor += total;
        __syncthreads();                                       // the pass's bits are in the image
        // the complete words leave; the incomplete one opens the next image (the barrier at the top of the pass closes it)
        refid_bits_retire<JPEG_BLOCKS>(image, cursor, w0, [&ff, parked](int w, unsigned v) {
            ff += jpeg_ff_bytes(v);
            parked[w] = __builtin_bswap32(v);
        });
    }
    __syncthreads();
    // padding to a byte with 1-bits; the last, incomplete word: only its bytes below the segment's end count
    const unsigned pad = (0u - cursor) & 7u;
    const unsigned end_bytes = (cursor + pad) >> 3;
    if (tid == 0) {
        const unsigned rest = cursor - 32u * (unsigned)w0;     // bits in image[0]: < 32
        unsigned v = image[0];
        if (pad) v |= ((1u << pad) - 1u) << (32u - rest - pad);
        const unsigned n = (rest + pad) >> 3;                  // bytes of it: 0 .. 4
        if (n) parked[w0] = __builtin_bswap32(v);              // (the room is a multiple of 4 bytes)
        for (unsigned k = 0; k < n; ++k) ff += ((v >> (24u - 8u * k)) & 0xffu) == 0xffu;
    }
    unsigned ff_total = 0;
    refid_block_scan<JPEG_BLOCKS / 64>(ff, red, &ff_total);
    if (tid == 0) {
        rec[JPEG_REC_RAW] = end_bytes;
        rec[JPEG_REC_STUFFED] = end_bytes + ff_total;
    }
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_offsets_kernel(uint8_t* __restrict__ out, int* __restrict__ lens_out, unsigned* __restrict__ work,
                                                                    const JpegGeom g, const JpegHeader header) {
    __shared__ unsigned red[JPEG_THREADS / 64];
    const int tid = threadIdx.x, f = blockIdx.x;
    unsigned* rec = work + (long long)f * g.segs * JPEG_REC;
    // a segment's bytes in the file: stuffed, and RSTm in front of all but the first (the sum is below the bound, which fits int32)
    const unsigned need = REFID_JPEG_HEADER_BYTES + 2;         // around the segments: the header and EOI
    const unsigned pitch = (unsigned)g.out_pitch;
    const unsigned total = need + refid_chunk_offsets<JPEG_THREADS>(
        g.segs, red, [rec](int j) { return rec[(long long)j * JPEG_REC + JPEG_REC_STUFFED] + (j ? 2u : 0u); },
        [rec, need, pitch](int j, unsigned off, unsigned sum) {
            unsigned* r = rec + (long long)j * JPEG_REC;
            r[JPEG_REC_OFF] = REFID_JPEG_HEADER_BYTES + off;   // where its RSTm (segment 0: its first byte) goes
            r[JPEG_REC_FITS] = need + sum <= pitch ? 1u : 0u;
        });
    const bool fits = total <= pitch;
    if (fits) {
        uint8_t* o = out + (long long)f * g.out_pitch;
        for (int i = tid; i < REFID_JPEG_HEADER_BYTES; i += JPEG_THREADS) o[i] = header.b[i];
        if (tid == 0) o[total - 2] = 0xff, o[total - 1] = 0xd9;
    }
    if (tid == 0) lens_out[f] = fits ? (int)total : -(int)total;
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_place_kernel(uint8_t* __restrict__ out, const unsigned* __restrict__ work, const JpegGeom g) {
    __shared__ unsigned red[JPEG_THREADS / 64];
    const int tid = threadIdx.x;
    const int f = blockIdx.x / g.segs, s = blockIdx.x % g.segs;
    const unsigned* rec = work + (long long)blockIdx.x * JPEG_REC;
    if (!rec[JPEG_REC_FITS]) return;                           // (workgroup-uniform)
    const uint8_t* parked = reinterpret_cast<const uint8_t*>(work + (long long)g.n_frames * g.segs * JPEG_REC + (long long)blockIdx.x * (g.seg_stride / 4));
    const int raw = (int)rec[JPEG_REC_RAW];
    uint8_t* o = out + (long long)f * g.out_pitch + rec[JPEG_REC_OFF];
    if (s) {
        if (tid == 0) o[0] = 0xff, o[1] = (uint8_t)(0xd0 + ((s - 1) & 7));
        o += 2;
    }
    unsigned cursor = 0;
    for (int i0 = tid * JPEG_PER_THREAD; i0 - tid * JPEG_PER_THREAD < raw; i0 += JPEG_PASS) {      // (the same trip count in every thread)
        const int mine = max(0, min(JPEG_PER_THREAD, raw - i0));
        unsigned d[JPEG_PER_THREAD / 4] = {0, 0, 0, 0};
        if (mine) {                                            // the room is a multiple of 4 bytes and 4-byte aligned; i0 is a multiple of 16
#pragma unroll
            for (int k = 0; k < JPEG_PER_THREAD / 4; ++k)
                if (4 * k < mine) d[k] = *reinterpret_cast<const unsigned*>(parked + i0 + 4 * k);
        }
        unsigned n = 0;
#pragma unroll
        for (int k = 0; k < JPEG_PER_THREAD; ++k) n += k < mine ? 1u + (((d[k >> 2] >> (8 * (k & 3))) & 0xffu) == 0xffu) : 0u;
        unsigned total = 0;
        unsigned at = cursor + refid_block_scan<JPEG_THREADS / 64>(n, red, &total);
#pragma unroll
        for (int k = 0; k < JPEG_PER_THREAD; ++k) {
            if (k < mine) {
                const unsigned byte = (d[k >> 2] >> (8 * (k & 3))) & 0xffu;
                o[at++] = (uint8_t)byte;
                if (byte == 0xffu) o[at++] = 0;
            }
        }
        cursor += total;
    }
}

// false for what the entry point turns down; else the geometry (without n_frames and out_pitch)
bool jpeg_geometry(long long height, long long width, long long subsampling, long long restart_mcus, JpegGeom* g) {
    if (height < 1 || height > 65535 || width < 1 || width > 65535 || restart_mcus < 0 || restart_mcus > 65535) return false;
    if (subsampling != REFID_JPEG_444 && subsampling != REFID_JPEG_420) return false;
    g->height = (int)height, g->width = (int)width, g->subsampling = (int)subsampling;
    g->mcu = subsampling == REFID_JPEG_420 ? 16 : 8;
    g->bpm = subsampling == REFID_JPEG_420 ? 6 : 3;
    g->rows = (g->height + g->mcu - 1) / g->mcu, g->cols = (g->width + g->mcu - 1) / g->mcu;
    g->restart = restart_mcus ? (int)restart_mcus : g->cols;
    const long long mcus = (long long)g->rows * g->cols;
    g->segs = (int)((mcus + g->restart - 1) / g->restart);
    const long long last = (mcus - (long long)(g->segs - 1) * g->restart) * g->bpm;
    const long long full = g->segs > 1 ? (long long)g->restart * g->bpm : last;        // the blocks of the largest segment
    g->seg_stride = (int)(((full * REFID_JPEG_BLOCK_BITS + 7) / 8 + 3) / 4 * 4);           // (<= 65535 * 6 * 208: fits)
    g->bound = REFID_JPEG_HEADER_BYTES + (long long)(g->segs - 1) * (2 * ((full * REFID_JPEG_BLOCK_BITS + 7) / 8) + 2) +
               2 * ((last * REFID_JPEG_BLOCK_BITS + 7) / 8) + 2;
    return g->bound <= 0x7fffffffll;
}

void jpeg_quant(int quality, JpegQuant* q) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) {
            const int v = (JPEG_QUANT[t][JPEG_ZIGZAG[k]] * s + 50) / 100;
            q->q[t][k] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
}

void jpeg_header(const JpegGeom& g, const JpegQuant& q, JpegHeader* h) {
    uint8_t* p = h->b;
    auto put = [&p](std::initializer_list<int> bytes) { for (int v : bytes) *p++ = (uint8_t)v; };
    put({0xff, 0xd8});
    put({0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    put({0xff, 0xdb, 0, 2 + 2 * 65});
    for (int t = 0; t < 2; ++t) {
        put({t});
        for (int k = 0; k < 64; ++k) put({q.q[t][k]});
    }
    const int hv = g.subsampling == REFID_JPEG_420 ? 0x22 : 0x11;
    put({0xff, 0xc0, 0, 17, 8, g.height >> 8, g.height & 255, g.width >> 8, g.width & 255, 3, 1, hv, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int c = 0; c < 2; ++c) {
        put({0xff, 0xc4, 0, 2 + 1 + 16 + 12, 0x00 | c});
        for (int k = 0; k < 16; ++k) put({JPEG_DC_BITS[c][k]});
        for (int k = 0; k < 12; ++k) put({k});
        put({0xff, 0xc4, 0, 2 + 1 + 16 + 162, 0x10 | c});
        for (int k = 0; k < 16; ++k) put({JPEG_AC_BITS[c][k]});
        for (int k = 0; k < 162; ++k) put({JPEG_AC_VALS[c][k]});
    }
    put({0xff, 0xdd, 0, 4, g.restart >> 8, g.restart & 255});
    put({0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    while (p < h->b + sizeof(h->b)) *p++ = 0;                  // (p == b + REFID_JPEG_HEADER_BYTES here)
}

}  // namespace

extern "C" size_t refid_jpeg_header_bytes(void) { return REFID_JPEG_HEADER_BYTES; }

extern "C" size_t refid_jpeg_bound(int32_t height, int32_t width, int32_t subsampling, int32_t restart_mcus) {
    JpegGeom g;
    return jpeg_geometry(height, width, subsampling, restart_mcus, &g) ? (size_t)g.bound : 0;
}

extern "C" size_t refid_jpeg_work_bytes(int32_t n_frames, int32_t height, int32_t width, int32_t subsampling, int32_t restart_mcus) {
    JpegGeom g;
    if (n_frames < 1 || !jpeg_geometry(height, width, subsampling, restart_mcus, &g)) return 0;
    if ((long long)n_frames * g.segs > 0x7fffffffll) return 0;
    return (size_t)n_frames * (size_t)g.segs * (size_t)(4 * JPEG_REC + g.seg_stride);
}

extern "C" int refid_jpeg_encode(const refid_jpeg_desc* d, void* stream) {
    REFID_CHECK(d, "jpeg: null descriptor");
    REFID_CHECK(d->frames && d->out && d->lens && d->work, "jpeg: %s is null",
                !d->frames ? "frames" : !d->out ? "out" : !d->lens ? "lens" : "work");
    REFID_CHECK(d->n_frames > 0, "jpeg: n_frames %d must be positive", d->n_frames);
    REFID_CHECK(d->height >= 1 && d->height <= 65535, "jpeg: height %d is not 1 .. 65535", d->height);
    REFID_CHECK(d->width >= 1 && d->width <= 65535, "jpeg: width %d is not 1 .. 65535", d->width);
    REFID_CHECK(d->quality >= 1 && d->quality <= 100, "jpeg: quality %d is not 1 .. 100", d->quality);
    REFID_CHECK(d->subsampling == REFID_JPEG_444 || d->subsampling == REFID_JPEG_420, "jpeg: subsampling %d is neither REFID_JPEG_444 (%d) nor REFID_JPEG_420 (%d)",
                d->subsampling, REFID_JPEG_444, REFID_JPEG_420);
    REFID_CHECK(d->restart_mcus >= 0 && d->restart_mcus <= 65535, "jpeg: restart_mcus %d is not 0 .. 65535", d->restart_mcus);
    JpegGeom g;
    REFID_CHECK(jpeg_geometry(d->height, d->width, d->subsampling, d->restart_mcus, &g),
                "jpeg: the bound of a height %d x width %d frame exceeds a 31-bit length", d->height, d->width);
    REFID_CHECK((long long)d->n_frames * g.segs <= 0x7fffffffll, "jpeg: n_frames %d of %d segments exceed the grid", d->n_frames, g.segs);
    REFID_CHECK(d->out_pitch >= REFID_JPEG_HEADER_BYTES + 2, "jpeg: out_pitch %d is below the header and EOI, %d", d->out_pitch,
                REFID_JPEG_HEADER_BYTES + 2);
    REFID_CHECK(((unsigned long long)d->lens & 3ull) == 0, "jpeg: lens is not aligned to 4 bytes");
    REFID_CHECK(((unsigned long long)d->work & 3ull) == 0, "jpeg: work is not aligned to 4 bytes");
    g.n_frames = d->n_frames, g.out_pitch = d->out_pitch;
    JpegQuant q;
    JpegHeader h;
    jpeg_quant(d->quality, &q);
    jpeg_header(g, q, &h);
    const unsigned grid = (unsigned)d->n_frames * (unsigned)g.segs;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_code_kernel, dim3(grid), dim3(JPEG_BLOCKS), 0, st, d->frames, d->work, g, q);
    REFID_LAUNCH_CHECK("jpeg (codes)");
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3((unsigned)d->n_frames), dim3(JPEG_THREADS), 0, st, d->out, d->lens, d->work, g, h);
    REFID_LAUNCH_CHECK("jpeg (offsets)");
    hipLaunchKernelGGL(jpeg_place_kernel, dim3(grid), dim3(JPEG_THREADS), 0, st, d->out, (const unsigned*)d->work, g);
    REFID_LAUNCH_CHECK("jpeg (place)");
    return 0;
}
