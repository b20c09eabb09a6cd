// Huffman-only deflate of the filtered rows png_filter.hip writes: one zlib stream per frame, one dynamic (or stored) block
// segment per PNGD block of input bytes, every segment byte-aligned by an empty stored block so that the blocks are coded
// independently and laid end to end.  The format is stated in include/refid_hip.h and restated in tests/deflate_ref.py.
//
// Three launches that meet only at the kernel boundaries; no workgroup waits for another, nothing spins, every loop count
// is known before the loop starts.
//   png_deflate_code_kernel    one workgroup per block.  256-bin histogram by LDS integer adds (one copy per wave; the
//     order of integer adds is free), the block's Adler sums A = sum d_i and B = sum (len - i) d_i modulo 65521 (per thread
//     in 64 bits, reduced before they are added up), a rank sort of the <= 257 occurring symbols by (frequency, symbol),
//     then ONE lane walks the two-queue merge, the depths and zlib's length repair in LDS (2*257 nodes per 1..64 KiB of
//     data), and all lanes deal the lengths out, number the canonical codes and add up the segment's bits.  The block's
//     record in `work` gets the segment length, stored / dynamic, A, B and the 257 (bit-reversed code, length) pairs.
//   png_deflate_offsets_kernel one workgroup per stream.  Exclusive sum of the segment lengths into the records (the chunk
//     walk of bit_image.h), the Adler sums combined in block order, then 78 01, the terminator, the Adler-32 and lens.
//   png_deflate_pack_kernel    one workgroup per block.  The bit stream is put together LSB first in the LDS image of
//     bit_image.h (writer, retire step and their barrier contract are stated there), which here stands for the ALIGNED
//     global words the segment lands in (bit 0 of the image is the first bit of the word that holds the segment's first
//     byte), 4096 input bytes per pass, 16 consecutive bytes per thread.  The sink stores complete words as aligned
//     dwords.  The first and the last word of a segment may share their word with the neighbouring segment: the bytes of
//     such a word that belong to this segment are stored one by one, by the lane that holds the word.  No global
//     atomics, no read-modify-write of a global word; nothing outside the segment's bytes is written.  Stored segments
//     are copied byte by byte.
// The workgroup sums and the scan are those of workgroup.h.
#include "common.h"
#include "bit_image.h"

namespace {

constexpr int PNGD_THREADS = 256;
constexpr int PNGD_REC = REFID_PNG_DEFLATE_RECORD / 4;        // words of a block's record in `work`
constexpr int PNGD_REC_SEG = 0, PNGD_REC_STORED = 1, PNGD_REC_A = 2, PNGD_REC_B = 3, PNGD_REC_OFF = 4, PNGD_REC_CODES = 8;
constexpr int PNGD_SYMS = 257;
constexpr int PNGD_MAX_BITS = 15;
constexpr unsigned PNGD_ADLER = 65521u;
constexpr int PNGD_FIXED_BITS = 3 + 5 + 5 + 4 + 19 * 3;       // block header up to the code-length-code lengths: 74
constexpr int PNGD_HEADER_BITS = PNGD_FIXED_BITS + 258 * 4;   // + 257 lengths and one distance length, 4 bits each: 1106
constexpr int PNGD_PER_THREAD = 16;
constexpr int PNGD_PASS = PNGD_THREADS * PNGD_PER_THREAD;     // input bytes per pass of the pack kernel
constexpr int PNGD_IMAGE = (31 + PNGD_PASS * PNGD_MAX_BITS + 31) / 32 + 3;      // words: carried bits + a pass at 15 bits per byte
static_assert(PNGD_REC_CODES + PNGD_SYMS <= PNGD_REC, "record too small");
static_assert(PNGD_IMAGE * 32 >= 31 + PNGD_HEADER_BITS && PNGD_IMAGE * 32 >= 31 + 15 + 3 + 7 + 32, "image too small");

// bit i of the fixed 74 bits: BFINAL 0 | BTYPE 10 (bit 2) | HLIT 0 | HDIST 0 | HCLEN 15 (bits 13..16) | lengths 0 0 0 (symbols 16,
// 17, 18), then sixteen times 4 = the third bit of every 3-bit entry from the fourth on
__device__ __forceinline__ bool pngd_fixed_bit(int i) {
    return i == 2 || (i >= 13 && i < 17) || (i >= 17 + 9 && (i - 17) % 3 == 2);
}

constexpr int PNGD_WAVES = PNGD_THREADS / 64;
constexpr RefidBitOrder PNGD_ORDER = REFID_BITS_LSB_FIRST;     // deflate packs codes from bit 0 of a byte up

__global__ __launch_bounds__(PNGD_THREADS) void png_deflate_code_kernel(const uint8_t* __restrict__ src, unsigned* __restrict__ work,
                                                                        int n_blocks, int stream_bytes, int block_bytes) {
    __shared__ unsigned hist[4][256];
    __shared__ unsigned freq[PNGD_SYMS], key[PNGD_SYMS], sorted[PNGD_SYMS], lens[PNGD_SYMS];
    __shared__ unsigned node_freq[2 * PNGD_SYMS];
    __shared__ unsigned short parent[2 * PNGD_SYMS];
    __shared__ unsigned char depth[2 * PNGD_SYMS];
    __shared__ unsigned count[PNGD_MAX_BITS + 1], next_code[PNGD_MAX_BITS + 1];
    __shared__ unsigned red[PNGD_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int s = blockIdx.x / n_blocks, b = blockIdx.x % n_blocks;
    const int start = b * block_bytes;                         // (< stream_bytes < 2^31)
    const int len = min(block_bytes, stream_bytes - start);
    const uint8_t* p = src + (long long)s * stream_bytes + start;
    unsigned* rec = work + (long long)blockIdx.x * PNGD_REC;

    for (int i = tid; i < 4 * 256; i += PNGD_THREADS) (&hist[0][0])[i] = 0;
    __syncthreads();
    // aligned dwords of the input; the bytes in front of the first and behind the last one by one
    const int head = min((int)((4 - ((unsigned long long)p & 3)) & 3), len);
    const int n_words = (len - head) >> 2, tail = len - head - 4 * n_words;
    unsigned s1 = 0;
    unsigned long long s2 = 0;                                 // <= 258 terms below 2^24 each
    for (int w = tid; w < n_words; w += PNGD_THREADS) {
        const int i0 = head + 4 * w;
        const unsigned v = *reinterpret_cast<const unsigned*>(p + i0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned d = (v >> (8 * k)) & 0xffu;
            atomicAdd(&hist[wave][d], 1u);
            s1 += d;
            s2 += (unsigned long long)(unsigned)(len - i0 - k) * d;
        }
    }
    if (tid < head) {
        const unsigned d = p[tid];
        atomicAdd(&hist[wave][d], 1u);
        s1 += d;
        s2 += (unsigned long long)(unsigned)(len - tid) * d;
    }
    if (tid < tail) {
        const int i = head + 4 * n_words + tid;
        const unsigned d = p[i];
        atomicAdd(&hist[wave][d], 1u);
        s1 += d;
        s2 += (unsigned long long)(unsigned)(len - i) * d;
    }
    // the three sums of this kernel share `red`: the barrier in front of each keeps its store behind the reads of the one before
    __syncthreads();
    const unsigned sum_a = refid_block_sum<unsigned, PNGD_WAVES>(s1, red);             // <= 65535 * 255; (its barrier also closes the histogram)
    __syncthreads();
    const unsigned sum_b = refid_block_sum<unsigned, PNGD_WAVES>((unsigned)(s2 % PNGD_ADLER), red);      // 256 terms below 65521

    // frequencies and sort keys; end-of-block (256) occurs once
    {
        const unsigned f = hist[0][tid] + hist[1][tid] + hist[2][tid] + hist[3][tid];
        freq[tid] = f;
        key[tid] = f ? (f << 9) | (unsigned)tid : 0xffffffffu;
        lens[tid] = 0;
        if (tid == 0) freq[256] = 1, key[256] = (1u << 9) | 256u, lens[256] = 0;
    }
    const int n = __syncthreads_count(freq[tid] != 0) + 1;     // leaves: 2 .. 257
    // rank sort: the keys of occurring symbols are distinct
    for (int sym = tid; sym < PNGD_SYMS; sym += PNGD_THREADS) {
        const unsigned k = key[sym];
        if (k != 0xffffffffu) {
            int r = 0;
            for (int j = 0; j < PNGD_SYMS; ++j) r += key[j] < k ? 1 : 0;
            sorted[r] = k;
            node_freq[r] = k >> 9;
        }
    }
    __syncthreads();
    if (tid == 0) {
        // two queues: leaves 0 .. n-1 in sorted order, merged nodes n .. 2n-2 in order of creation; the leaf wins a tie
        int leaf = 0, merged = n, next = n;
        for (int m = 0; m < n - 1; ++m) {
            int pick[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (leaf < n && (merged >= next || node_freq[leaf] <= node_freq[merged])) pick[q] = leaf++;
                else pick[q] = merged++;
            }
            node_freq[next] = node_freq[pick[0]] + node_freq[pick[1]];
            parent[pick[0]] = parent[pick[1]] = (unsigned short)next;
            ++next;
        }
        for (int l = 0; l <= PNGD_MAX_BITS; ++l) count[l] = 0;
        int overflow = 0;
        depth[2 * n - 2] = 0;
        for (int i = 2 * n - 3; i >= 0; --i) {                 // a parent was created after its children: it comes first
            int d = depth[parent[i]] + 1;
            if (d > PNGD_MAX_BITS) d = PNGD_MAX_BITS, ++overflow;
            depth[i] = (unsigned char)d;
            if (i < n) ++count[d];
        }
        // zlib's gen_bitlen repair; overflow is bounded by 2n before the loop and falls by 2 per turn
        for (int turn = 0, turns = (overflow + 1) / 2; turn < turns; ++turn) {
            int bits = 1;                                      // the longest length below 15 that has a leaf (one exists)
            for (int l = 2; l < PNGD_MAX_BITS; ++l) bits = count[l] ? l : bits;
            --count[bits];
            count[bits + 1] += 2;
            --count[PNGD_MAX_BITS];
        }
        unsigned code = 0;
        next_code[0] = 0;
        for (int l = 1; l <= PNGD_MAX_BITS; ++l) {
            code = (code + (l > 1 ? count[l - 1] : 0u)) << 1;
            next_code[l] = code;
        }
    }
    __syncthreads();
    // the counts dealt out longest first over the leaves in sorted order
    for (int i = tid; i < n; i += PNGD_THREADS) {
        int l = PNGD_MAX_BITS, before = 0;
#pragma unroll
        for (int bits = PNGD_MAX_BITS; bits >= 1; --bits) {
            const int c = (int)count[bits];
            if (i >= before + c && l == bits) l = bits - 1;
            before += c;
        }
        lens[sorted[i] & 511u] = (unsigned)l;
    }
    __syncthreads();
    // canonical codes: symbols of one length in symbol order; stored bit-reversed, as the stream wants them
    unsigned body = 0;
    for (int sym = tid; sym < PNGD_SYMS; sym += PNGD_THREADS) {
        const unsigned l = lens[sym];
        unsigned entry = 0;
        if (l) {
            unsigned c = next_code[l];
            for (int j = 0; j < PNGD_SYMS - 1; ++j) c += (j < sym && lens[j] == l) ? 1u : 0u;
            entry = (__brev(c) >> (32 - l)) | (l << 16);
        }
        rec[PNGD_REC_CODES + sym] = entry;
        body += freq[sym] * l;                                 // <= 65536 * 15 over the workgroup
    }
    __syncthreads();
    body = refid_block_sum<unsigned, PNGD_WAVES>(body, red);
    if (tid == 0) {
        const unsigned bits = PNGD_HEADER_BITS + body + 3;
        const unsigned dynamic = (bits + 7) / 8 + 4;
        const bool stored = dynamic >= (unsigned)len + 5;
        rec[PNGD_REC_SEG] = stored ? (unsigned)len + 5 : dynamic;
        rec[PNGD_REC_STORED] = stored ? 1u : 0u;
        rec[PNGD_REC_A] = sum_a % PNGD_ADLER;
        rec[PNGD_REC_B] = sum_b % PNGD_ADLER;
    }
}

__global__ __launch_bounds__(PNGD_THREADS) void png_deflate_offsets_kernel(uint8_t* __restrict__ out, unsigned* __restrict__ lens_out,
                                                                           unsigned* __restrict__ work, int n_blocks, int stream_bytes,
                                                                           int block_bytes, int out_pitch) {
    __shared__ unsigned red[PNGD_WAVES];
    __shared__ unsigned part_a[PNGD_THREADS], part_b[PNGD_THREADS], part_l[PNGD_THREADS];
    const int tid = threadIdx.x, s = blockIdx.x;
    unsigned* rec = work + (long long)s * n_blocks * PNGD_REC;
    // a thread's blocks lo .. hi-1 (the chunk the walk below gives it too): their Adler sums combined in order:
    // (A1, B1, L1) then (A2, B2, L2) = (A1 + A2, B1 + L2 A1 + B2, L1 + L2)
    int lo, hi;
    refid_chunk<PNGD_THREADS>(n_blocks, &lo, &hi);
    unsigned long long a = 0, bsum = 0, l = 0;
    for (int j = lo; j < hi; ++j) {
        const unsigned* r = rec + (long long)j * PNGD_REC;
        const unsigned long long l2 = (unsigned)(j == n_blocks - 1 ? stream_bytes - j * block_bytes : block_bytes);
        bsum = (bsum + l2 * a + r[PNGD_REC_B]) % PNGD_ADLER;
        a = (a + r[PNGD_REC_A]) % PNGD_ADLER;
        l = (l + l2) % PNGD_ADLER;
    }
    part_a[tid] = (unsigned)a, part_b[tid] = (unsigned)bsum, part_l[tid] = (unsigned)l;
    // the segments laid end to end behind 78 01; (the scan's barriers also publish the parts)
    const unsigned total = refid_chunk_offsets<PNGD_THREADS>(
        n_blocks, red, [rec](int j) { return rec[(long long)j * PNGD_REC + PNGD_REC_SEG]; },
        [rec](int j, unsigned off, unsigned) { rec[(long long)j * PNGD_REC + PNGD_REC_OFF] = 2 + off; });
    if (tid == 0) {
        unsigned long long ta = 0, tb = 0, tl = 0;
        for (int t = 0; t < PNGD_THREADS; ++t) {
            tb = (tb + (unsigned long long)part_l[t] * ta + part_b[t]) % PNGD_ADLER;
            ta = (ta + part_a[t]) % PNGD_ADLER;
            tl = (tl + part_l[t]) % PNGD_ADLER;
        }
        const unsigned adler_a = (unsigned)((1 + ta) % PNGD_ADLER), adler_b = (unsigned)((tl + tb) % PNGD_ADLER);     // a starts at 1
        uint8_t* o = out + (long long)s * out_pitch;
        o[0] = 0x78, o[1] = 0x01;
        uint8_t* e = o + 2 + total;
        e[0] = 0x01, e[1] = 0x00, e[2] = 0x00, e[3] = 0xff, e[4] = 0xff;
        e[5] = (uint8_t)(adler_b >> 8), e[6] = (uint8_t)adler_b, e[7] = (uint8_t)(adler_a >> 8), e[8] = (uint8_t)adler_a;
        lens_out[s] = 2 + total + 9;
    }
}

// where the image's words go: word w of the stream is the aligned global word w counted from `base`; the segment owns
// bytes [lo, hi) from base
struct PngdFlush {
    uint8_t* base;
    int lo, hi;
    __device__ __forceinline__ void operator()(int w, unsigned v) const {
        const int byte0 = 4 * w;
        if (byte0 >= lo && byte0 + 4 <= hi) {
            *reinterpret_cast<unsigned*>(base + byte0) = v;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (byte0 + k >= lo && byte0 + k < hi) base[byte0 + k] = (uint8_t)(v >> (8 * k));
        }
    }
};

__global__ __launch_bounds__(PNGD_THREADS) void png_deflate_pack_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ out,
                                                                        const unsigned* __restrict__ work, int n_blocks, int stream_bytes,
                                                                        int block_bytes, int out_pitch) {
    __shared__ unsigned table[PNGD_SYMS + 1];
    __shared__ unsigned image[PNGD_IMAGE];
    __shared__ unsigned red[PNGD_WAVES];
    const int tid = threadIdx.x;
    const int s = blockIdx.x / n_blocks, b = blockIdx.x % n_blocks;
    const int start = b * block_bytes;
    const int len = min(block_bytes, stream_bytes - start);
    const uint8_t* p = src + (long long)s * stream_bytes + start;
    const unsigned* rec = work + (long long)blockIdx.x * PNGD_REC;
    const int seg = (int)rec[PNGD_REC_SEG];
    uint8_t* o = out + (long long)s * out_pitch + rec[PNGD_REC_OFF];

    if (rec[PNGD_REC_STORED]) {                                // (workgroup-uniform)
        if (tid == 0) {
            o[0] = 0, o[1] = (uint8_t)len, o[2] = (uint8_t)(len >> 8), o[3] = (uint8_t)~len, o[4] = (uint8_t)(~len >> 8);
        }
        for (int i = tid; i < len; i += PNGD_THREADS) o[5 + i] = p[i];
        return;
    }

    const int lo = (int)((unsigned long long)o & 3), hi = lo + seg;       // the segment's bytes, counted from the aligned word
    const PngdFlush flush = {o - lo, lo, hi};
    for (int i = tid; i < PNGD_SYMS + 1; i += PNGD_THREADS) table[i] = i < PNGD_SYMS ? rec[PNGD_REC_CODES + i] : 0u;     // (257: the distance length)
    for (int i = tid; i < PNGD_IMAGE; i += PNGD_THREADS) image[i] = 0;
    __syncthreads();

    // the header
    unsigned cursor = 8u * lo;                                 // bit position of the next bit, counted from base
    int w0 = 0;                                                // the global word that image[0] stands for
    if (tid < PNGD_FIXED_BITS && pngd_fixed_bit(tid)) refid_bits_put_at<PNGD_ORDER>(image, cursor + tid, 1u, 1u);
    for (int i = tid; i < PNGD_SYMS + 1; i += PNGD_THREADS) {
        const unsigned l = table[i] >> 16;
        refid_bits_put_at<PNGD_ORDER>(image, cursor + PNGD_FIXED_BITS + 4 * i, ((l & 1) << 3) | ((l & 2) << 1) | ((l & 4) >> 1) | ((l & 8) >> 3), 4u);
    }
    cursor += PNGD_HEADER_BITS;

    const int passes = (len + PNGD_PASS - 1) / PNGD_PASS;
    for (int pass = 0; pass <= passes; ++pass) {
        __syncthreads();                                       // the bits put so far are in the image
        refid_bits_retire<PNGD_THREADS>(image, cursor, w0, flush);       // the complete words leave; the incomplete one opens the next image
        __syncthreads();
        if (pass == passes) break;

        const int i0 = pass * PNGD_PASS + tid * PNGD_PER_THREAD;
        const int mine = max(0, min(PNGD_PER_THREAD, len - i0));
        unsigned d[PNGD_PER_THREAD / 4] = {0, 0, 0, 0};
        if (mine == PNGD_PER_THREAD) {
            __builtin_memcpy(d, p + i0, PNGD_PER_THREAD);      // (no alignment is assumed)
        } else {
            for (int k = 0; k < mine; ++k) d[k >> 2] |= (unsigned)p[i0 + k] << (8 * (k & 3));
        }
        unsigned bits = 0;
#pragma unroll
        for (int k = 0; k < PNGD_PER_THREAD; ++k)
            bits += k < mine ? table[(d[k >> 2] >> (8 * (k & 3))) & 0xffu] >> 16 : 0u;
        unsigned total = 0;
        RefidBitWriter<PNGD_ORDER> w(cursor + refid_block_scan<PNGD_WAVES>(bits, red, &total) - 32u * w0);      // bit position in the image
#pragma unroll
        for (int k = 0; k < PNGD_PER_THREAD; ++k) {
            if (k < mine) {
                const unsigned e = table[(d[k >> 2] >> (8 * (k & 3))) & 0xffu];
                w.put(image, e & 0xffffu, e >> 16);
            }
        }
        w.flush(image);
        cursor += total;
    }

    // end-of-block, the empty stored block 000, padding to a byte, 00 00 FF FF
    const unsigned eob = table[256];
    if (tid == 0) refid_bits_put_at<PNGD_ORDER>(image, cursor - 32u * w0, eob & 0xffffu, eob >> 16);
    cursor += (eob >> 16) + 3;
    cursor = (cursor + 7u) & ~7u;
    if (tid == 0) refid_bits_put_at<PNGD_ORDER>(image, cursor + 16 - 32u * w0, 0xffffu, 16u);
    cursor += 32;                                              // == 8 * hi
    __syncthreads();
    refid_bits_drain<PNGD_THREADS>(image, (int)((cursor + 31) >> 5) - w0, w0, flush);
}

int pngd_blocks(long long stream_bytes, long long block_bytes) { return (int)((stream_bytes + block_bytes - 1) / block_bytes); }

bool pngd_sizes_ok(long long n_streams, long long stream_bytes, long long block_bytes) {
    if (n_streams < 1 || stream_bytes < 1 || block_bytes < 1 || block_bytes > REFID_PNG_DEFLATE_MAX_BLOCK) return false;
    const long long blocks = (stream_bytes + block_bytes - 1) / block_bytes;
    return 2 + stream_bytes + 5 * blocks + 9 <= 0x7fffffffll && n_streams * blocks <= 0x7fffffffll;
}

}  // namespace

extern "C" size_t refid_png_deflate_bound(int32_t stream_bytes, int32_t block_bytes) {
    if (!pngd_sizes_ok(1, stream_bytes, block_bytes)) return 0;
    return (size_t)2 + (size_t)stream_bytes + (size_t)5 * pngd_blocks(stream_bytes, block_bytes) + 9;
}

extern "C" size_t refid_png_deflate_work_bytes(int32_t n_streams, int32_t stream_bytes, int32_t block_bytes) {
    if (!pngd_sizes_ok(n_streams, stream_bytes, block_bytes)) return 0;
    return (size_t)n_streams * pngd_blocks(stream_bytes, block_bytes) * REFID_PNG_DEFLATE_RECORD;
}

extern "C" int refid_png_deflate(const refid_png_deflate_desc* d, void* stream) {
    REFID_CHECK(d, "png_deflate: null descriptor");
    REFID_CHECK(d->src && d->out && d->lens && d->work, "png_deflate: %s is null",
                !d->src ? "src" : !d->out ? "out" : !d->lens ? "lens" : "work");
    REFID_CHECK(d->n_streams > 0 && d->stream_bytes > 0 && d->block_bytes > 0, "png_deflate: n_streams %d, stream_bytes %d, block_bytes %d must be positive",
                d->n_streams, d->stream_bytes, d->block_bytes);
    REFID_CHECK(d->block_bytes <= REFID_PNG_DEFLATE_MAX_BLOCK, "png_deflate: block_bytes %d exceeds %d (a stored block's LEN is 16 bits)",
                d->block_bytes, REFID_PNG_DEFLATE_MAX_BLOCK);
    REFID_CHECK(pngd_sizes_ok(d->n_streams, d->stream_bytes, d->block_bytes),
                "png_deflate: n_streams %d of stream_bytes %d in blocks of %d exceed the grid or a 31-bit stream", d->n_streams,
                d->stream_bytes, d->block_bytes);
    const size_t bound = refid_png_deflate_bound(d->stream_bytes, d->block_bytes);
    REFID_CHECK(d->out_pitch > 0 && (size_t)d->out_pitch >= bound, "png_deflate: out_pitch %d is below the bound %zu", d->out_pitch, bound);
    REFID_CHECK(((unsigned long long)d->lens & 3ull) == 0, "png_deflate: lens is not aligned to 4 bytes");
    REFID_CHECK(((unsigned long long)d->work & 3ull) == 0, "png_deflate: work is not aligned to 4 bytes");
    const int n_blocks = pngd_blocks(d->stream_bytes, d->block_bytes);
    const unsigned grid = (unsigned)d->n_streams * (unsigned)n_blocks;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(png_deflate_code_kernel, dim3(grid), dim3(PNGD_THREADS), 0, st, d->src, d->work, n_blocks, d->stream_bytes,
                       d->block_bytes);
    REFID_LAUNCH_CHECK("png_deflate (codes)");
    hipLaunchKernelGGL(png_deflate_offsets_kernel, dim3((unsigned)d->n_streams), dim3(PNGD_THREADS), 0, st, d->out, d->lens, d->work,
                       n_blocks, d->stream_bytes, d->block_bytes, d->out_pitch);
    REFID_LAUNCH_CHECK("png_deflate (offsets)");
    hipLaunchKernelGGL(png_deflate_pack_kernel, dim3(grid), dim3(PNGD_THREADS), 0, st, d->src, d->out, d->work, n_blocks,
                       d->stream_bytes, d->block_bytes, d->out_pitch);
    REFID_LAUNCH_CHECK("png_deflate (pack)");
    return 0;
}
