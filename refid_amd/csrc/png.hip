// PNG reconstruction ("unfiltering", PNG specification 9.2 / 9.4) of inflated key frames on the device: the serial half of
// refid_amd/png.py's _unfilter, which walks Average and Paeth rows byte by byte in Python.  Inflate stays on the host.
//
// Byte (y, x) needs a = (y, x-bpp), b = (y-1, x) and c = (y-1, x-bpp): an anti-diagonal wavefront.  One workgroup of
// PNG_THREADS = 256 threads (four waves, one per SIMD) owns one band of rows and walks it in blocks of 256 consecutive rows;
// thread r owns row r of the block.
//   - A step is one GROUP of 12 bytes of a row (four RGB pixels or twelve grey ones: a multiple of both bpp), held in three
//     dwords.  At step t thread r works on group (t - r) mod P of block (t - r) / P, P = max(groups per row, 256): thread
//     r-1 is one group ahead, so `b` of a whole group is thread r-1's result of the previous step -- three __shfl_up per
//     step inside a wave -- and `c` comes from the group `b` was one step earlier; `a` is the thread's own previous
//     result.  All of it is in registers.
//   - Between waves the row above goes through LDS: lane 63 of a wave leaves its group in a two-slot ring for lane 0 of the
//     next wave, which reads it one step later; thread 255's groups go to an LDS line (one row: PNG_LINE_BYTES), which
//     thread 0 reads in the NEXT block.  One __syncthreads per step orders both: P >= 256 puts the line's read at least one
//     step after its write and the next overwrite after the read.  Every dependency stays inside the workgroup in program
//     order: no flag in memory, no spin, nothing between workgroups.  Threads do not wait for a block to drain: a band of
//     R rows takes ceil(R/256) * P + (R-1) mod 256 steps, a bound computed before the loop.
//   - The five filter types differ per lane: every predictor is computed and one is selected, no branch per type.
//   - A row of the input starts at byte 1 + y * (1 + W*bpp), aligned to nothing: a group is moved with one 12-byte copy the
//     compiler is told nothing about the alignment of (__builtin_memcpy: an unaligned dwordx3 access on gfx950).  The last,
//     partial group of a row is read the same way: the surplus is the start of the next row, never used and never stored;
//     at the end of the input the 12 bytes are read ending there and shifted.  Partial groups are stored byte by byte.
//     Nothing is read outside [rows, rows + n*H*pitch) and nothing written outside the frames.
//   - A step's input does not depend on any result, so it is requested PNG_AHEAD steps early into a register queue (with
//     the row's filter byte), without a branch: one wave per band has nothing else to hide the latency of a load behind.
// Integer arithmetic modulo 256 only; no floating point, no atomics: the bytes are defined by the specification.
#include "common.h"

namespace {

constexpr int PNG_GROUP = 12;                              // bytes per step: lcm of the two bpp times four
constexpr int PNG_LINE_BYTES = REFID_PNG_MAX_ROW_BYTES;    // the LDS line: one reconstructed row
constexpr int PNG_THREADS = 256;                          // rows of a block: four waves, one wavefront
constexpr int PNG_AHEAD = 8;                               // steps between the request of a group and its use
static_assert(PNG_LINE_BYTES % PNG_GROUP == 0 && PNG_LINE_BYTES % 4 == 0, "whole groups of whole dwords");
static_assert(PNG_AHEAD % 2 == 0 && PNG_THREADS % 64 == 0, "the ring's slot is the parity of the unrolled step");

__device__ __forceinline__ unsigned png_paeth(unsigned a, unsigned b, unsigned c) {
    const int p = (int)a + (int)b - (int)c;
    const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);                // ties: a, then b, then c
}

// bytes by which a 12-byte read at p would pass the end of the input: 0..11
__device__ __forceinline__ int png_over(const uint8_t* p, const uint8_t* end) {
    const long long past = p + PNG_GROUP - end;
    return past > 0 ? (int)past : 0;
}

template <int BPP>
__global__ __launch_bounds__(PNG_THREADS) void png_unfilter_kernel(const uint8_t* __restrict__ rows, uint8_t* __restrict__ frames,
                                                          const int32_t* __restrict__ bands, int n_frames, int height,
                                                          int width) {
    __shared__ unsigned line[PNG_LINE_BYTES / 4];
    __shared__ unsigned ring[PNG_THREADS / 64][2][4];       // [wave][step parity]: lane 63's group, for the next wave
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int f = blockIdx.x, row0 = 0, row1 = height;
    if (bands) {
        f = bands[3 * blockIdx.x], row0 = bands[3 * blockIdx.x + 1], row1 = bands[3 * blockIdx.x + 2];
        if (f < 0 || f >= n_frames || row0 < 0 || row1 > height || row0 >= row1) return;      // (workgroup-uniform)
    }
    const int stride = width * BPP;                        // bytes of a row without its filter byte
    const int groups = (stride + PNG_GROUP - 1) / PNG_GROUP;
    const int period = groups > PNG_THREADS ? groups : PNG_THREADS;
    const int nblk = (row1 - row0 + PNG_THREADS - 1) / PNG_THREADS;
    const int steps = nblk * period + (row1 - row0 - 1) % PNG_THREADS;
    const uint8_t* src = rows + (size_t)f * height * (stride + 1);
    uint8_t* dst = frames + (size_t)f * height * width * 3;
    const uint8_t* src_end = rows + (size_t)n_frames * height * (stride + 1);
    const bool tiny = (size_t)n_frames * height * (stride + 1) < (size_t)PNG_GROUP;

    // the request queue: entry j holds the three dwords and the filter byte of step t + j
    unsigned queue[PNG_AHEAD][4];
    int qblk = 0, qg = -tid;                               // the cursor of the requests, PNG_AHEAD steps ahead of (blk, g)
    // Branch-free, so that the loads of PNG_AHEAD steps stay in flight: a lane with nothing to do reads the start of the
    // input, and where 12 bytes would pass the end of the input (the tail of its last row) they are read ending there and
    // shifted down.  An input of fewer than 12 bytes (a kernel-uniform case) is read byte by byte at clamped addresses.
    auto request = [&](unsigned (&q)[4]) {
        const int row = row0 + qblk * PNG_THREADS + tid;
        const bool want = qg >= 0 && qg < groups && row < row1;
        const uint8_t* p = want ? src + (size_t)row * (stride + 1) : rows;       // the row's filter byte
        q[3] = p[0];
        p += 1 + (want ? qg * PNG_GROUP : 0);
        if (!tiny) {
            __builtin_memcpy(q, p - png_over(p, src_end), PNG_GROUP);           // shifted down when the step uses it
        } else {
            q[0] = q[1] = q[2] = 0;
#pragma unroll
            for (int i = 0; i < PNG_GROUP; ++i) {
                const uint8_t* b = p + i < src_end ? p + i : src_end - 1;
                q[i >> 2] |= (unsigned)*b << (8 * (i & 3));
            }
        }
        if (++qg == period) qg = 0, ++qblk;
    };
#pragma unroll
    for (int j = 0; j < PNG_AHEAD; ++j) request(queue[j]);

    unsigned rec[3] = {0, 0, 0};                           // this lane's result of the previous step
    unsigned up_prev[3] = {0, 0, 0};                       // the group above the previous step's: c comes from its tail
    int blk = 0, g = -tid;                                 // t - tid = blk * period + g
    // (steps past the last one, up to a whole round of the queue, find every thread beyond its band: they do nothing;
    //  PNG_AHEAD is even, so the parity of step t + j is that of j)
    for (int t = 0; t < steps; t += PNG_AHEAD) {
#pragma unroll
      for (int j = 0; j < PNG_AHEAD; ++j) {
        // b: thread r-1's previous result -- by shuffle, for lane 0 of waves 1.. from the ring; thread 0 takes the last row
        // of the block before, or zero at the top of the band
        unsigned up[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) up[k] = __shfl_up(rec[k], 1, 64);
        const int row = row0 + blk * PNG_THREADS + tid;
        const bool on = g >= 0 && g < groups && row < row1;
        if (tid == 0) {
            const bool have = on && blk > 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) up[k] = have ? line[3 * g + k] : 0u;
        } else if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) up[k] = ring[wave - 1][(j & 1) ^ 1][k];
        }
        if (g == 0) rec[0] = rec[1] = rec[2] = up_prev[0] = up_prev[1] = up_prev[2] = 0;    // nothing left of column 0
        if (on) {
            const int x0 = g * PNG_GROUP, nvalid = min(stride - x0, PNG_GROUP);
            const unsigned ft = queue[j][3];
            unsigned raw[3] = {queue[j][0], queue[j][1], queue[j][2]};
            const int over = tiny ? 0 : png_over(src + (size_t)row * (stride + 1) + 1 + x0, src_end);
            if (over) {                                    // the tail of the input's last row: read ending at the end
                const unsigned w[5] = {raw[0], raw[1], raw[2], 0u, 0u};
                const int ws = over >> 2, bs = 8 * (over & 3);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const unsigned lo = ws == 0 ? w[k] : (ws == 1 ? w[k + 1] : w[k + 2]);
                    const unsigned hi = ws == 0 ? w[k + 1] : (ws == 1 ? w[k + 2] : 0u);
                    raw[k] = (unsigned)((((unsigned long long)hi << 32) | lo) >> bs);
                }
            }
            // bytes 0..2: the tail of the group before (a from rec, c from up_prev); bytes 3..14: this group
            unsigned rx[3 + PNG_GROUP], ux[3 + PNG_GROUP];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                rx[i] = (rec[2] >> (8 * (i + 1))) & 0xffu;
                ux[i] = (up_prev[2] >> (8 * (i + 1))) & 0xffu;
            }
#pragma unroll
            for (int i = 0; i < PNG_GROUP; ++i) ux[3 + i] = (up[i >> 2] >> (8 * (i & 3))) & 0xffu;
#pragma unroll
            for (int i = 0; i < PNG_GROUP; ++i) {
                const unsigned x = (raw[i >> 2] >> (8 * (i & 3))) & 0xffu;
                const unsigned a = rx[3 + i - BPP], b = ux[3 + i], c = ux[3 + i - BPP];
                unsigned pred = 0;
                pred = ft == 1 ? a : pred;
                pred = ft == 2 ? b : pred;
                pred = ft == 3 ? (a + b) >> 1 : pred;
                pred = ft == 4 ? png_paeth(a, b, c) : pred;
                rx[3 + i] = (x + pred) & 0xffu;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                rec[k] = rx[3 + 4 * k] | (rx[4 + 4 * k] << 8) | (rx[5 + 4 * k] << 16) | (rx[6 + 4 * k] << 24);
                up_prev[k] = up[k];
            }
            if (BPP == 3) {
                uint8_t* q = dst + ((size_t)row * width) * 3 + x0;
                if (nvalid == PNG_GROUP) {
                    __builtin_memcpy(q, rec, PNG_GROUP);
                } else {
#pragma unroll
                    for (int i = 0; i < PNG_GROUP; ++i)
                        if (i < nvalid) q[i] = (uint8_t)rx[3 + i];
                }
            } else {                                       // grey: every byte to three channels
                uint8_t* q = dst + ((size_t)row * width + x0) * 3;
                if (nvalid == PNG_GROUP) {
                    unsigned o[9];
#pragma unroll
                    for (int m = 0; m < 3 * PNG_GROUP; ++m) {
                        if ((m & 3) == 0) o[m >> 2] = 0;
                        o[m >> 2] |= rx[3 + m / 3] << (8 * (m & 3));
                    }
                    __builtin_memcpy(q, o, 3 * PNG_GROUP);
                } else {
#pragma unroll
                    for (int i = 0; i < PNG_GROUP; ++i)
                        if (i < nvalid) q[3 * i] = q[3 * i + 1] = q[3 * i + 2] = (uint8_t)rx[3 + i];
                }
            }
            if (lane == 63) {
#pragma unroll
                for (int k = 0; k < 3; ++k) ring[wave][j & 1][k] = rec[k];
                if (tid == PNG_THREADS - 1) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) line[3 * g + k] = rec[k];
                }
            }
        }
        __syncthreads();                                   // this step's ring and line entries, before the next step reads
        if (++g == period) g = 0, ++blk;
        request(queue[j]);
      }
    }
}

}  // namespace

extern "C" int refid_png_unfilter(const refid_png_unfilter_desc* d, void* stream) {
    REFID_CHECK(d, "png_unfilter: null descriptor");
    REFID_CHECK(d->rows && d->frames, "png_unfilter: rows / frames is null");
    REFID_CHECK(d->n_frames > 0 && d->height > 0 && d->width > 0, "png_unfilter: n_frames %d, height %d, width %d must be positive",
                d->n_frames, d->height, d->width);
    REFID_CHECK(d->channels == 1 || d->channels == 3, "png_unfilter: channels %d (1 or 3)", d->channels);
    REFID_CHECK((long long)d->width * d->channels <= REFID_PNG_MAX_ROW_BYTES,
                "png_unfilter: width*channels %lld exceeds the LDS line of %d bytes (use the host route)",
                (long long)d->width * d->channels, REFID_PNG_MAX_ROW_BYTES);
    REFID_CHECK(d->bands ? d->n_bands > 0 : d->n_bands == 0, "png_unfilter: n_bands %d with%s a band table", d->n_bands,
                d->bands ? "" : "out");
    const unsigned grid = (unsigned)(d->bands ? d->n_bands : d->n_frames);
    hipStream_t st = (hipStream_t)stream;
    if (d->channels == 3)
        hipLaunchKernelGGL(png_unfilter_kernel<3>, dim3(grid), dim3(PNG_THREADS), 0, st, d->rows, d->frames, d->bands, d->n_frames, d->height,
                           d->width);
    else
        hipLaunchKernelGGL(png_unfilter_kernel<1>, dim3(grid), dim3(PNG_THREADS), 0, st, d->rows, d->frames, d->bands, d->n_frames, d->height,
                           d->width);
    REFID_LAUNCH_CHECK("png_unfilter");
    return 0;
}
