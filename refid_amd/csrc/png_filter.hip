// PNG forward filtering (PNG specification 9.2) of resident uint8 RGB frames, with libpng's adaptive heuristic: the half of
// an encoder that is a streaming pass over bytes.  Deflate is the host's (refid_amd/png.py: encode_png_rows) or png_deflate.hip's.  The
// mirror image of png.hip: forward filtering reads original pixels only -- a = the byte 3 to the left, b = the byte above,
// c = the byte above-left, 0 outside the frame -- so no row waits for another.
//
// One wave owns one row of one frame; (frame, row) is folded into blockIdx.x, PNGF_WAVES rows per workgroup.  The waves of
// a workgroup share nothing: no LDS, no barrier, no atomics.
//   - A row is cut into UNITS of four output bytes at the 4-byte-aligned addresses of the OUTPUT (whose pitch 1 + 3W is
//     odd, so every row starts somewhere else): unit u holds body bytes i0 .. i0+3 with i0 = head - 4 + 4u, head = the 0..3
//     bytes in front of the first aligned address.  Lane l takes units l, l+64, ...: a wave instruction covers 256
//     contiguous bytes on both sides.  A unit needs x[i0-3 .. i0+3] of its row and of the row above: two 8-byte loads the
//     compiler is told nothing about the alignment of; where the window crosses an end of the row (the first two units,
//     the last one) it is gathered byte by byte with every index checked, so nothing outside the two rows is read.
//   - Pass 1 sums |residual as int8| of the five types over the row: a uint32 per type and lane, then a fixed xor-shuffle
//     tree (integers: the order is free); every lane ends with the five totals.  The least wins, the lowest type on a tie.
//   - Pass 2 reads the row again -- it was just read by the same wave, so this comes out of L1 / L2 -- and writes the one
//     chosen residual.  The five candidates of a row are NOT kept in registers: a 1280-pixel row would take 75 VGPRs per
//     lane for them, a 32760-byte one more than a wave has, and the row length would have to be a compile-time bound.
//     Hence no width limit from the kernel's structure (REFID_PNG_FILTER_MAX_WIDTH only keeps a cost sum inside uint32).
//     A fixed mode without `costs` skips pass 1.
//   - Stores: a whole unit is one aligned dword store.  The filter byte, the head and the tail of a row -- the bytes that
//     share a word with the neighbouring row -- are single byte stores by the one lane that owns them, never a
//     read-modify-write of the word: no two waves write the same byte, nothing is written outside
//     [rows, rows + N*H*pitch), and any alignment of `rows` works.
// Integer arithmetic modulo 256 only: the bytes are defined by the specification, the choice by the sums.
#include "common.h"
#include "workgroup.h"

namespace {

constexpr int PNGF_WAVES = 4;                               // rows per workgroup: one wave per SIMD

// bytes i0-4 .. i0+3 of a row of `stride` bytes as one little-endian word (byte m = row[i0 - 4 + m]), 0 outside the row
__device__ __forceinline__ unsigned long long pngf_window(const uint8_t* __restrict__ row, int i0, int stride) {
    unsigned long long v = 0;
    if (i0 >= 4 && i0 + 4 <= stride) {
        __builtin_memcpy(&v, row + i0 - 4, 8);
    } else {
#pragma unroll
        for (int m = 1; m < 8; ++m) {                          // (byte 0 is never used)
            const int i = i0 - 4 + m;
            if (i >= 0 && i < stride) v |= (unsigned long long)row[i] << (8 * m);
        }
    }
    return v;
}

__device__ __forceinline__ unsigned pngf_paeth(unsigned a, unsigned b, unsigned c) {
    const int p = (int)a + (int)b - (int)c;
    const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);                // ties: a, then b, then c
}

// the five residuals of byte k (0..3) of a unit from its windows: cur = this row, up = the row above
__device__ __forceinline__ void pngf_residuals(unsigned long long cur, unsigned long long up, int k, unsigned (&r)[5]) {
    const unsigned x = (unsigned)(cur >> (8 * (k + 4))) & 0xffu, a = (unsigned)(cur >> (8 * (k + 1))) & 0xffu;
    const unsigned b = (unsigned)(up >> (8 * (k + 4))) & 0xffu, c = (unsigned)(up >> (8 * (k + 1))) & 0xffu;
    r[0] = x;
    r[1] = (x - a) & 0xffu;
    r[2] = (x - b) & 0xffu;
    r[3] = (x - ((a + b) >> 1)) & 0xffu;
    r[4] = (x - pngf_paeth(a, b, c)) & 0xffu;
}

__global__ __launch_bounds__(64 * PNGF_WAVES) void png_filter_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ rows,
                                                                 unsigned* __restrict__ costs, long long n_rows, int height,
                                                                 int width, int mode) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * PNGF_WAVES + (threadIdx.x >> 6);       // frame * height + row
    if (r >= n_rows) return;                                   // (wave-uniform; the waves share nothing)
    const int stride = 3 * width;
    const bool top = r % height == 0;                          // row 0 of a frame never reads the frame before
    const uint8_t* cur_row = frames + r * stride;
    const uint8_t* up_row = cur_row - (top ? 0 : stride);      // (never read when top)
    uint8_t* out = rows + r * ((long long)stride + 1);         // the filter byte; the body follows
    const int head = min((int)((4 - ((unsigned long long)(out + 1) & 3)) & 3), stride);
    const int units = 1 + (stride - head + 3) / 4;             // unit 0: the head (maybe empty); the last may be partial

    int ft = mode;
    if (mode == 5 || costs) {
        unsigned sum[5] = {0, 0, 0, 0, 0};
        for (int u = lane; u < units; u += 64) {
            const int i0 = head - 4 + 4 * u;
            const unsigned long long cur = pngf_window(cur_row, i0, stride);
            const unsigned long long up = top ? 0ull : pngf_window(up_row, i0, stride);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                unsigned res[5];
                pngf_residuals(cur, up, k, res);
                const bool valid = i0 + k >= 0 && i0 + k < stride;
#pragma unroll
                for (int t = 0; t < 5; ++t) {
                    const unsigned mag = res[t] < 128u ? res[t] : 256u - res[t];            // |residual read as int8|
                    sum[t] += valid ? mag : 0u;
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            sum[t] = refid_wave_sum(sum[t]);
        }
        if (costs && lane < 5) {
            unsigned v = sum[0];
#pragma unroll
            for (int t = 1; t < 5; ++t) v = lane == t ? sum[t] : v;
            costs[r * 5 + lane] = v;
        }
        if (mode == 5) {
            ft = 0;
            unsigned best = sum[0];
#pragma unroll
            for (int t = 1; t < 5; ++t)
                if (sum[t] < best) best = sum[t], ft = t;      // strictly less: the lowest type wins a tie
        }
    }

    if (lane == 0) out[0] = (uint8_t)ft;
    uint8_t* body = out + 1;
    for (int u = lane; u < units; u += 64) {
        const int i0 = head - 4 + 4 * u;
        const unsigned long long cur = pngf_window(cur_row, i0, stride);
        const unsigned long long up = (top || ft < 2) ? 0ull : pngf_window(up_row, i0, stride);
        unsigned word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            unsigned res[5];
            pngf_residuals(cur, up, k, res);
            unsigned v = res[0];
#pragma unroll
            for (int t = 1; t < 5; ++t) v = ft == t ? res[t] : v;
            word |= v << (8 * k);
        }
        if (i0 >= 0 && i0 + 4 <= stride) {
            *reinterpret_cast<unsigned*>(body + i0) = word;    // aligned: body + head is, and i0 - head is a multiple of 4
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i0 + k >= 0 && i0 + k < stride) body[i0 + k] = (uint8_t)(word >> (8 * k));
        }
    }
}

}  // namespace

extern "C" int refid_png_filter(const refid_png_filter_desc* d, void* stream) {
    REFID_CHECK(d, "png_filter: null descriptor");
    REFID_CHECK(d->frames && d->rows, "png_filter: frames / rows is null");
    REFID_CHECK(d->n_frames > 0 && d->height > 0 && d->width > 0, "png_filter: n_frames %d, height %d, width %d must be positive",
                d->n_frames, d->height, d->width);
    REFID_CHECK(d->mode >= 0 && d->mode <= REFID_PNG_FILTER_ADAPTIVE, "png_filter: mode %d (0..4 a filter type, 5 adaptive)", d->mode);
    REFID_CHECK(d->width <= REFID_PNG_FILTER_MAX_WIDTH, "png_filter: width %d exceeds %d (a row's cost sum would leave uint32)",
                d->width, REFID_PNG_FILTER_MAX_WIDTH);
    REFID_CHECK(((unsigned long long)d->costs & 3ull) == 0, "png_filter: costs is not aligned to 4 bytes");
    const long long n_rows = (long long)d->n_frames * d->height;
    const long long blocks = (n_rows + PNGF_WAVES - 1) / PNGF_WAVES;
    // (grid x block stays below 2^32 threads)
    REFID_CHECK(blocks <= 0xffffffll, "png_filter: %lld rows exceed the grid (n_frames=%d, height=%d)", n_rows, d->n_frames, d->height);
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)blocks), dim3(64 * PNGF_WAVES), 0, (hipStream_t)stream, d->frames, d->rows,
                       d->costs, n_rows, d->height, d->width, d->mode);
    REFID_LAUNCH_CHECK("png_filter");
    return 0;
}
