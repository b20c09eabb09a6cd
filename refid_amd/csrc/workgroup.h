// The reductions the non-GEMM kernels share: one wave sum, one workgroup sum, one workgroup exclusive scan.  The ORDER of
// the additions is part of each contract: floating-point callers (train.hip, io.hip, score.hip, ssim3d_tile.h, egaca.hip)
// are pinned to their references in exactly this order, and a fixed order is what makes a logged loss or score
// independent of how workgroups arrive.  All three are for whole waves of 64 lanes with every lane taking part.
//
// Not here, on purpose: the sums whose tree runs the other way, offsets 1, 2, .. 32 (vn_block_sum in voxel_norm.h, the
// moments of niqe.hip) -- other roundings, pinned to other references; the partial trees of the conv and
// weight-gradient tiles; the max-reductions of pack.hip and conv_split.hip.
#pragma once
#include <hip/hip_runtime.h>

// Sum over the 64 lanes of a wave: xor tree with offsets 32, 16, 8, 4, 2, 1, that is
//   lane l first adds lane l ^ 32, then the sum of lane l ^ 16, ... ; every lane ends with the same total (same bits:
//   the two operands of each step are swapped between partners, and addition commutes).
template <class T>
__device__ __forceinline__ T refid_wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sum over a workgroup of NW waves: refid_wave_sum, lane 0 of wave w stores to sh[w], ONE barrier, then
// R(sh[0]) + sh[1] + ... + sh[NW-1] added left to right in R (the type of v, or a wider integer that keeps the total of
// the waves from wrapping).  Every thread gets the total.  sh: NW values of LDS.  There is no barrier in front of the
// store: a caller that uses sh a second time (or reads it elsewhere) puts its own barrier before the call.
template <class R, int NW, class T>
__device__ __forceinline__ R refid_block_sum(T v, T* sh) {
    v = refid_wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    R r = (R)sh[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) r += sh[w];
    return r;
}

// Exclusive prefix sum over a workgroup of NW waves in thread order (integers: the order is free); *total = the sum, in
// every thread.  red: NW words of LDS.  Two barriers: the first keeps the store to `red` behind the reads of the call
// before, the second publishes it -- so back-to-back calls may share one `red`, and whatever the caller wrote to LDS
// before the call is visible to every thread after it.
template <int NW>
__device__ __forceinline__ unsigned refid_block_scan(unsigned v, unsigned* red, unsigned* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    __syncthreads();                                           // (red may still be read from the call before)
    if (lane == 63) red[wave] = inc;
    __syncthreads();
    unsigned before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) before += w < wave ? red[w] : 0u, sum += red[w];
    *total = sum;
    return before + inc - v;
}
