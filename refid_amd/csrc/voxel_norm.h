// voxel_norm shared by the two assemblers (sample.hip: refid_voxel_norm and refid_assemble_single, sequence.hip:
// refid_seq_assemble_single): statistics over the non-zero elements of a sample, then (v - mean) / std on them.  One
// definition of the summation order and of the mean / std arithmetic, so that both produce the same bits by construction.
// The order and the arithmetic are described at the top of sample.hip and in include/refid_hip.h.
#pragma once
#include <cstdint>

#include "common.h"
#include "event_fixed.h"

namespace {

constexpr int VN_CHUNK = 4096;                 // elements per workgroup of the statistics pass: 256 threads x 16
constexpr double VN_TWO_M32 = 1.0 / 4294967296.0;

// In = float: the element itself, S1 in float64 (same tree as S2).  In = long long: the scatter's fixed-point sum,
// v = fixed_to_float(a), S1 as the exact integer sum of v * 2^32.
template <class In> struct VoxelIn;
template <> struct VoxelIn<float> {
    typedef double S1;
    static __device__ __forceinline__ float value(float a) { return a; }
    static __device__ __forceinline__ double term(float v) { return (double)v; }
    static __device__ __forceinline__ double sum(double s1) { return s1; }
};
template <> struct VoxelIn<long long> {
    typedef long long S1;
    static __device__ __forceinline__ float value(long long a) { return fixed_to_float(a); }
    static __device__ __forceinline__ long long term(float v) { return (long long)(v * REFID_TWO32); }   // exact
    static __device__ __forceinline__ double sum(long long s1) { return (double)s1 * VN_TWO_M32; }
};

// fixed xor tree over the 64 lanes (adjacent pairs first), then the four waves in index order; the total is in thread 0
// (offsets 1, 2, .. 32: the other way round than refid_block_sum of workgroup.h, and pinned to its reference in this order)
template <class T>
__device__ __forceinline__ T vn_block_sum(T v, T* sh) {
#pragma clang fp contract(off)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __syncthreads();
    return v;
}

// grid = (chunks of the sample, batch); parts[(b * chunks + c) * 3 + {0, 1, 2}] = S0, S1, S2 of chunk c of sample b
template <class In>
__global__ __launch_bounds__(256) void voxel_stats_kernel(const In* __restrict__ in, long long per_sample,
                                                         unsigned long long* __restrict__ parts) {
#pragma clang fp contract(off)
    typedef typename VoxelIn<In>::S1 S1;
    __shared__ unsigned long long sh[4];
    const In* src = in + (long long)blockIdx.y * per_sample;
    const long long base = (long long)blockIdx.x * VN_CHUNK + threadIdx.x;
    long long s0 = 0;
    S1 s1 = 0;
    double s2 = 0.0;
#pragma unroll 4
    for (int k = 0; k < VN_CHUNK / 256; ++k) {
        const long long e = base + k * 256;
        if (e >= per_sample) break;
        const float v = VoxelIn<In>::value(src[e]);
        s0 += v != 0.f;
        s1 += VoxelIn<In>::term(v);
        s2 += (double)v * (double)v;
    }
    s0 = vn_block_sum(s0, reinterpret_cast<long long*>(sh));
    s1 = vn_block_sum(s1, reinterpret_cast<S1*>(sh));
    s2 = vn_block_sum(s2, reinterpret_cast<double*>(sh));
    if (threadIdx.x == 0) {
        unsigned long long* p = parts + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 3;
        p[0] = (unsigned long long)s0;
        __builtin_memcpy(p + 1, &s1, 8);
        __builtin_memcpy(p + 2, &s2, 8);
    }
}

// One thread sums the `chunks` partials of a sample (p: its first word) in index order: mean64 = S1/S0,
// var64 = S2/S0 - mean64^2, ms = {(float)mean64, (float)sqrt(var64)}.  False -- the sample comes out all zeros -- when
// S0 == 0, var64 <= 0 or the fp32 std is 0.
template <class In>
__device__ __forceinline__ bool vn_mean_std(const unsigned long long* __restrict__ p, int chunks, float* ms) {
#pragma clang fp contract(off)
    typedef typename VoxelIn<In>::S1 S1;
    long long s0 = 0;
    S1 s1 = 0;
    double s2 = 0.0;
    for (int c = 0; c < chunks; ++c) {
        S1 t1;
        double t2;
        __builtin_memcpy(&t1, p + c * 3ll + 1, 8);
        __builtin_memcpy(&t2, p + c * 3ll + 2, 8);
        s0 += (long long)p[c * 3ll];
        s1 += t1;
        s2 += t2;
    }
    const double n = (double)s0;
    const double mean = VoxelIn<In>::sum(s1) / n;
    const double var = s2 / n - mean * mean;
    const float std_f = (float)sqrt(var);
    ms[0] = (float)mean;
    ms[1] = std_f;
    return s0 > 0 && var > 0.0 && std_f != 0.f;
}

// out = v != 0 ? (v - mean_f) / std_f : 0 on V elements: one fp32 subtraction and one IEEE fp32 division
template <int V>
__device__ __forceinline__ void vn_apply(float* v, bool ok, float mean_f, float std_f) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = (ok && v[k] != 0.f) ? (v[k] - mean_f) / std_f : 0.f;
}

// grid = (chunks of the sample, batch); one thread = V consecutive elements.  parts == nullptr: conversion only.
// Every workgroup sums the sample's partials itself (vn_mean_std).
template <class In, int V>
__global__ __launch_bounds__(256) void voxel_apply_kernel(const In* in, float* out,                   // (out may be in)
                                                         long long per_sample, const unsigned long long* __restrict__ parts,
                                                         int chunks) {
#pragma clang fp contract(off)
    __shared__ float sh_ms[2];
    __shared__ int sh_ok;
    const int b = blockIdx.y;
    if (parts && threadIdx.x == 0) sh_ok = vn_mean_std<In>(parts + (long long)b * chunks * 3, chunks, sh_ms);
    __syncthreads();
    const long long e = (blockIdx.x * 256ll + threadIdx.x) * V;
    if (e >= per_sample) return;
    const In* src = in + (long long)b * per_sample + e;
    float v[V];
    if constexpr (V == 4 && sizeof(In) == 8) {
        const longlong2 a0 = *reinterpret_cast<const longlong2*>(src), a1 = *reinterpret_cast<const longlong2*>(src + 2);
        v[0] = VoxelIn<In>::value(a0.x); v[1] = VoxelIn<In>::value(a0.y);
        v[2] = VoxelIn<In>::value(a1.x); v[3] = VoxelIn<In>::value(a1.y);
    } else if constexpr (V == 4) {
        const float4 a = *reinterpret_cast<const float4*>(src);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else {
        v[0] = VoxelIn<In>::value(src[0]);
    }
    if (parts) vn_apply<V>(v, sh_ok != 0, sh_ms[0], sh_ms[1]);
    store_v<V>(out + (long long)b * per_sample + e, v);
}

static inline long long vn_chunks(long long per_sample) { return (per_sample + VN_CHUNK - 1) / VN_CHUNK; }

// statistics (stats) and / or normalisation (apply; parts == nullptr: conversion only) of `batch` samples, one launch each
template <class In>
int voxel_norm_launch(const In* in, float* out, int batch, long long per_sample, void* parts, bool stats, bool apply,
                      hipStream_t st, const char* what) {
    const long long chunks = vn_chunks(per_sample);
    unsigned long long* p = static_cast<unsigned long long*>(parts);
    if (stats) {
        hipLaunchKernelGGL(voxel_stats_kernel<In>, dim3((unsigned)chunks, batch), dim3(256), 0, st, in, per_sample, p);
        REFID_LAUNCH_CHECK(what);
    }
    if (apply) {
        const bool vec = (per_sample & 3) == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
        const unsigned nb = (unsigned)(((vec ? per_sample / 4 : per_sample) + 255) / 256);
        if (vec) hipLaunchKernelGGL((voxel_apply_kernel<In, 4>), dim3(nb, batch), dim3(256), 0, st, in, out, per_sample, p, (int)chunks);
        else hipLaunchKernelGGL((voxel_apply_kernel<In, 1>), dim3(nb, batch), dim3(256), 0, st, in, out, per_sample, p, (int)chunks);
        REFID_LAUNCH_CHECK(what);
    }
    return 0;
}

}  // namespace
