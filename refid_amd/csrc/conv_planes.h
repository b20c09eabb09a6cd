// Operand planes of the reduced-precision MFMA forms: an fp32 value as a sum of bf16 / fp16 numbers, eight channels (one
// 16-byte MFMA fragment per plane) at a time.  Shared by the conv tiles that split their activations in registers
// (conv_wino6.hip, conv_split.hip, conv_pw.hip); the bf16 tiles take their vector types from here.
#pragma once
#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int OOB = -1;                 // voffset 0xFFFFFFFF: buffer loads return 0 (hardware range check)
// bytes in front of the fp16 planes of a weight packing: int scale exponent at byte 0, zeros (written by pack.hip's prepass)
constexpr int PACK_HEADER_BYTES = 64;

// v (8 fp32 channels) -> PL bf16 planes (h = rne(v), m = rne(v - h), l = v - h - m); the planes sum to v exactly for PL = 3
// (44 VALU) and to 2^-17 |v| for PL = 2
template <int PL, int N>
__device__ __forceinline__ void split8(const f32x4& v0, const f32x4& v1, f32x4 (&pl)[N]) {
    static_assert(PL >= 1 && PL <= 3 && PL <= N, "one to three planes");
    bf16x8 p0, p1, p2;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float v = k < 4 ? v0[k] : v1[k - 4];
        const __bf16 h = (__bf16)v;
        p0[k] = h;
        if (PL >= 2) {
            const float r = v - (float)h;
            const __bf16 m = (__bf16)r;
            p1[k] = m;
            if (PL == 3) p2[k] = (__bf16)(r - (float)m);
        }
    }
    pl[0] = __builtin_bit_cast(f32x4, p0);
    if constexpr (PL >= 2) pl[1] = __builtin_bit_cast(f32x4, p1);
    if constexpr (PL == 3) pl[2] = __builtin_bit_cast(f32x4, p2);
}

// v (8 fp32 channels, already scaled into fp16's range) -> two fp16 planes, h + l = v to 22 bits (20 VALU)
template <int N>
__device__ __forceinline__ void split8h(const f32x4& v0, const f32x4& v1, f32x4 (&pl)[N]) {
    static_assert(N >= 2, "two planes");
    f16x8 h, l;
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        const f32x2 ab = {k < 4 ? v0[k] : v1[k - 4], k < 4 ? v0[k + 1] : v1[k - 3]};
        const f16x2 hh = __builtin_convertvector(ab, f16x2);                  // v_cvt_pk_f16_f32 (RNE)
        const f32x2 r = ab - __builtin_convertvector(hh, f32x2);              // exact
        const f16x2 ll = __builtin_convertvector(r, f16x2);
        h[k] = hh[0]; h[k + 1] = hh[1];
        l[k] = ll[0]; l[k + 1] = ll[1];
    }
    pl[0] = __builtin_bit_cast(f32x4, h);
    pl[1] = __builtin_bit_cast(f32x4, l);
}

// v (8 fp32 channels, already scaled into fp16's range) -> ONE fp16 plane, rounded to nearest even (4 VALU)
template <int N>
__device__ __forceinline__ void round8h(const f32x4& v0, const f32x4& v1, f32x4 (&pl)[N]) {
    f16x8 h;
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        const f32x2 ab = {k < 4 ? v0[k] : v1[k - 4], k < 4 ? v0[k + 1] : v1[k - 3]};
        const f16x2 hh = __builtin_convertvector(ab, f16x2);                  // v_cvt_pk_f16_f32 (RNE)
        h[k] = hh[0]; h[k + 1] = hh[1];
    }
    pl[0] = __builtin_bit_cast(f32x4, h);
}
