// The conv tiles' fused epilogue (refid_conv_desc), stated once for conv_igemm / conv_wino (+ the split-K finishing kernel) /
// conv_wino6 / conv_split / conv_pw:
//     out = mask( post( pre(acc + bias) + res [+ res2] ) ),   out2 = out + add2
// on one fp32 channel quad v of GEMM columns j0 .. j0+3 of one output pixel.  vec = the quad is whole and every tensor takes
// 16-byte accesses; otherwise a scalar tail that stops at Cout.  Every step is one fp32 operation in this order -- the bits
// are part of the contract (tests/test_hip_conv_epilogue.py).
//
// A tile calls conv_epilogue(), or -- where it loads the bias once for several pixels, or keeps an ablation branch between the
// steps -- the pieces it is made of: epi_bias4, epi_pre, epi_tail.  WHERE the quad's tensors live is the caller's:
//   EpiAtOp     tensor + op * ld + c                    (pixel index op, channel c: every tile but one)
//   EpiSteps    one base per tensor and thread + workgroup-uniform row / column steps (conv_wino6.hip: a per-item offset
//               product was as much vector-issue time as its K loop at 64 input channels)
// Addresses are formed only where a tensor is present, under the same conditions as the loads.
#pragma once
#include "common.h"
#include "conv_args.h"

enum EpiTensor { EPI_OUT, EPI_RES, EPI_MASK, EPI_OUT2, EPI_ADD2, EPI_TENSORS };

__device__ __forceinline__ float* epi_base(const ConvKArgs& a, int t) {
    return t == EPI_OUT ? a.out : t == EPI_RES ? const_cast<float*>(a.res) : t == EPI_MASK ? const_cast<float*>(a.mask)
         : t == EPI_OUT2 ? a.out2 : const_cast<float*>(a.add2);
}
__device__ __forceinline__ int epi_ld(const ConvKArgs& a, int t) {
    return t == EPI_OUT ? a.ldO : t == EPI_RES ? a.ldR : t == EPI_MASK ? a.ldM : t == EPI_OUT2 ? a.ldO2 : a.ldA2;
}
__device__ __forceinline__ f32x4 epi_load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

struct EpiAtOp {
    long long op; int c;
    __device__ __forceinline__ float* operator()(const ConvKArgs& a, int t) const { return epi_base(a, t) + op * epi_ld(a, t) + c; }
};

// a thread's items are pixels (row r, column block cb) of ITS channel quad: base + r * step[0] + cb * step[1], steps uniform
struct EpiSteps {
    float* base[EPI_TENSORS]; int step[EPI_TENSORS][2];
    // out0: a.out, or the split-K partial output; opb: the thread's first pixel; steps in pixels; two: the second output is on
    __device__ __forceinline__ EpiSteps(const ConvKArgs& a, float* out0, long long opb, int c, int rowPix, int colPix, bool two) {
#pragma unroll
        for (int t = 0; t < EPI_TENSORS; ++t) {
            float* const b = t == EPI_OUT ? out0 : epi_base(a, t);
            const bool on = b != nullptr && (t < EPI_OUT2 || two);
            base[t] = on ? b + opb * epi_ld(a, t) + c : nullptr;
            step[t][0] = rowPix * epi_ld(a, t); step[t][1] = colPix * epi_ld(a, t);
        }
    }
    __device__ __forceinline__ float* at(int t, int r, int cb) const { return base[t] + r * step[t][0] + cb * step[t][1]; }
};
struct EpiAtSteps {
    const EpiSteps& s; int r, cb;
    __device__ __forceinline__ float* operator()(const ConvKArgs&, int t) const { return s.at(t, r, cb); }
};

// bias quad of GEMM columns j0 .. j0+3 from a.bias + bidx (a.coBase + j0; the real channel under the pixel shuffle); zeros
// without a bias and past Cout
__device__ __forceinline__ f32x4 epi_bias4(const ConvKArgs& a, int bidx, int j0, bool vec) {
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (a.bias) {
        const float* bp = a.bias + bidx;
        if (vec) bv = epi_load4(bp);
        else
#pragma unroll
            for (int k = 0; k < 4; ++k) if (j0 + k < a.Cout) bv[k] = bp[k];
    }
    return bv;
}

__device__ __forceinline__ void epi_pre(const ConvKArgs& a, f32x4& v) { lrelu4(v, a.slopePre, a.slopePre != 1.f); }

// activation-derivative mask: LeakyReLU' of the stashed activation; GELU (the pointwise tile, maskMode 1): GELU_erf'(mask)
template <bool GELU>
__device__ __forceinline__ float epi_mask(const ConvKArgs& a, float x, float m) {
    if (GELU && a.maskMode == 1) return x * gelu_d(m);          // (workgroup-uniform)
    return x * ((m > 0.f) ? 1.f : a.slopeMask);
}

// v = pre(acc + bias) -> + res (prefetched: pres / pmask hold the quad's residual and mask) [+ the quad at res2] -> post ->
// mask -> out, out2 = out + add2.  Leaves the stored quad in v (vec).
template <bool GELU = false, class At>
__device__ __forceinline__ void epi_tail(const ConvKArgs& a, f32x4& v, int j0, bool vec, const At& at, bool pre = false,
                                         const f32x4& pres = f32x4{}, const f32x4& pmask = f32x4{}, const float* res2 = nullptr) {
    if (vec) {
        if (a.res) v += pre ? pres : epi_load4(at(a, EPI_RES));
        if (res2) v += epi_load4(res2);
        lrelu4(v, a.slopePost, a.slopePost != 1.f);
        if (a.mask) {
            const f32x4 mv = pre ? pmask : epi_load4(at(a, EPI_MASK));
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = epi_mask<GELU>(a, v[k], mv[k]);
        }
        *reinterpret_cast<f32x4*>(at(a, EPI_OUT)) = v;
        if (a.out2) *reinterpret_cast<f32x4*>(at(a, EPI_OUT2)) = v + epi_load4(at(a, EPI_ADD2));
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (j0 + k >= a.Cout) break;
            float t = v[k];
            if (a.res) t += at(a, EPI_RES)[k];
            t = lrelu(t, a.slopePost);
            if (a.mask) t = epi_mask<GELU>(a, t, at(a, EPI_MASK)[k]);
            at(a, EPI_OUT)[k] = t;
            if (a.out2) at(a, EPI_OUT2)[k] = t + at(a, EPI_ADD2)[k];
        }
    }
}

// The whole epilogue of one accumulator quad.  zeroBias: add the bias quad even when it is zeros (no bias) -- the tiles do,
// the split-K finishing kernel and the pointwise tile skip the add on their 16-byte path (x + 0 and x differ for x = -0)
template <bool GELU = false, class At>
__device__ __forceinline__ void conv_epilogue(const ConvKArgs& a, f32x4& v, int bidx, int j0, bool vec, const At& at,
                                              bool zeroBias = true, const float* res2 = nullptr) {
    if (zeroBias || !vec || a.bias) v += epi_bias4(a, bidx, j0, vec);
    epi_pre(a, v);
    epi_tail<GELU>(a, v, j0, vec, at, false, f32x4{}, f32x4{}, res2);
}
