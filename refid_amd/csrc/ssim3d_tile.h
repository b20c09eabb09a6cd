// The SSIM arithmetic of the reference's _ssim_3d (metrics/psnr_ssim.py:135-182) on one 16x16 tile with its 5-pixel halo:
// 11x11x11 separable Gaussian (sigma 1.5) over (H, W, C=3) with REPLICATE padding in all three axes, fp32.  One body for
// ssim3d_kernel and val_tail_kernel (io.hip) and score_u8_kernel (score.hip), which must give the same bits for the same
// staged values.
//
// The body is shared as TEXT (statement macros), not as device functions, on purpose.  This fp32 code runs under the
// compiler's default contraction, and which of its multiplies end up fused into an FMA is decided by the optimiser from
// the shape of the statements: behind a __forceinline__ function boundary the same statements came out with 18 more
// fused lanes per thread (counted in the gfx950 code of all three kernels), that is, with other roundings than the
// kernels had.  Expanded in place the statements are the ones io.hip always held, and the two kernels there compile to
// the instructions they compiled to before the body moved here.  tests/test_hip_score.py holds the new kernel to
// refid_ssim3d_u8 bit for bit, tests/test_hip_val_tail.py the two old ones to each other.
//   sA, sB  [3][26][27] the two frames' uint8 values as floats, plane c = R, G, B, row r = y0 - 5 + r clamped, column likewise
//   sH      [5][3][26][17] the horizontal pass of the five fields (a, b, a^2, b^2, ab)
//   k       the SsimConst kernel argument
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "workgroup.h"

struct SsimConst { float g[11]; float mc[3][3]; };

constexpr int SSIM_T = 16, SSIM_R = 5, SSIM_HS = SSIM_T + 2 * SSIM_R;          // 26

// horizontal pass, 5 fields; the caller synchronises before (sA, sB complete) and after (sH complete)
#define SSIM3D_HPASS(sA, sB, sH, k)                                                                                         \
    for (int e = threadIdx.x; e < 3 * SSIM_HS * SSIM_T; e += 256) {                                                         \
        const int c = e / (SSIM_HS * SSIM_T), r = (e / SSIM_T) % SSIM_HS, q = e % SSIM_T;                                   \
        float m1 = 0.f, m2 = 0.f, s11 = 0.f, s22 = 0.f, s12 = 0.f;                                                          \
        _Pragma("unroll")                                                                                                   \
        for (int j = 0; j < 11; ++j) {                                                                                      \
            const float va = sA[c][r][q + j], vb = sB[c][r][q + j], g = k.g[j];                                             \
            m1 += g * va; m2 += g * vb; s11 += g * va * va; s22 += g * vb * vb; s12 += g * va * vb;                         \
        }                                                                                                                   \
        sH[0][c][r][q] = m1; sH[1][c][r][q] = m2; sH[2][c][r][q] = s11; sH[3][c][r][q] = s22; sH[4][c][r][q] = s12;         \
    }

// vertical pass, channel-axis pass (replicate-padded) and the map of pixel (ty, tx) of the tile; declares `double acc` = the
// sum of the pixel's three map values, 0.0 where `inside` (an expression) is false
#define SSIM3D_PIXEL(acc, sH, k, ty, tx, inside)                                                                            \
    float v[5][3];                                                                                                          \
    _Pragma("unroll")                                                                                                       \
    for (int fi = 0; fi < 5; ++fi)                                                                                          \
        _Pragma("unroll")                                                                                                   \
        for (int c = 0; c < 3; ++c) {                                                                                       \
            float s = 0.f;                                                                                                  \
            _Pragma("unroll")                                                                                               \
            for (int j = 0; j < 11; ++j) s += k.g[j] * sH[fi][c][ty + j][tx];                                               \
            v[fi][c] = s;                                                                                                   \
        }                                                                                                                   \
    double acc = 0.0;                                                                                                       \
    if (inside) {                                                                                                           \
        const float C1 = (0.01f * 255.f) * (0.01f * 255.f), C2 = (0.03f * 255.f) * (0.03f * 255.f);                         \
        _Pragma("unroll")                                                                                                   \
        for (int c = 0; c < 3; ++c) {                                                                                       \
            float w[5];                                                                                                     \
            _Pragma("unroll")                                                                                               \
            for (int fi = 0; fi < 5; ++fi) w[fi] = k.mc[c][0] * v[fi][0] + k.mc[c][1] * v[fi][1] + k.mc[c][2] * v[fi][2];   \
            const float mu1 = w[0], mu2 = w[1];                                                                             \
            const float s1 = w[2] - mu1 * mu1, s2 = w[3] - mu2 * mu2, s12 = w[4] - mu1 * mu2;                               \
            acc += (double)(((2.f * mu1 * mu2 + C1) * (2.f * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))); \
        }                                                                                                                   \
    }

// The workgroup's sum of `acc` (one double per thread) in the fixed order of refid_block_sum (workgroup.h), which thread 0
// stores to `dst`.  sred: 4 doubles of LDS that nothing else uses in the kernel.
#define SSIM3D_BLOCK_SUM(acc, sred, dst)                                                                                    \
    { const double ssim_sum = refid_block_sum<double, 4>(acc, sred); if (threadIdx.x == 0) dst = ssim_sum; }

static inline SsimConst ssim_const() {
    SsimConst k;
    double g[11], s = 0.0;                                  // cv2.getGaussianKernel(11, 1.5)
    for (int i = 0; i < 11; ++i) { g[i] = exp(-((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); s += g[i]; }
    for (int i = 0; i < 11; ++i) { g[i] /= s; k.g[i] = (float)g[i]; }
    for (int c = 0; c < 3; ++c) {                           // 11 taps along the 3-channel axis, replicate padding
        double m[3] = {0, 0, 0};
        for (int j = 0; j < 11; ++j) { int cc = c + j - 5; cc = cc < 0 ? 0 : (cc > 2 ? 2 : cc); m[cc] += g[j]; }
        for (int q = 0; q < 3; ++q) k.mc[c][q] = (float)m[q];
    }
    return k;
}
