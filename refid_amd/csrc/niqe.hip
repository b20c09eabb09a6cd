// NIQE moments (basicsr/metrics/niqe.py: calculate_niqe -> niqe -> compute_feature -> estimate_aggd_param) on the uint8
// frames that refid_val_tail leaves on the device: everything per pixel, for both scales, in one pass per scale.
//
// One workgroup of 256 threads owns one block of one frame at one scale (96x96 at scale 1, 48x48 at scale 2):
//   A  the Y tile with its 3-pixel halo goes into LDS straight from the uint8 frame (byte loads: a row is 3*w bytes,
//      which is aligned to nothing); coordinates are clamped at the edges of the cropped image, not of the block.  At
//      scale 2 a tile element is the float32 2x2 mean of four Y values, which are recomputed from the frame (the second
//      read of the frame comes out of L2).
//   B  per pixel the two 49-tap float64 sums (taps in row-major order from a zero accumulator, one rounded product and
//      one rounded add per tap), rounded to float32, and the float32 normalisation; the map goes into LDS.
//   C  the five maps -- n and n * roll(n, s), the roll wrapping inside the block: an LDS index -- and their five sums per
//      map, in float64: each thread adds its pixels in index order, the 64 lanes of a wave by the xor tree 1, 2, .., 32,
//      the four waves in order.  No atomics; the bits do not depend on the run, the frame's place in the call or nf.
// Every float operation is a single correctly rounded one: contraction is off for this file (hipcc fuses by default),
// fp32 division and square root are the IEEE ones, checked in the emitted code: v_div_scale / v_div_fmas / v_div_fixup for
// the divisions, and for sqrtf the v_sqrt_f32 whose two neighbours are tried against fma residuals (the only fused
// operations in the file are those inside these two expansions and the float64 division's).
#include "common.h"
#include "y_plane.h"

#pragma clang fp contract(off)

namespace {

constexpr int NQ_THREADS = 256;
constexpr int NQ_HALO = 3;
constexpr int NQ_ENTRIES = 25;                             // 5 maps x {count<0, count>0, sum_{<0} x^2, sum_{>0} x^2, sum |x|}

template <int BS>
constexpr int niqe_lds_bytes() {
    return (NQ_THREADS / 64) * NQ_ENTRIES * 8 + ((BS + 2 * NQ_HALO) * (BS + 2 * NQ_HALO) + BS * BS) * 4;
}

// to_y_channel after astype(float32): fl32(fl32(y64 / 255) * 255), y64 in float64 from the fl32(u8 / 255) channels
__device__ __forceinline__ float niqe_y(const unsigned char* __restrict__ p, int bgr) {
    const float c0 = (float)p[0], c1 = (float)p[1], c2 = (float)p[2];
    return refid_y601_u8(bgr ? c2 : c0, c1, bgr ? c0 : c2);        // y_plane.h: shared with score.hip
}

template <int BS, int SCALE>
__global__ __launch_bounds__(NQ_THREADS) void niqe_moments_kernel(const unsigned char* __restrict__ frames, int h, int w,
                                                                  int hc, int wc, int cb, int bgr,
                                                                  const double* __restrict__ window, double* __restrict__ sums,
                                                                  float* __restrict__ y_out, float* __restrict__ n_out) {
    constexpr int TS = BS + 2 * NQ_HALO;
    constexpr int PER_THREAD = BS * BS / NQ_THREADS;
    static_assert(BS * BS % NQ_THREADS == 0, "whole rounds of the workgroup");
    extern __shared__ __align__(16) unsigned char niqe_smem[];
    double* red = reinterpret_cast<double*>(niqe_smem);                    // [4 waves][25]
    float* ty = reinterpret_cast<float*>(red + (NQ_THREADS / 64) * NQ_ENTRIES);   // [TS][TS]
    float* tn = ty + TS * TS;                                              // [BS][BS]

    const int tid = threadIdx.x;
    const int nbh = hc / 96, nbw = wc / 96, nb = nbh * nbw;
    const int f = blockIdx.x / nb, blk = blockIdx.x % nb;                  // blocks are width-major, as the reference walks them
    const int by0 = (blk % nbh) * BS, bx0 = (blk / nbh) * BS;
    const int hs = hc / SCALE, ws = wc / SCALE;                            // this scale's image
    const unsigned char* frame = frames + (long long)f * h * w * 3;

    for (int i = tid; i < TS * TS; i += NQ_THREADS) {
        const int r = i / TS, c = i % TS;
        const int gy = min(max(by0 - NQ_HALO + r, 0), hs - 1), gx = min(max(bx0 - NQ_HALO + c, 0), ws - 1);
        float y;
        if (SCALE == 1) {
            y = niqe_y(frame + ((long long)(cb + gy) * w + (cb + gx)) * 3, bgr);
            if (y_out && r >= NQ_HALO && r < NQ_HALO + BS && c >= NQ_HALO && c < NQ_HALO + BS)
                y_out[((long long)f * hc + gy) * wc + gx] = y;
        } else {
            const unsigned char* p = frame + ((long long)(cb + 2 * gy) * w + (cb + 2 * gx)) * 3;
            const float v00 = __fdiv_rn(niqe_y(p, bgr), 255.f), v01 = __fdiv_rn(niqe_y(p + 3, bgr), 255.f);
            const float v10 = __fdiv_rn(niqe_y(p + (long long)w * 3, bgr), 255.f);
            const float v11 = __fdiv_rn(niqe_y(p + (long long)w * 3 + 3, bgr), 255.f);
            const float top = v00 * 0.5f + v01 * 0.5f, bot = v10 * 0.5f + v11 * 0.5f;
            y = (top * 0.5f + bot * 0.5f) * 255.f;
        }
        ty[i] = y;
    }
    __syncthreads();

    for (int k = 0; k < PER_THREAD; ++k) {
        const int idx = tid + k * NQ_THREADS, py = idx / BS, px = idx % BS;
        const float* t = ty + py * TS + px;
        double mu64 = 0.0, sq64 = 0.0;
#pragma unroll
        for (int i = 0; i < 7; ++i)
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                const double wk = window[i * 7 + j];
                const float x = t[i * TS + j];
                mu64 = mu64 + wk * (double)x;
                sq64 = sq64 + wk * (double)(x * x);
            }
        const float mu = (float)mu64, sq = (float)sq64;
        const float sigma = sqrtf(fabsf(sq - mu * mu));         // (not __fsqrt_rn: that one is the bare 1-ulp v_sqrt_f32)
        const float n = __fdiv_rn(t[NQ_HALO * TS + NQ_HALO] - mu, sigma + 1.f);
        tn[idx] = n;
        if (n_out) n_out[((long long)f * hs + by0 + py) * ws + bx0 + px] = n;
    }
    __syncthreads();

    double acc[5][3];
    int cnt[5][2];
#pragma unroll
    for (int m = 0; m < 5; ++m) {
        acc[m][0] = acc[m][1] = acc[m][2] = 0.0;
        cnt[m][0] = cnt[m][1] = 0;
    }
    for (int k = 0; k < PER_THREAD; ++k) {
        const int idx = tid + k * NQ_THREADS, py = idx / BS, px = idx % BS;
        const int pym = (py ? py : BS) - 1, pxm = (px ? px : BS) - 1, pxp = px + 1 == BS ? 0 : px + 1;
        const float n = tn[idx];
        // np.roll(block, (sy, sx))[i, j] = block[i - sy, j - sx] for the shifts (0,1), (1,0), (1,1), (1,-1)
        const float v[5] = {n, n * tn[py * BS + pxm], n * tn[pym * BS + px], n * tn[pym * BS + pxm], n * tn[pym * BS + pxp]};
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            const double x = (double)v[m], s = x * x;                      // the square of a float is exact in float64
            cnt[m][0] += v[m] < 0.f;
            cnt[m][1] += v[m] > 0.f;
            acc[m][0] = acc[m][0] + (v[m] < 0.f ? s : 0.0);
            acc[m][1] = acc[m][1] + (v[m] > 0.f ? s : 0.0);
            acc[m][2] = acc[m][2] + fabs(x);
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int m = 0; m < 5; ++m) {
        double e[5] = {(double)cnt[m][0], (double)cnt[m][1], acc[m][0], acc[m][1], acc[m][2]};
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            // (offsets 1, 2, .. 32: the other way round than refid_wave_sum of workgroup.h, and pinned to its reference in this order)
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) e[q] = e[q] + __shfl_xor(e[q], o, 64);
            if (lane == 0) red[wave * NQ_ENTRIES + m * 5 + q] = e[q];
        }
    }
    __syncthreads();
    if (tid < NQ_ENTRIES) {
        double total = red[tid];
        for (int wv = 1; wv < NQ_THREADS / 64; ++wv) total = total + red[wv * NQ_ENTRIES + tid];
        sums[(((long long)f * 2 + (SCALE - 1)) * nb + blk) * NQ_ENTRIES + tid] = total;
    }
}

std::atomic<unsigned long long> niqe_lds_done_1{0}, niqe_lds_done_2{0};

}  // namespace

// Every workgroup finishes its own block: the call needs no partials.
extern "C" long long refid_niqe_moments_parts(int n_frames, int h, int w) { return 0; }

extern "C" int refid_niqe_moments(const unsigned char* frames_u8, int n_frames, int h, int w, int flags, int crop_border,
                                  const double* window49, double* sums, void* parts, float* y_out, float* mscn1_out,
                                  float* mscn2_out, void* stream) {
    REFID_CHECK(frames_u8 && window49 && sums && n_frames > 0 && h > 0 && w > 0, "niqe_moments: bad arguments");
    REFID_CHECK((flags & ~REFID_NIQE_BGR) == 0, "niqe_moments: unknown flags 0x%x", flags);
    REFID_CHECK(crop_border >= 0 && crop_border < 0x3fffffff, "niqe_moments: crop_border %d", crop_border);
    const long long hb = (long long)h - 2ll * crop_border, wb = (long long)w - 2ll * crop_border;
    REFID_CHECK(hb >= 96 && wb >= 96, "niqe_moments: a %dx%d frame with crop_border %d holds no 96x96 block", h, w, crop_border);
    const int hc = (int)(hb / 96) * 96, wc = (int)(wb / 96) * 96;
    const long long blocks = (long long)n_frames * (hc / 96) * (wc / 96);
    REFID_CHECK(blocks <= 0x7fffffffll, "niqe_moments: %lld blocks exceed the grid (n_frames=%d, %dx%d)", blocks, n_frames, h, w);
    hipStream_t st = (hipStream_t)stream;
    const int bgr = (flags & REFID_NIQE_BGR) ? 1 : 0;
    constexpr int lds1 = niqe_lds_bytes<96>(), lds2 = niqe_lds_bytes<48>();
    if (int rc = refid_lds_attr_once(niqe_lds_done_1, niqe_moments_kernel<96, 1>, lds1, "niqe_moments")) return rc;
    if (int rc = refid_lds_attr_once(niqe_lds_done_2, niqe_moments_kernel<48, 2>, lds2, "niqe_moments")) return rc;
    hipLaunchKernelGGL((niqe_moments_kernel<96, 1>), dim3((unsigned)blocks), dim3(NQ_THREADS), lds1, st, frames_u8, h, w, hc, wc,
                       crop_border, bgr, window49, sums, y_out, mscn1_out);
    REFID_LAUNCH_CHECK("niqe_moments/scale1");
    hipLaunchKernelGGL((niqe_moments_kernel<48, 2>), dim3((unsigned)blocks), dim3(NQ_THREADS), lds2, st, frames_u8, h, w, hc, wc,
                       crop_border, bgr, window49, sums, (float*)nullptr, mscn2_out);
    REFID_LAUNCH_CHECK("niqe_moments/scale2");
    return 0;
}
