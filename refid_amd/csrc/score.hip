// Full-reference scores of uint8 HWC frames that are already on the device (include/refid_hip.h, "Full-reference scores"):
// calculate_psnr / calculate_ssim of basicsr/metrics/psnr_ssim.py with crop_border and test_y_channel, per frame.
//
// One workgroup of 256 threads owns one 16x16 tile of one cropped frame; blockIdx.x = [frame][tile row][tile column]:
//   A  the rows of the tile (with its 5-pixel halo when an SSIM is asked for) are copied from both frames into LDS as
//      ALIGNED 4-byte words: the cropped origin and the 3*w pitch put a row segment at any byte address.  A word that holds
//      one byte of the buffer lies in that byte's page, so the up to 3 bytes read either side of a buffer are harmless; they
//      are never used;
//   B  the bytes are picked out of those words with the coordinates clamped to the cropped frame: into float planes R, G, B
//      (what ssim3d_kernel / val_tail_kernel stage from float frames) or into the two Y planes (y_plane.h);
//   C  per pixel the integer squared error and the 3-D SSIM body of ssim3d_tile.h, or fl32((Ya - Yb)^2) and the 121-tap
//      float64 SSIM of _ssim_cly; per tile one partial each, by a fixed tree (xor-shuffle inside a wave, the four waves in
//      order).  The partials are finished per frame by the fixed-order row sums.
// No atomics, nothing allocated; every loop count is known before the loop.
//
// The colour outputs (sq_rgb, ssim3d) and the Y outputs (sq_y, ssim_y, the taps) are two kernels of that one shape, and a
// kernel none of whose outputs is asked for is not launched.  They are apart because the 3-D SSIM must give the bits of
// refid_ssim3d_u8: which multiplies of that fp32 body the optimiser fuses depends on the code it stands next to
// (ssim3d_tile.h), and next to the float64 filter it came out differently (seen in the vectoriser's output), while next to
// the integer error alone it comes out as in io.hip.  The Y arithmetic is one correctly rounded operation per step:
// contraction is off inside those bodies.
#include "common.h"
#include "workgroup.h"
#include "ssim3d_tile.h"
#include "y_plane.h"

namespace {

constexpr int SC_T = SSIM_T, SC_R = SSIM_R, SC_HS = SSIM_HS;   // 16, 5, 26
constexpr int SC_RAW = 21;                                     // words per halo row: ceil((3 + 26*3 + 3) / 4)

struct ScoreConst { double win[121]; double c1, c2; };       // outer(g, g) row-major, (0.01*255)^2, (0.03*255)^2

// What both kernels know of their tile.
struct ScoreTile {
    long long f;                                               // frame
    int y0, x0;                                                // the tile's origin in the cropped frame
    int xs, nbytes;                                            // first halo column inside the cropped frame; bytes of a row segment
};

__device__ __forceinline__ ScoreTile score_tile(int tiles_x, int tiles_y, int wc) {
    ScoreTile t;
    const int tile = blockIdx.x % (tiles_x * tiles_y);
    t.f = blockIdx.x / (tiles_x * tiles_y);
    t.y0 = (tile / tiles_x) * SC_T;
    t.x0 = (tile % tiles_x) * SC_T;
    t.xs = max(t.x0 - SC_R, 0);
    t.nbytes = (min(t.x0 + SC_T + SC_R - 1, wc - 1) - t.xs + 1) * 3;       // <= 78
    return t;
}

// byte offset of column t.xs of halo row r (clamped to the cropped frame) in a frame set of (h, w) with crop cb
__device__ __forceinline__ long long score_row_offset(const ScoreTile& t, int r, int h, int w, int hc, int cb) {
    const int y = min(max(t.y0 + r - SC_R, 0), hc - 1);
    return (((t.f * h + cb + y) * w) + cb + t.xs) * 3;
}

// A: the aligned words that hold the row segments of halo rows [r0, r1) of both frames.  Word d of a row is read when it
// holds one of the segment's bytes: d < (misalignment + nbytes + 3) / 4 <= SC_RAW.
__device__ __forceinline__ void score_stage_raw(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b,
                                                const ScoreTile& t, int h, int w, int hc, int cb, int r0, int r1,
                                                unsigned (*rawA)[SC_RAW], unsigned (*rawB)[SC_RAW]) {
    for (int e = threadIdx.x; e < SC_HS * SC_RAW; e += 256) {
        const int r = e / SC_RAW, d = e % SC_RAW;
        if (r < r0 || r >= r1) continue;
        const long long off = score_row_offset(t, r, h, w, hc, cb);
        const unsigned char* pa = a + off;
        const unsigned char* pb = b + off;
        const int ma = (int)((unsigned long long)pa & 3), mb = (int)((unsigned long long)pb & 3);
        if (d < (ma + t.nbytes + 3) >> 2) rawA[r][d] = reinterpret_cast<const unsigned*>(pa - ma)[d];
        if (d < (mb + t.nbytes + 3) >> 2) rawB[r][d] = reinterpret_cast<const unsigned*>(pb - mb)[d];
    }
}

// byte k of the row segment that score_stage_raw put into `raw_row` from the global address `p`
__device__ __forceinline__ float score_byte(const unsigned* raw_row, const unsigned char* p, int k) {
    return (float)reinterpret_cast<const unsigned char*>(raw_row)[(int)((unsigned long long)p & 3) + k];
}

// ---- colour: sq_rgb and, with S3D, the 3-D SSIM (the halo is staged only then)
template <bool S3D>
__global__ __launch_bounds__(256) void score_rgb_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b,
                                                       int h, int w, int hc, int wc, int cb, int tiles_x, int tiles_y, int bgr,
                                                       const SsimConst k, unsigned long long* __restrict__ sq_parts,
                                                       double* __restrict__ ssim_parts) {
    constexpr int T = SC_T, R = SC_R, HS = SC_HS;
    constexpr int LO = S3D ? 0 : R, HI = S3D ? HS : R + T;         // the halo rows and columns in use
    __shared__ unsigned rawA[HS][SC_RAW], rawB[HS][SC_RAW];
    __shared__ float sA[3][HS][HS + 1], sB[3][HS][HS + 1];
    __shared__ float sH[S3D ? 5 : 1][3][S3D ? HS : 1][T + 1];
    __shared__ double sred[4];
    __shared__ unsigned sqred[4];
    const ScoreTile t = score_tile(tiles_x, tiles_y, wc);
    score_stage_raw(a, b, t, h, w, hc, cb, LO, HI, rawA, rawB);
    __syncthreads();
    for (int e = threadIdx.x; e < 3 * HS * HS; e += 256) {          // plane c = R, G, B whatever the byte order
        const int c = e / (HS * HS), r = (e / HS) % HS, q = e % HS;
        if (r < LO || r >= HI || q < LO || q >= HI) continue;
        const int x = min(max(t.x0 + q - R, 0), wc - 1);           // replicate
        const long long off = score_row_offset(t, r, h, w, hc, cb);
        const int kb = (x - t.xs) * 3 + (bgr ? 2 - c : c);
        sA[c][r][q] = score_byte(rawA[r], a + off, kb);
        sB[c][r][q] = score_byte(rawB[r], b + off, kb);
    }
    __syncthreads();
    const int ty = threadIdx.x / T, tx = threadIdx.x % T;
    const bool inside = t.y0 + ty < hc && t.x0 + tx < wc;
    if (sq_parts) {                                                 // (block-uniform)
        unsigned d2 = 0;
        if (inside) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int d = (int)sA[c][ty + R][tx + R] - (int)sB[c][ty + R][tx + R];
                d2 += (unsigned)(d * d);
            }
        }
        const unsigned long long s = refid_block_sum<unsigned long long, 4>(d2, sqred);     // (each d2 <= 3 * 255^2)
        if (threadIdx.x == 0) sq_parts[blockIdx.x] = s;
    }
    if constexpr (S3D) {
        SSIM3D_HPASS(sA, sB, sH, k)
        __syncthreads();
        SSIM3D_PIXEL(acc, sH, k, ty, tx, inside)
        SSIM3D_BLOCK_SUM(acc, sred, ssim_parts[blockIdx.x])
    }
}

// ---- Y: fl32((Ya - Yb)^2), _ssim_cly, the taps

// fl32(d * d) with d = fl32(ya - yb), widened: one term of the float32 (img1 - img2)**2
__device__ __forceinline__ double score_sqy_term(float ya, float yb) {
#pragma clang fp contract(off)
    const float d = ya - yb;
    const float e = d * d;
    return (double)e;
}

// _ssim_cly's map at pixel (ty, tx) of the tile: five 121-tap float64 sums in row-major tap order from zero, then the map
// in the reference's operation order.  The products of two float32 values are exact in float64.
__device__ __forceinline__ double score_ssim_y_pixel(const float (*y1)[SC_HS + 1], const float (*y2)[SC_HS + 1],
                                                     const ScoreConst& k, int ty, int tx) {
#pragma clang fp contract(off)
    double m1 = 0.0, m2 = 0.0, s11 = 0.0, s22 = 0.0, s12 = 0.0;
#pragma unroll
    for (int i = 0; i < 11; ++i)
#pragma unroll
        for (int j = 0; j < 11; ++j) {
            const double wk = k.win[i * 11 + j];
            const double x1 = (double)y1[ty + i][tx + j], x2 = (double)y2[ty + i][tx + j];
            m1 = m1 + wk * x1;
            m2 = m2 + wk * x2;
            s11 = s11 + wk * (x1 * x1);
            s22 = s22 + wk * (x2 * x2);
            s12 = s12 + wk * (x1 * x2);
        }
    const double mu1_sq = m1 * m1, mu2_sq = m2 * m2, mu1_mu2 = m1 * m2;
    const double sg1 = s11 - mu1_sq, sg2 = s22 - mu2_sq, sg12 = s12 - mu1_mu2;
    return ((2.0 * mu1_mu2 + k.c1) * (2.0 * sg12 + k.c2)) / ((mu1_sq + mu2_sq + k.c1) * (sg1 + sg2 + k.c2));
}

__global__ __launch_bounds__(256) void score_y_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b,
                                                     int h, int w, int hc, int wc, int cb, int tiles_x, int tiles_y, int bgr,
                                                     const ScoreConst k, double* __restrict__ sqy_parts,
                                                     double* __restrict__ ssim_parts, float* __restrict__ ya_out,
                                                     double* __restrict__ map_out) {
    constexpr int T = SC_T, R = SC_R, HS = SC_HS;
    __shared__ unsigned rawA[HS][SC_RAW], rawB[HS][SC_RAW];
    __shared__ float yA[HS][HS + 1], yB[HS][HS + 1];
    __shared__ double sred[2][4];
    const ScoreTile t = score_tile(tiles_x, tiles_y, wc);
    const int lo = ssim_parts ? 0 : R, hi = ssim_parts ? HS : R + T;        // (block-uniform) the halo only for the SSIM
    score_stage_raw(a, b, t, h, w, hc, cb, lo, hi, rawA, rawB);
    __syncthreads();
    for (int e = threadIdx.x; e < HS * HS; e += 256) {
        const int r = e / HS, q = e % HS;
        if (r < lo || r >= hi || q < lo || q >= hi) continue;
        const int x = min(max(t.x0 + q - R, 0), wc - 1);           // replicate
        const long long off = score_row_offset(t, r, h, w, hc, cb);
        const int k0 = (x - t.xs) * 3, kr = bgr ? k0 + 2 : k0, kbl = bgr ? k0 : k0 + 2;
        yA[r][q] = refid_y601_u8(score_byte(rawA[r], a + off, kr), score_byte(rawA[r], a + off, k0 + 1),
                                 score_byte(rawA[r], a + off, kbl));
        yB[r][q] = refid_y601_u8(score_byte(rawB[r], b + off, kr), score_byte(rawB[r], b + off, k0 + 1),
                                 score_byte(rawB[r], b + off, kbl));
    }
    __syncthreads();
    const int ty = threadIdx.x / T, tx = threadIdx.x % T;
    const bool inside = t.y0 + ty < hc && t.x0 + tx < wc;
    const long long pix = (t.f * hc + t.y0 + ty) * wc + t.x0 + tx; // used only when inside
    if (ya_out && inside) ya_out[pix] = yA[ty + R][tx + R];
    if (sqy_parts) {                                                // (block-uniform)
        double e = inside ? score_sqy_term(yA[ty + R][tx + R], yB[ty + R][tx + R]) : 0.0;
        SSIM3D_BLOCK_SUM(e, sred[0], sqy_parts[blockIdx.x])
    }
    if (ssim_parts) {
        double m = inside ? score_ssim_y_pixel(yA, yB, k, ty, tx) : 0.0;
        if (map_out && inside) map_out[pix] = m;
        SSIM3D_BLOCK_SUM(m, sred[1], ssim_parts[blockIdx.x])
    }
}

ScoreConst score_const() {
    ScoreConst k;
    double g[11], s = 0.0;                                  // cv2.getGaussianKernel(11, 1.5), as ssim_const()
    for (int i = 0; i < 11; ++i) { g[i] = exp(-((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); s += g[i]; }
    for (int i = 0; i < 11; ++i) g[i] /= s;
    for (int i = 0; i < 11; ++i)
        for (int j = 0; j < 11; ++j) k.win[i * 11 + j] = g[i] * g[j];       // np.outer(kernel, kernel.transpose())
    k.c1 = (0.01 * 255) * (0.01 * 255);
    k.c2 = (0.03 * 255) * (0.03 * 255);
    return k;
}

// tiles of the call, or 0 for arguments the entry point turns down
long long score_blocks(int n_frames, int h, int w, int crop_border) {
    if (n_frames < 1 || h < 1 || w < 1 || crop_border < 0) return 0;
    const long long hc = (long long)h - 2ll * crop_border, wc = (long long)w - 2ll * crop_border;
    if (hc < 1 || wc < 1) return 0;
    if ((long long)n_frames * h * w * 3 > 0x7fffffffll) return 0;
    const long long blocks = (long long)n_frames * ((hc + SC_T - 1) / SC_T) * ((wc + SC_T - 1) / SC_T);
    return blocks <= 0x7fffffffll ? blocks : 0;
}

}  // namespace

extern "C" long long refid_score_u8_parts(int n_frames, int h, int w, int crop_border) {
    return 4 * score_blocks(n_frames, h, w, crop_border);
}

extern "C" int refid_score_u8(const unsigned char* a_u8, const unsigned char* b_u8, int n_frames, int h, int w, int flags,
                              int crop_border, unsigned long long* sq_rgb, double* sq_y, double* ssim3d, double* ssim_y,
                              void* parts, float* ya_out, double* ssim_y_map_out, void* stream) {
    REFID_CHECK(a_u8 && b_u8, "score_u8: NULL frames");
    REFID_CHECK(n_frames > 0 && h > 0 && w > 0, "score_u8: bad arguments (n_frames=%d, %dx%d)", n_frames, h, w);
    REFID_CHECK((flags & ~REFID_SCORE_BGR) == 0, "score_u8: unknown flags 0x%x", flags);
    REFID_CHECK(crop_border >= 0, "score_u8: crop_border %d is negative", crop_border);
    const long long hb = (long long)h - 2ll * crop_border, wb = (long long)w - 2ll * crop_border;
    REFID_CHECK(hb >= 1 && wb >= 1, "score_u8: crop_border %d leaves nothing of a %dx%d frame", crop_border, h, w);
    REFID_CHECK((long long)n_frames * h * w * 3 <= 0x7fffffffll,
                "score_u8: %d frames of %dx%d put a byte offset beyond 31 bits (split the call)", n_frames, h, w);
    const long long blocks = score_blocks(n_frames, h, w, crop_border);
    REFID_CHECK(blocks > 0, "score_u8: the tiles of %d frames of %dx%d exceed the grid (split the call)", n_frames, h, w);
    REFID_CHECK(parts || !(sq_rgb || sq_y || ssim3d || ssim_y), "score_u8: the outputs need parts");
    REFID_CHECK(ssim_y || !ssim_y_map_out, "score_u8: ssim_y_map_out needs ssim_y");
    hipStream_t st = (hipStream_t)stream;
    const int hc = (int)hb, wc = (int)wb, tx = cdiv(wc, SC_T), ty = cdiv(hc, SC_T), bgr = flags & REFID_SCORE_BGR;
    const dim3 grid((unsigned)blocks);
    unsigned long long* w0 = (unsigned long long*)parts;    // [blocks] words per output: sq_rgb | sq_y | ssim3d | ssim_y
    unsigned long long* sq_parts = sq_rgb ? w0 : nullptr;
    double* sqy_parts = sq_y ? (double*)(w0 + blocks) : nullptr;
    double* s3_parts = ssim3d ? (double*)(w0 + 2 * blocks) : nullptr;
    double* sy_parts = ssim_y ? (double*)(w0 + 3 * blocks) : nullptr;
    if (ssim3d) {
        hipLaunchKernelGGL(score_rgb_kernel<true>, grid, dim3(256), 0, st, a_u8, b_u8, h, w, hc, wc, crop_border, tx, ty, bgr,
                           ssim_const(), sq_parts, s3_parts);
        REFID_LAUNCH_CHECK("score_u8/rgb");
    } else if (sq_rgb) {
        hipLaunchKernelGGL(score_rgb_kernel<false>, grid, dim3(256), 0, st, a_u8, b_u8, h, w, hc, wc, crop_border, tx, ty, bgr,
                           SsimConst{}, sq_parts, s3_parts);
        REFID_LAUNCH_CHECK("score_u8/rgb");
    }
    if (sq_y || ssim_y || ya_out) {
        hipLaunchKernelGGL(score_y_kernel, grid, dim3(256), 0, st, a_u8, b_u8, h, w, hc, wc, crop_border, tx, ty, bgr,
                           ssim_y ? score_const() : ScoreConst{}, sqy_parts, sy_parts, ya_out, ssim_y_map_out);
        REFID_LAUNCH_CHECK("score_u8/y");
    }
    if (sq_rgb)
        if (int rc = refid_launch_sum_rows_u64(sq_parts, n_frames, tx * ty, sq_rgb, st)) return rc;
    if (sq_y)
        if (int rc = refid_launch_sum_rows_f64(sqy_parts, n_frames, tx * ty, sq_y, st)) return rc;
    if (ssim3d)
        if (int rc = refid_launch_sum_rows_f64(s3_parts, n_frames, tx * ty, ssim3d, st)) return rc;
    if (ssim_y)
        if (int rc = refid_launch_sum_rows_f64(sy_parts, n_frames, tx * ty, ssim_y, st)) return rc;
    return 0;
}
