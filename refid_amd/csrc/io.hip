// Callers either side of the hot path (SURVEY.md section 8f "next" rows 1-3):
//   * event voxelisation     basicsr/data/event_util.py:6-66  (events_to_voxel_grid)
//   * validation tail        basicsr/utils/img_util.py:90-117 (tensor2img quantisation) +
//                            basicsr/metrics/psnr_ssim.py:48-63 (calculate_psnr, float64 MSE)
//   * tile overlap-averaging basicsr/models/twoImage_event_recurrent_model.py:252-268 (grids_inverse)
// HBM-bound streaming kernels; the scalar sums (PSNR / SSIM) are two-stage and deterministic, only the event scatter-add
// uses (fp32) atomics, as np.add.at's order is unspecified too.  That whole-frame, float64-event voxeliser stays for
// callers that want a full grid; the training path does not need it any more: sample.hip voxelises the float32 event
// rows of the datasets inside the crop with integer (bit-reproducible) sums while it assembles the batch.
#include "common.h"
#include "workgroup.h"
#include "ssim3d_tile.h"

namespace {

// voxel[(ti) * H*W + y*W + x] += pol*(1-dt) ; voxel[(ti+1)...] += pol*dt   (bilinear in time)
__global__ __launch_bounds__(256) void voxel_kernel(const double* __restrict__ ts, const int* __restrict__ xs,
                                                   const int* __restrict__ ys, const float* __restrict__ ps,
                                                   long long n, int bins, int W, int H, double first, double deltaT,
                                                   float* __restrict__ voxel) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double t = (double)(bins - 1) * (ts[i] - first) / deltaT;       // event_util.py:36
        const int ti = (int)t;                                                // astype(int): truncation
        const double dt = t - (double)ti;
        double pol = (double)ps[i];
        if (pol == 0.0) pol = -1.0;                                           // event_util.py:41
        const int x = xs[i], y = ys[i];
        if (x < 0 || x >= W || y < 0 || y >= H) continue;
        const long long base = (long long)y * W + x;
        if (ti >= 0 && ti < bins) atomicAdd(voxel + (long long)ti * W * H + base, (float)(pol * (1.0 - dt)));
        if (ti + 1 >= 0 && ti + 1 < bins) atomicAdd(voxel + (long long)(ti + 1) * W * H + base, (float)(pol * dt));
    }
}

__device__ __forceinline__ float quant255(float v) {          // tensor2img: clamp [0,1], *255, round (half to even)
    v = fminf(fmaxf(v, 0.f), 1.f);
    return rintf(v * 255.f);
}

// sq[f][chunk] = sum over the chunk's share of the frame of (q(a) - q(b))^2 ; grid = (chunks, frames)
__global__ __launch_bounds__(256) void sqerr_u8_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                      long long frame_elems, double* __restrict__ sq) {
    __shared__ double sh[4];
    const long long f = blockIdx.y;
    const float* pa = a + f * frame_elems;
    const float* pb = b + f * frame_elems;
    double acc = 0.0;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < frame_elems; i += (long long)gridDim.x * 256) {
        const float d = quant255(pa[i]) - quant255(pb[i]);
        acc += (double)(d * d);
    }
    const double t = refid_block_sum<double, 4>(acc, sh);
    if (threadIdx.x == 0) sq[f * gridDim.x + blockIdx.x] = t;   // partial [frame][chunk]
}

// acc[c][i0+y][j0+x] += tile[c][y][x] ; cnt[i0+y][j0+x] += 1     (one tile)
__global__ __launch_bounds__(256) void tile_add_kernel(const float* __restrict__ tile, float* __restrict__ acc,
                                                      float* __restrict__ cnt, int C, int th, int tw, int H, int W,
                                                      int i0, int j0) {
    const long long total = (long long)C * th * tw;
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int x = e % tw; long long r = e / tw;
        const int y = r % th; const int c = r / th;
        const long long d = ((long long)c * H + i0 + y) * W + j0 + x;
        acc[d] += tile[e];
        if (c == 0) cnt[(long long)(i0 + y) * W + j0 + x] += 1.f;
    }
}

__global__ __launch_bounds__(256) void tile_norm_kernel(float* __restrict__ acc, const float* __restrict__ cnt, int C,
                                                       long long HW) {
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < C * HW; e += (long long)gridDim.x * 256)
        acc[e] /= cnt[e % HW];
}

// ---- SSIM of the reference's _ssim_3d (metrics/psnr_ssim.py:135-182): 11x11x11 separable Gaussian
// (sigma 1.5) over (H, W, C=3) with REPLICATE padding in all three axes, fp32, on the uint8-quantised
// frames; ssim map mean over H*W*3.  One block = 16x16 output pixels x 3 channels.
// The arithmetic lives in ssim3d_tile.h, shared with val_tail_kernel below and with score.hip.
__global__ __launch_bounds__(256) void ssim3d_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                    int H, int W, const SsimConst k, double* __restrict__ out) {
    constexpr int T = SSIM_T, R = SSIM_R, HS = SSIM_HS;   // 16, 5, 26
    __shared__ float sA[3][HS][HS + 1], sB[3][HS][HS + 1];
    __shared__ float sH[5][3][HS][T + 1];
    __shared__ double sred[4];
    const int f = blockIdx.z;
    const int y0 = blockIdx.y * T, x0 = blockIdx.x * T;
    const float* pa = a + (long long)f * 3 * H * W;
    const float* pb = b + (long long)f * 3 * H * W;
    for (int e = threadIdx.x; e < 3 * HS * HS; e += 256) {
        const int c = e / (HS * HS), r = (e / HS) % HS, q = e % HS;
        const int y = min(max(y0 + r - R, 0), H - 1), x = min(max(x0 + q - R, 0), W - 1);   // replicate
        sA[c][r][q] = quant255(pa[((long long)c * H + y) * W + x]);
        sB[c][r][q] = quant255(pb[((long long)c * H + y) * W + x]);
    }
    __syncthreads();
    SSIM3D_HPASS(sA, sB, sH, k)
    __syncthreads();
    const int ty = threadIdx.x / T, tx = threadIdx.x % T;
    SSIM3D_PIXEL(acc, sH, k, ty, tx, y0 + ty < H && x0 + tx < W)
    // partial [frame][tile row][tile column]
    SSIM3D_BLOCK_SUM(acc, sred, out[((long long)f * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x])
}

// ---- fused validation tail (twoImage_event_recurrent_model.py:412-491): tensor2img of pred / gt into HWC uint8 images,
// the integer squared error of calculate_psnr and the _ssim_3d sum, in one pass over the fp32 frames.  Same 16x16 tile,
// same staging and same SSIM arithmetic as ssim3d_kernel, so its partials (and their fixed-order finish) are the same
// bits; the frame index is folded into blockIdx.x: partial index = blockIdx.x = [frame][tile row][tile column].

// One 16-lane group writes one row segment of a tile (nv = 3 * pixels bytes, HWC) from its image in LDS, which the
// staging loop laid out so that LDS and global addresses agree modulo 16 (see val_tail_kernel).  Aligned full segments
// (48 bytes) go out as three 16-byte stores; otherwise 4-byte stores from the first aligned address, and lanes 12 / 13
// write the at most three head / tail bytes that a neighbouring tile's segment shares a word with.
__device__ __forceinline__ void val_store_row(unsigned char* __restrict__ dst, const unsigned* srow, int j, int nv) {
    const unsigned long long a = (unsigned long long)dst;
    const unsigned char* src = reinterpret_cast<const unsigned char*>(srow) + (a & 3);      // src[k] = byte k of the segment
    if (nv == 48 && (a & 15) == 0) {
        if (j < 3) *reinterpret_cast<uint4*>(dst + 16 * j) = *reinterpret_cast<const uint4*>(src + 16 * j);
        return;
    }
    const int head = min((int)((4 - (a & 3)) & 3), nv);
    const int nd = (nv - head) >> 2;                               // <= 12
    if (j < nd) *reinterpret_cast<unsigned*>(dst + head + 4 * j) = *reinterpret_cast<const unsigned*>(src + head + 4 * j);
    else if (j == 12) { for (int k = 0; k < head; ++k) dst[k] = src[k]; }
    else if (j == 13) { for (int k = head + 4 * nd; k < nv; ++k) dst[k] = src[k]; }
}

template <bool SSIM>
__global__ __launch_bounds__(256) void val_tail_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W,
                                                      int tiles_x, int tiles_y, int bgr, const SsimConst k,
                                                      unsigned char* __restrict__ a_u8, unsigned char* __restrict__ b_u8,
                                                      unsigned long long* __restrict__ sq_parts,
                                                      double* __restrict__ ssim_parts) {
    constexpr int T = 16, R = SSIM ? 5 : 0, HS = T + 2 * R;         // 26 with the SSIM halo, 16 without
    __shared__ float sA[3][HS][HS + 1], sB[3][HS][HS + 1];
    __shared__ float sH[SSIM ? 5 : 1][3][SSIM ? HS : 1][T + 1];
    // the tile's uint8 HWC rows, 64 bytes each; byte k of a row lies at (address of its global row segment & 3) + k, so
    // the word a lane stores to an aligned global address is an aligned word here
    __shared__ __attribute__((aligned(16))) unsigned uA[T][16], uB[T][16];
    __shared__ double sred[4];
    __shared__ unsigned sqred[4];
    const int tile = blockIdx.x % (tiles_x * tiles_y);
    const long long f = blockIdx.x / (tiles_x * tiles_y);
    const int y0 = (tile / tiles_x) * T, x0 = (tile % tiles_x) * T;
    const float* pa = a + f * 3 * H * W;
    const float* pb = b ? b + f * 3 * H * W : nullptr;
    const long long off0 = ((f * H + y0) * W + x0) * 3;            // the tile's first byte in the uint8 images
    const unsigned a_lo = (unsigned)(unsigned long long)(a_u8 + off0);
    const unsigned b_lo = b_u8 ? (unsigned)(unsigned long long)(b_u8 + off0) : 0u;
    for (int e = threadIdx.x; e < 3 * HS * HS; e += 256) {
        const int c = e / (HS * HS), r = (e / HS) % HS, q = e % HS;
        const int y = min(max(y0 + r - R, 0), H - 1), x = min(max(x0 + q - R, 0), W - 1);   // replicate
        const float va = quant255(pa[((long long)c * H + y) * W + x]);
        const float vb = pb ? quant255(pb[((long long)c * H + y) * W + x]) : 0.f;
        sA[c][r][q] = va;
        sB[c][r][q] = vb;
        const int row = r - R, px = q - R;
        if (row >= 0 && row < T && px >= 0 && px < T) {            // interior: also as a byte of the HWC row
            const int k = 3 * px + (bgr ? 2 - c : c);
            const unsigned step = 3u * (unsigned)W * (unsigned)row; // the row segment's address, modulo 4
            reinterpret_cast<unsigned char*>(uA[row])[((a_lo + step) & 3) + k] = (unsigned char)va;
            if (b_u8) reinterpret_cast<unsigned char*>(uB[row])[((b_lo + step) & 3) + k] = (unsigned char)vb;
        }
    }
    __syncthreads();
    const int ty = threadIdx.x / T, tx = threadIdx.x % T;
    const bool inside = y0 + ty < H && x0 + tx < W;
    if (y0 + ty < H) {                                              // 16 lanes per row segment
        const int nv = min(T, W - x0) * 3;
        const long long off = off0 + (long long)ty * W * 3;
        val_store_row(a_u8 + off, uA[ty], tx, nv);
        if (b_u8) val_store_row(b_u8 + off, uB[ty], tx, nv);
    }
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
    if constexpr (SSIM) {
        SSIM3D_HPASS(sA, sB, sH, k)
        __syncthreads();
        SSIM3D_PIXEL(acc, sH, k, ty, tx, inside)
        SSIM3D_BLOCK_SUM(acc, sred, ssim_parts[blockIdx.x])
    }
}

// out[f] = sum of the frame's n integer partials (any order gives the same integer)
__global__ __launch_bounds__(256) void sum_rows_u64_kernel(const unsigned long long* __restrict__ part, int n,
                                                          unsigned long long* __restrict__ out) {
    __shared__ unsigned long long sh[4];
    const unsigned long long* p = part + (long long)blockIdx.x * n;
    unsigned long long acc = 0;
    for (int i = threadIdx.x; i < n; i += 256) acc += p[i];
    const unsigned long long t = refid_block_sum<unsigned long long, 4>(acc, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = t;
}

int nb(long long n) { long long b = (n + 255) / 256; return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b)); }

}  // namespace

int refid_launch_sum_rows_u64(const unsigned long long* part, int rows, int n, unsigned long long* out, hipStream_t st) {
    hipLaunchKernelGGL(sum_rows_u64_kernel, dim3(rows), dim3(256), 0, st, part, n, out);
    REFID_LAUNCH_CHECK("sum_rows_u64");
    return 0;
}

extern "C" int refid_events_to_voxel(const double* ts, const int* xs, const int* ys, const float* ps,
                                     long long n_events, int num_bins, int width, int height, double first_stamp,
                                     double last_stamp, float* voxel, void* stream) {
    REFID_CHECK(ts && xs && ys && ps && voxel && n_events > 0 && num_bins > 0 && width > 0 && height > 0,
                "events_to_voxel: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(voxel, 0, sizeof(float) * (size_t)num_bins * width * height, st);
    REFID_CHECK(e == hipSuccess, "events_to_voxel: memset failed: %s", hipGetErrorString(e));
    double deltaT = last_stamp - first_stamp;
    if (deltaT == 0) deltaT = 1.0;                                            // event_util.py:33-34
    hipLaunchKernelGGL(voxel_kernel, dim3(nb(n_events)), dim3(256), 0, st, ts, xs, ys, ps, n_events, num_bins, width,
                       height, first_stamp, deltaT, voxel);
    REFID_LAUNCH_CHECK("events_to_voxel");
    return 0;
}

static int sqerr_chunks(long long frame_elems) {
    const int c = nb(frame_elems);
    return c > 256 ? 256 : c;
}

extern "C" int refid_sqerr_u8_parts(int n_frames, long long frame_elems) {
    return (n_frames > 0 && frame_elems > 0) ? n_frames * sqerr_chunks(frame_elems) : 0;
}

extern "C" int refid_sqerr_u8(const float* a, const float* b, int n_frames, long long frame_elems, double* sq,
                              double* parts, void* stream) {
    REFID_CHECK(a && b && sq && parts && n_frames > 0 && frame_elems > 0, "sqerr_u8: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const int chunks = sqerr_chunks(frame_elems);
    hipLaunchKernelGGL(sqerr_u8_kernel, dim3(chunks, n_frames), dim3(256), 0, st, a, b, frame_elems, parts);
    REFID_LAUNCH_CHECK("sqerr_u8");
    return refid_launch_sum_rows_f64(parts, n_frames, chunks, sq, st);
}

extern "C" int refid_tile_add(const float* tile, float* acc, float* cnt, int c, int th, int tw, int h, int w, int i0,
                              int j0, void* stream) {
    REFID_CHECK(tile && acc && cnt && c > 0 && th > 0 && tw > 0 && i0 >= 0 && j0 >= 0 && i0 + th <= h && j0 + tw <= w,
                "tile_add: tile (%d,%d)+(%d,%d) outside %dx%d", i0, j0, th, tw, h, w);
    hipLaunchKernelGGL(tile_add_kernel, dim3(nb((long long)c * th * tw)), dim3(256), 0, (hipStream_t)stream, tile, acc,
                       cnt, c, th, tw, h, w, i0, j0);
    REFID_LAUNCH_CHECK("tile_add");
    return 0;
}

extern "C" int refid_tile_normalize(float* acc, const float* cnt, int c, int h, int w, void* stream) {
    REFID_CHECK(acc && cnt && c > 0 && h > 0 && w > 0, "tile_normalize: bad arguments");
    hipLaunchKernelGGL(tile_norm_kernel, dim3(nb((long long)c * h * w)), dim3(256), 0, (hipStream_t)stream, acc, cnt, c,
                       (long long)h * w);
    REFID_LAUNCH_CHECK("tile_normalize");
    return 0;
}

extern "C" int refid_ssim3d_u8_parts(int n_frames, int h, int w) {
    return (n_frames > 0 && h > 0 && w > 0) ? n_frames * cdiv(w, 16) * cdiv(h, 16) : 0;
}

extern "C" int refid_ssim3d_u8(const float* a, const float* b, int n_frames, int h, int w, double* sum_out,
                               double* parts, void* stream) {
    REFID_CHECK(a && b && sum_out && parts && n_frames > 0 && h > 0 && w > 0, "ssim3d_u8: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const SsimConst k = ssim_const();
    dim3 grid(cdiv(w, 16), cdiv(h, 16), n_frames);
    hipLaunchKernelGGL(ssim3d_kernel, grid, dim3(256), 0, st, a, b, h, w, k, parts);
    REFID_LAUNCH_CHECK("ssim3d_u8");
    return refid_launch_sum_rows_f64(parts, n_frames, (int)(grid.x * grid.y), sum_out, st);
}

static long long val_tail_blocks(int n_frames, int h, int w) { return (long long)n_frames * cdiv(w, 16) * cdiv(h, 16); }

extern "C" long long refid_val_tail_parts(int n_frames, int h, int w) {
    return (n_frames > 0 && h > 0 && w > 0) ? 2 * val_tail_blocks(n_frames, h, w) : 0;
}

extern "C" int refid_val_tail(const float* pred, const float* gt, int n_frames, int h, int w, int flags,
                              unsigned char* pred_u8, unsigned char* gt_u8, unsigned long long* sq_out, double* ssim_out,
                              void* parts, void* stream) {
    REFID_CHECK(pred && pred_u8 && n_frames > 0 && h > 0 && w > 0, "val_tail: bad arguments");
    REFID_CHECK(gt || !(gt_u8 || sq_out || ssim_out), "val_tail: gt_u8 / sq_out / ssim_out need gt");
    REFID_CHECK(parts || !(sq_out || ssim_out), "val_tail: sq_out / ssim_out need parts");
    REFID_CHECK((flags & ~REFID_VAL_TAIL_BGR) == 0, "val_tail: unknown flags 0x%x", flags);
    const long long blocks = val_tail_blocks(n_frames, h, w);
    REFID_CHECK(blocks <= 0x7fffffffll, "val_tail: %lld tiles exceed the grid (n_frames=%d, %dx%d)", blocks, n_frames, h, w);
    hipStream_t st = (hipStream_t)stream;
    const int tx = cdiv(w, 16), ty = cdiv(h, 16), bgr = flags & REFID_VAL_TAIL_BGR;
    double* ssim_parts = (double*)parts;                    // [blocks] doubles, then [blocks] integer squared errors
    unsigned long long* sq_parts = sq_out ? (unsigned long long*)parts + blocks : nullptr;
    if (ssim_out)
        hipLaunchKernelGGL(val_tail_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, pred, gt, h, w, tx, ty, bgr,
                           ssim_const(), pred_u8, gt_u8, sq_parts, ssim_parts);
    else
        hipLaunchKernelGGL(val_tail_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, pred, gt, h, w, tx, ty, bgr,
                           SsimConst{}, pred_u8, gt_u8, sq_parts, ssim_parts);
    REFID_LAUNCH_CHECK("val_tail");
    if (sq_out) {
        if (int rc = refid_launch_sum_rows_u64(sq_parts, n_frames, tx * ty, sq_out, st)) return rc;
    }
    if (ssim_out) return refid_launch_sum_rows_f64(ssim_parts, n_frames, tx * ty, ssim_out, st);
    return 0;
}
