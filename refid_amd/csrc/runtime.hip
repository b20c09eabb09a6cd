// Error plumbing, device queries, layout conversion and small elementwise kernels of the REFID C ABI.
// (Weight packing: pack.hip.)
#include "common.h"

static thread_local char g_err[512] = "";

void refid_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* refid_last_error(void) { return g_err; }
extern "C" int refid_abi_version(void) { return REFID_ABI_VERSION; }
extern "C" int refid_experimental_tiles(void) {
    return 0;
}

extern "C" int refid_device_cu_count(void) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, dev) != hipSuccess) return -1;
    return p.multiProcessorCount;
}

namespace {

// ---- NCHW -> NHWC (padded) : one block transposes a 32-pixel x C strip through LDS ----------
// (tCount > 1: the source is (n, tCount, C, HW) and the tCount slices are summed on the way -- the gradient of a tensor
// every time step reads, e.g. `head` in `pred(z_t + head)`, XXNet_final_attenfusion_arch.py:215)
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ src,
                                                          long long srcBatchStride,
                                                          float* __restrict__ dst, int C, int HW,
                                                          int Cpad, int tCount, long long tStride, int nb) {
    // grid.x = pixel blocks of 64, grid.y = n.  nb > 0 (time-major form, tCount = 1): output sample n = t nb + b reads the
    // source's (b, t) block, at b srcBatchStride + t tStride
    __shared__ float tile[64][65];
    const int n = blockIdx.y;
    const long long srcOff = nb > 0 ? (long long)(n % nb) * srcBatchStride + (long long)(n / nb) * tStride
                                    : (long long)n * srcBatchStride;
    const int p0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;   // ty in 0..3
    for (int c0 = 0; c0 < Cpad; c0 += 64) {
        // read: coalesced along pixels
        for (int cc = ty; cc < 64; cc += 4) {
            const int c = c0 + cc, p = p0 + tx;
            float v = 0.f;
            if (c < C && p < HW) {
                const float* sp = src + srcOff + (long long)c * HW + p;
                for (int t = 0; t < tCount; ++t) v += sp[t * tStride];
            }
            tile[cc][tx] = v;
        }
        __syncthreads();
        // write: coalesced along channels
        for (int pp = ty; pp < 64; pp += 4) {
            const int c = c0 + tx, p = p0 + pp;
            if (c < Cpad && p < HW) dst[((long long)n * HW + p) * Cpad + c] = tile[tx][pp];
        }
        __syncthreads();
    }
}

// Thin tensors (C <= 4: event voxels 2 -> 4, the 3-channel output and its gradient): the 64-channel LDS transpose above moves
// 16 bytes per store instruction for them (0.06-0.13 of HBM).  Here a thread owns a PIXEL: C coalesced plane reads, one 16-byte
// NHWC access (a wave writes 1 KB contiguous) -- and the reverse.  Same sample addressing (time-major form, sum over T).
__global__ __launch_bounds__(256) void nchw_to_nhwc4_kernel(const float* __restrict__ src, long long srcBatchStride,
                                                           f32x4* __restrict__ dst, int C, int HW, int tCount, long long tStride,
                                                           int nb) {
    const int n = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const long long srcOff = nb > 0 ? (long long)(n % nb) * srcBatchStride + (long long)(n / nb) * tStride
                                    : (long long)n * srcBatchStride;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c >= C) break;
        const float* sp = src + srcOff + (long long)c * HW + p;
        float acc = 0.f;
        for (int t = 0; t < tCount; ++t) acc += sp[t * tStride];
        v[c] = acc;
    }
    dst[(long long)n * HW + p] = v;
}

__global__ __launch_bounds__(256) void nhwc4_to_nchw_kernel(const f32x4* __restrict__ src, float* __restrict__ dst,
                                                           long long dstBatchStride, int C, int HW, int nb, long long tStride) {
    const int n = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const long long dstOff = nb > 0 ? (long long)(n % nb) * dstBatchStride + (long long)(n / nb) * tStride
                                    : (long long)n * dstBatchStride;
    const f32x4 v = src[(long long)n * HW + p];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c >= C) break;
        dst[dstOff + (long long)c * HW + p] = v[c];
    }
}

__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const float* __restrict__ src, int ld,
                                                          float* __restrict__ dst,
                                                          long long dstBatchStride, int C, int HW, int nb, long long tStride) {
    // nb > 0: source sample n = t nb + b (time-major) goes to the destination's (b, t) block
    __shared__ float tile[64][65];
    const int n = blockIdx.y;
    const long long dstOff = nb > 0 ? (long long)(n % nb) * dstBatchStride + (long long)(n / nb) * tStride
                                    : (long long)n * dstBatchStride;
    const int p0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int c0 = 0; c0 < C; c0 += 64) {
        for (int pp = ty; pp < 64; pp += 4) {
            const int c = c0 + tx, p = p0 + pp;
            tile[pp][tx] = (c < C && p < HW) ? src[((long long)n * HW + p) * ld + c] : 0.f;
        }
        __syncthreads();
        for (int cc = ty; cc < 64; cc += 4) {
            const int c = c0 + cc, p = p0 + tx;
            if (c < C && p < HW) dst[dstOff + (long long)c * HW + p] = tile[tx][cc];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void add_kernel(const f32x4* __restrict__ a, const f32x4* __restrict__ b,
                                                 f32x4* __restrict__ out, long long n4) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        out[i] = a[i] + b[i];
    }
}

// out = in[0] + in[1] + ... + in[n-1], added in index order (deterministic).  Gradients that several time steps contribute to
// (the image branch's x_blocks, the final backward states) are summed ONCE after BPTT from the per-step tensors -- (n + 1)
// tensor passes instead of the 3 (n - 1) of n - 1 in-place accumulations, one launch instead of n - 1.
struct SumNArgs { const f32x4* in[REFID_SUM_MAX]; int n; };
__global__ __launch_bounds__(256) void sum_n_kernel(const SumNArgs a, f32x4* __restrict__ out, long long n4) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        f32x4 s = a.in[0][i];
        for (int k = 1; k < a.n; ++k) s += a.in[k][i];
        out[i] = s;
    }
}

__global__ __launch_bounds__(256) void act_bwd_kernel(const f32x4* __restrict__ g, const f32x4* __restrict__ y,
                                                     f32x4* __restrict__ out, float slope, int acc,
                                                     long long n4) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4 gv = g[i], yv = y[i];
        f32x4 o = acc ? out[i] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] += gv[k] * (yv[k] > 0.f ? 1.f : slope);
        out[i] = o;
    }
}

}  // namespace

// one launcher for the four NCHW -> NHWC entry points: thin tensors (c_pad == 4, 16-byte aligned dst) take the pixel-per-thread form
static int launch_to_nhwc(const float* src, long long b_stride, float* dst, int n, int c, int hw, int c_pad, int t_count,
                          long long t_stride, int nb, hipStream_t st, const char* what) {
    // a tCount sum in the time-major form would need two time strides: the entry points never combine them
    if (c_pad == 4 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        hipLaunchKernelGGL(nchw_to_nhwc4_kernel, dim3(cdiv(hw, 256), n), dim3(256), 0, st, src, b_stride,
                           reinterpret_cast<f32x4*>(dst), c, hw, t_count, t_stride, nb);
    } else {
        hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(cdiv(hw, 64), n), dim3(256), 0, st, src, b_stride, dst, c, hw, c_pad, t_count,
                           t_stride, nb);
    }
    REFID_LAUNCH_CHECK(what);
    return 0;
}

extern "C" int refid_nchw_to_nhwc(const float* src, long long src_batch_stride, float* dst, int n, int c, int h,
                                  int w, int c_pad, void* stream) {
    REFID_CHECK(src && dst && n > 0 && c > 0 && h > 0 && w > 0 && c_pad >= c, "nchw_to_nhwc: bad arguments");
    return launch_to_nhwc(src, src_batch_stride, dst, n, c, h * w, c_pad, 1, 0ll, 0, (hipStream_t)stream, "nchw_to_nhwc");
}

extern "C" int refid_nchw_to_nhwc_tb(const float* src, long long b_stride, long long t_stride, float* dst, int nb, int nt,
                                     int c, int h, int w, int c_pad, void* stream) {
    REFID_CHECK(src && dst && nb > 0 && nt > 0 && c > 0 && h > 0 && w > 0 && c_pad >= c, "nchw_to_nhwc_tb: bad arguments");
    REFID_CHECK((long long)nb * nt <= 65535, "nchw_to_nhwc_tb: more than 65535 (sample, step) blocks");
    return launch_to_nhwc(src, b_stride, dst, nb * nt, c, h * w, c_pad, 1, t_stride, nb, (hipStream_t)stream, "nchw_to_nhwc_tb");
}

extern "C" int refid_nchw_tsum_to_nhwc(const float* src, long long src_batch_stride, long long t_stride, int t_count,
                                       float* dst, int n, int c, int h, int w, int c_pad, void* stream) {
    REFID_CHECK(src && dst && n > 0 && c > 0 && h > 0 && w > 0 && c_pad >= c && t_count > 0,
                "nchw_tsum_to_nhwc: bad arguments");
    return launch_to_nhwc(src, src_batch_stride, dst, n, c, h * w, c_pad, t_count, t_stride, 0, (hipStream_t)stream,
                          "nchw_tsum_to_nhwc");
}

static int launch_to_nchw(const float* src, int ld, float* dst, long long b_stride, int n, int c, int hw, int nb,
                          long long t_stride, hipStream_t st, const char* what) {
    if (ld == 4 && c <= 4 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        hipLaunchKernelGGL(nhwc4_to_nchw_kernel, dim3(cdiv(hw, 256), n), dim3(256), 0, st, reinterpret_cast<const f32x4*>(src), dst,
                           b_stride, c, hw, nb, t_stride);
    } else {
        hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(cdiv(hw, 64), n), dim3(256), 0, st, src, ld, dst, b_stride, c, hw, nb, t_stride);
    }
    REFID_LAUNCH_CHECK(what);
    return 0;
}

extern "C" int refid_nhwc_to_nchw(const float* src, int ld, float* dst, long long dst_batch_stride, int n,
                                  int c, int h, int w, void* stream) {
    REFID_CHECK(src && dst && n > 0 && c > 0 && h > 0 && w > 0 && ld >= c, "nhwc_to_nchw: bad arguments");
    return launch_to_nchw(src, ld, dst, dst_batch_stride, n, c, h * w, 0, 0ll, (hipStream_t)stream, "nhwc_to_nchw");
}

extern "C" int refid_nhwc_to_nchw_tb(const float* src, int ld, float* dst, long long b_stride, long long t_stride, int nb,
                                     int nt, int c, int h, int w, void* stream) {
    REFID_CHECK(src && dst && nb > 0 && nt > 0 && c > 0 && h > 0 && w > 0 && ld >= c, "nhwc_to_nchw_tb: bad arguments");
    REFID_CHECK((long long)nb * nt <= 65535, "nhwc_to_nchw_tb: more than 65535 (sample, step) blocks");
    return launch_to_nchw(src, ld, dst, b_stride, nb * nt, c, h * w, nb, t_stride, (hipStream_t)stream, "nhwc_to_nchw_tb");
}

extern "C" int refid_add(const float* a, const float* b, float* out, long long count, void* stream) {
    REFID_CHECK(a && b && out && count > 0 && count % 4 == 0, "add: bad arguments (count=%lld)", count);
    hipLaunchKernelGGL(add_kernel, dim3(grid_for(count / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const f32x4*)a, (const f32x4*)b, (f32x4*)out, count / 4);
    REFID_LAUNCH_CHECK("add");
    return 0;
}

extern "C" int refid_sum_n(const float* const* in, int n, float* out, long long count, void* stream) {
    REFID_CHECK(in && out && n >= 1 && n <= REFID_SUM_MAX && count > 0 && count % 4 == 0,
                "sum_n: 1..%d inputs, count a positive multiple of 4 (n=%d, count=%lld)", REFID_SUM_MAX, n, count);
    SumNArgs a;
    for (int k = 0; k < REFID_SUM_MAX; ++k) {
        a.in[k] = reinterpret_cast<const f32x4*>(k < n ? in[k] : in[0]);
        REFID_CHECK(a.in[k] != nullptr && (reinterpret_cast<uintptr_t>(a.in[k]) & 15) == 0, "sum_n: input %d is null or not 16-byte aligned", k);
    }
    a.n = n;
    hipLaunchKernelGGL(sum_n_kernel, dim3(grid_for(count / 4)), dim3(256), 0, (hipStream_t)stream, a, (f32x4*)out, count / 4);
    REFID_LAUNCH_CHECK("sum_n");
    return 0;
}

extern "C" int refid_act_bwd(const float* g, const float* y, float* out, float slope, int accumulate,
                             long long count, void* stream) {
    REFID_CHECK(g && y && out && count > 0 && count % 4 == 0, "act_bwd: bad arguments (count=%lld)", count);
    hipLaunchKernelGGL(act_bwd_kernel, dim3(grid_for(count / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const f32x4*)g, (const f32x4*)y, (f32x4*)out, slope, accumulate, count / 4);
    REFID_LAUNCH_CHECK("act_bwd");
    return 0;
}
