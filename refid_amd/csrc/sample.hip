// Training-batch assembly on the device: what the recurrent datasets' __getitem__ does between "frames and events are in
// memory" and "lq / voxel / gt tensors" (basicsr/data/image_npy_dataset.py:188-232, image_sharp_npy_dataset.py:180-225):
//   * events_to_voxel_grid on the FLOAT32 event rows the datasets build (image_npy_dataset.py:155-163, event_util.py:6-66),
//     restricted to the crop window,
//   * triple_random_crop + augment (transforms.py:110-129, 212-231): crop, hflip, vflip, transpose,
//   * img2tensor + imfrombytes' /255 (img_util.py:9-33, 147): BGR -> RGB, HWC -> CHW, float32,
//   * lq = blur0 | bins 1..m-1 | blur1 | bins m+2+n.. and the sliding two-bin `voxel` (image_npy_dataset.py:211-232).
// Three kernels per BATCH (grid.y/z walk the samples through a device-resident descriptor table), after one memset.
//
// Arithmetic.  ts = (bins-1)*(t-first)/dT is three correctly rounded fp32 operations in the reference's order (numpy
// evaluates that expression on a float32 column), ti = (int)ts, dts = ts - ti (exact).  The two bilinear contributions
// pol*(1-dts) and pol*dts are accumulated as 64-bit fixed point with 32 fractional bits, q = (long long)(dts * 2^32):
// right bin += pol*q, left bin += pol*(2^32 - q), by integer atomics.  Integer adds commute, so the sums do not depend
// on arrival order, grid size or the other samples of the launch; a left/right pair adds to exactly +-2^32.  The finish
// kernel converts each sum to fp32 with ONE rounding (int64 -> fp32 RNE, then an exact scaling by 2^-32).
//
// NOT reproduced from the reference: its flat index xs + ys*W + tis*W*H (event_util.py:54-59) lets an event outside the
// frame, or with a negative normalised time, wrap or spill into another pixel / bin.  Such events are dropped here, as
// are events outside the crop window.  Polarity: > 0 counts as +1, everything else (0 or -1) as -1.
#include <cstdint>

#include "common.h"
#include "event_fixed.h"

namespace {

struct BatchGeom {
    int bins, m, n, layout;
    int ch, cw;          // crop (before the transpose)
    int oh, ow;          // output plane
    int lq_chn;          // blur layout: channels of lq
};

// (cy, cx) in the crop -> flat index in the output plane: hflip, vflip, then transpose (transforms.py:116-128)
__device__ __forceinline__ int out_index(const refid_sample_desc& s, const BatchGeom& g, int cy, int cx) {
    if (s.hflip) cx = g.cw - 1 - cx;
    if (s.vflip) cy = g.ch - 1 - cy;
    return s.rot90 ? cx * g.ow + cy : cy * g.ow + cx;
}

__global__ __launch_bounds__(256) void sample_scatter_kernel(const refid_sample_desc* __restrict__ tab, BatchGeom g,
                                                            unsigned long long* __restrict__ scratch) {
#pragma clang fp contract(off)
    const refid_sample_desc s = tab[blockIdx.y];
    const long long plane = (long long)g.oh * g.ow;
    unsigned long long* acc = scratch + (long long)blockIdx.y * g.bins * plane;
    float dT = s.last_stamp - s.first_stamp;
    if (dT == 0.f) dT = 1.f;                                                   // event_util.py:34-35
    const float scale = (float)(g.bins - 1);
    const float4* ev = reinterpret_cast<const float4*>(s.events);
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < s.n_events; i += (long long)gridDim.x * 256) {
        EventTerm t;
        if (!event_term(ev[i], s.first_stamp, dT, scale, g.bins, s.width, s.height, t)) continue;
        const int cy = t.y - s.top, cx = t.x - s.left;
        if (cy < 0 || cy >= g.ch || cx < 0 || cx >= g.cw) continue;
        event_add(acc + (long long)t.ti * plane + out_index(s, g, cy, cx), plane, g.bins, t);
    }
}

// grid = (chunks of the plane, bins, batch); one thread = V consecutive elements of one bin plane
template <int V>
__global__ __launch_bounds__(256) void sample_finish_kernel(BatchGeom g, const long long* __restrict__ scratch,
                                                           float* __restrict__ lq, float* __restrict__ voxel) {
    const long long plane = (long long)g.oh * g.ow;
    const long long e = (blockIdx.x * 256ll + threadIdx.x) * V;
    if (e >= plane) return;
    const int i = blockIdx.y, b = blockIdx.z;
    const long long* src = scratch + ((long long)b * g.bins + i) * plane + e;
    float v[V];
    if constexpr (V == 4) {
        const longlong2 a0 = *reinterpret_cast<const longlong2*>(src), a1 = *reinterpret_cast<const longlong2*>(src + 2);
        v[0] = fixed_to_float(a0.x); v[1] = fixed_to_float(a0.y); v[2] = fixed_to_float(a1.x); v[3] = fixed_to_float(a1.y);
    } else {
        v[0] = fixed_to_float(src[0]);
    }
    float* vox = voxel + (long long)b * (g.bins - 1) * 2 * plane + e;           // (bins-1, 2, h, w)
    if (i < g.bins - 1) store_v<V>(vox + ((long long)i * 2 + 0) * plane, v);   // image_npy_dataset.py:226-232
    if (i >= 1) store_v<V>(vox + ((long long)(i - 1) * 2 + 1) * plane, v);
    if (g.layout == REFID_LAYOUT_BLUR) {                                       // image_npy_dataset.py:211-221
        float* l = lq + (long long)b * g.lq_chn * plane + e;
        if (i >= 1 && i <= g.m - 1) store_v<V>(l + (long long)(3 + (i - 1)) * plane, v);
        if (i >= g.m + 2 + g.n) store_v<V>(l + (long long)(3 + (g.m - 1) + 3 + (i - (g.m + 2 + g.n))) * plane, v);
    }
}

// grid = (chunks of the plane, 2 + n_gt frames, batch); one thread = V consecutive output pixels x 3 channels
template <int V>
__global__ __launch_bounds__(256) void sample_frames_kernel(const refid_sample_desc* __restrict__ tab, BatchGeom g,
                                                           float* __restrict__ lq, float* __restrict__ gt) {
    const long long plane = (long long)g.oh * g.ow;
    const long long e = (blockIdx.x * 256ll + threadIdx.x) * V;
    if (e >= plane) return;
    const int f = blockIdx.y, b = blockIdx.z;
    const refid_sample_desc s = tab[b];
    const unsigned char* src = s.frames + (long long)f * s.frame_stride;
    float c[3][V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const int r = ((int)e + k) / g.ow, q = ((int)e + k) % g.ow;           // the plane has at most 2^30 elements
        int cy = s.rot90 ? q : r, cx = s.rot90 ? r : q;                        // undo transpose, vflip, hflip
        if (s.vflip) cy = g.ch - 1 - cy;
        if (s.hflip) cx = g.cw - 1 - cx;
        const unsigned char* px = src + (long long)(s.top - s.y0 + cy) * s.row_pitch + (long long)(s.left - s.x0 + cx) * 3;
        c[0][k] = (float)px[2] / 255.f;                                        // BGR -> RGB; img_util.py:147 (true division)
        c[1][k] = (float)px[1] / 255.f;
        c[2][k] = (float)px[0] / 255.f;
    }
    float* dst;
    if (f >= 2) dst = gt + ((long long)b * (g.bins - 1) + (f - 2)) * 3 * plane;
    else if (g.layout == REFID_LAYOUT_BLUR) dst = lq + ((long long)b * g.lq_chn + (f == 0 ? 0 : 3 + (g.m - 1))) * plane;
    else dst = lq + ((long long)b * 2 + f) * 3 * plane;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) store_v<V>(dst + ch * plane + e, c[ch]);
}

}  // namespace

extern "C" int refid_assemble_bins(int m, int n, int layout) {
    int bins;
    if (layout == REFID_LAYOUT_BLUR) {
        if (m < 1 || n < 0) { refid_set_error("assemble: blur layout needs m >= 1 and n >= 0 (m=%d, n=%d)", m, n); return -1; }
        bins = 2 * m + n + 1;
    } else if (layout == REFID_LAYOUT_SHARP) {
        if (m != 1 || n < 1) { refid_set_error("assemble: sharp layout needs m == 1 and n >= 1 (m=%d, n=%d)", m, n); return -1; }
        bins = n + 1;
    } else {
        refid_set_error("assemble: unknown layout %d", layout);
        return -1;
    }
    if (bins == 3) {
        refid_set_error("assemble: num_bins == 3 is not supported: the reference's img2tensor (img_util.py:23-24) takes a 3-bin "
                        "voxel for a BGR image and swaps bins 0 and 2");
        return -1;
    }
    return bins;
}

extern "C" int refid_assemble_batch(const refid_assemble_desc* d, int stages, void* stream) {
    REFID_CHECK(d && d->samples_host && d->samples_dev && d->batch > 0 && d->batch <= 65535 && d->crop_h > 0 && d->crop_w > 0 &&
                d->scratch && d->lq && d->voxel && d->gt, "assemble: bad arguments");
    const int bins = refid_assemble_bins(d->m, d->n, d->layout);
    if (bins < 0) return 1;
    REFID_CHECK((long long)d->crop_h * d->crop_w <= (1ll << 30), "assemble: crop %dx%d too large", d->crop_h, d->crop_w);
    long long max_events = 0;
    bool any_rot = false;
    for (int b = 0; b < d->batch; ++b) {
        const refid_sample_desc& s = d->samples_host[b];
        REFID_CHECK(s.n_events >= 0 && (s.n_events == 0 || s.events) && ((uintptr_t)s.events & 15) == 0,
                    "assemble: sample %d: events must be %lld 16-byte aligned float32 rows", b, s.n_events);
        REFID_CHECK(s.frames && s.height > 0 && s.width > 0, "assemble: sample %d: no frames", b);
        REFID_CHECK(s.top >= 0 && s.left >= 0 && s.top + d->crop_h <= s.height && s.left + d->crop_w <= s.width,
                    "assemble: sample %d: crop %dx%d at (%d,%d) does not fit inside the %dx%d frame", b, d->crop_h, d->crop_w,
                    s.top, s.left, s.height, s.width);
        const long long wy = (long long)s.top - s.y0, wx = (long long)s.left - s.x0;
        REFID_CHECK(s.y0 >= 0 && s.x0 >= 0 && wy >= 0 && wx >= 0 && s.row_pitch > 0 && (wx + d->crop_w) * 3 <= s.row_pitch &&
                    (wy + d->crop_h) * s.row_pitch <= s.frame_stride,
                    "assemble: sample %d: crop %dx%d at (%d,%d) does not fit inside the uploaded window (origin (%d,%d), row "
                    "pitch %d, frame stride %lld)", b, d->crop_h, d->crop_w, s.top, s.left, s.y0, s.x0, s.row_pitch, s.frame_stride);
        any_rot = any_rot || s.rot90;
        if (s.n_events > max_events) max_events = s.n_events;
    }
    REFID_CHECK(!any_rot || d->crop_h == d->crop_w, "assemble: rot90 (a transpose) needs a square crop, got %dx%d", d->crop_h,
                d->crop_w);
    BatchGeom g;
    g.bins = bins; g.m = d->m; g.n = d->n; g.layout = d->layout;
    g.ch = d->crop_h; g.cw = d->crop_w;
    g.oh = d->crop_h; g.ow = d->crop_w;                                        // (a transposed square keeps its shape)
    g.lq_chn = 6 + 2 * (d->m - 1);
    const long long plane = (long long)g.oh * g.ow;
    hipStream_t st = (hipStream_t)stream;
    if (stages & REFID_ASSEMBLE_ZERO) {
        hipError_t e = hipMemsetAsync(d->scratch, 0, sizeof(long long) * (size_t)d->batch * bins * plane, st);
        REFID_CHECK(e == hipSuccess, "assemble: memset failed: %s", hipGetErrorString(e));
    }
    if ((stages & REFID_ASSEMBLE_SCATTER) && max_events > 0) {
        long long nbx = (max_events + 255) / 256;
        if (nbx > 2048) nbx = 2048;
        hipLaunchKernelGGL(sample_scatter_kernel, dim3((unsigned)nbx, d->batch), dim3(256), 0, st, d->samples_dev, g,
                           reinterpret_cast<unsigned long long*>(d->scratch));
        REFID_LAUNCH_CHECK("assemble: scatter");
    }
    const bool vec = (plane & 3) == 0;                                         // planes stay 16-byte aligned
    const unsigned chunks = (unsigned)(((vec ? plane / 4 : plane) + 255) / 256);
    if (stages & REFID_ASSEMBLE_FINISH) {
        if (vec) hipLaunchKernelGGL(sample_finish_kernel<4>, dim3(chunks, bins, d->batch), dim3(256), 0, st, g, d->scratch, d->lq, d->voxel);
        else hipLaunchKernelGGL(sample_finish_kernel<1>, dim3(chunks, bins, d->batch), dim3(256), 0, st, g, d->scratch, d->lq, d->voxel);
        REFID_LAUNCH_CHECK("assemble: finish");
    }
    if (stages & REFID_ASSEMBLE_FRAMES) {
        if (vec) hipLaunchKernelGGL(sample_frames_kernel<4>, dim3(chunks, bins + 1, d->batch), dim3(256), 0, st, d->samples_dev, g, d->lq, d->gt);
        else hipLaunchKernelGGL(sample_frames_kernel<1>, dim3(chunks, bins + 1, d->batch), dim3(256), 0, st, d->samples_dev, g, d->lq, d->gt);
        REFID_LAUNCH_CHECK("assemble: frames");
    }
    return 0;
}
