// Training-batch assembly on the device: what the recurrent datasets' __getitem__ does between "frames and events are in
// memory" and "lq / voxel / gt tensors" (basicsr/data/image_npy_dataset.py:188-232, image_sharp_npy_dataset.py:180-225):
//   * events_to_voxel_grid on the FLOAT32 event rows the datasets build (image_npy_dataset.py:155-163, event_util.py:6-66),
//     restricted to the crop window,
//   * triple_random_crop + augment (transforms.py:110-129, 212-231): crop, hflip, vflip, transpose,
//   * img2tensor + imfrombytes' /255 (img_util.py:9-33, 147): BGR -> RGB, HWC -> CHW, float32,
//   * lq = blur0 | bins 1..m-1 | blur1 | bins m+2+n.. and the sliding two-bin `voxel` (:211-232; event_fixed.h's helpers).
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
// NOT reproduced either: voxel_norm (event_util.py:141-160) of a sample whose non-zero elements have no spread (one
// element, or all equal) divides 0 by 0 and returns an all-NaN voxel; here such a sample's voxel is all zeros.
//
// The single-image layout (data/Single_image_npy_dataset.py:136-201): lq (B,3,h,w) from frame 0, gt (B,3,h,w) from frame 1,
// voxel (B,bins,h,w) = the plain bins after voxel_norm, the one data-dependent step: a reduction over the sample between
// the scatter and the finish; its kernels are in voxel_norm.h, shared with sequence.hip.
// voxel_stats_kernel writes one partial {S0, S1, S2} per (sample, chunk of 4096 elements),
// voxel_apply_kernel sums a sample's partials in index order and normalises.  S0 (the count of non-zero elements) is an
// integer; on the fused route S1 is an exact int64 sum of v * 2^32 (v = fixed_to_float(a) is a multiple of 2^-32: an
// integer rounded to 24 bits is an integer); S2 = sum v^2 is FLOAT64 IN A FIXED TREE ORDER: every product is exact in
// float64, a thread adds its 16 elements e = chunk*4096 + k*256 + t in the order k = 0..15, the 64 lanes of a wave are
// added by the xor tree 1, 2, 4, .., 32 (adjacent pairs first), the four waves and then the chunks in index order.  The
// order depends on the element's index inside the sample only: not on the batch, the sample's place in it, or the run.
#include <cstdint>

#include "common.h"
#include "event_fixed.h"
#include "voxel_norm.h"

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
    store_bin_plane<V>(g, b, i, plane, e, v, lq, voxel);
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
    float* dst;                                                                // single: frame 1 -> gt, laid out as lq
    if (g.layout == LAYOUT_SINGLE) dst = lq_frame_dst(g, f == 0 ? lq : gt, b, f, plane);
    else if (f >= 2) dst = gt + ((long long)b * (g.bins - 1) + (f - 2)) * 3 * plane;
    else dst = lq_frame_dst(g, lq, b, f, plane);
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

// The per-sample checks both assemblers make on the host table; max_events: the longest event list of the batch
static int check_samples(const refid_sample_desc* tab, int batch, int crop_h, int crop_w, long long* max_events) {
    REFID_CHECK((long long)crop_h * crop_w <= (1ll << 30), "assemble: crop %dx%d too large", crop_h, crop_w);
    bool any_rot = false;
    *max_events = 0;
    for (int b = 0; b < batch; ++b) {
        const refid_sample_desc& s = tab[b];
        REFID_CHECK(s.n_events >= 0 && (s.n_events == 0 || s.events) && ((uintptr_t)s.events & 15) == 0,
                    "assemble: sample %d: events must be %lld 16-byte aligned float32 rows", b, s.n_events);
        REFID_CHECK(s.frames && s.height > 0 && s.width > 0, "assemble: sample %d: no frames", b);
        REFID_CHECK(s.top >= 0 && s.left >= 0 && s.top + crop_h <= s.height && s.left + crop_w <= s.width,
                    "assemble: sample %d: crop %dx%d at (%d,%d) does not fit inside the %dx%d frame", b, crop_h, crop_w,
                    s.top, s.left, s.height, s.width);
        const long long wy = (long long)s.top - s.y0, wx = (long long)s.left - s.x0;
        REFID_CHECK(s.y0 >= 0 && s.x0 >= 0 && wy >= 0 && wx >= 0 && s.row_pitch > 0 && (wx + crop_w) * 3 <= s.row_pitch &&
                    (wy + crop_h) * s.row_pitch <= s.frame_stride,
                    "assemble: sample %d: crop %dx%d at (%d,%d) does not fit inside the uploaded window (origin (%d,%d), row "
                    "pitch %d, frame stride %lld)", b, crop_h, crop_w, s.top, s.left, s.y0, s.x0, s.row_pitch, s.frame_stride);
        any_rot = any_rot || s.rot90;
        if (s.n_events > *max_events) *max_events = s.n_events;
    }
    REFID_CHECK(!any_rot || crop_h == crop_w, "assemble: rot90 (a transpose) needs a square crop, got %dx%d", crop_h, crop_w);
    return 0;
}

// stages zero and scatter of both assemblers
static int launch_zero_scatter(const refid_sample_desc* tab_dev, int batch, const BatchGeom& g, long long max_events,
                               long long* scratch, int stages, hipStream_t st) {
    const long long plane = (long long)g.oh * g.ow;
    if (stages & REFID_ASSEMBLE_ZERO) {
        hipError_t e = hipMemsetAsync(scratch, 0, sizeof(long long) * (size_t)batch * g.bins * plane, st);
        REFID_CHECK(e == hipSuccess, "assemble: memset failed: %s", hipGetErrorString(e));
    }
    if ((stages & REFID_ASSEMBLE_SCATTER) && max_events > 0) {
        hipLaunchKernelGGL(sample_scatter_kernel, dim3(scatter_grid_x(max_events), batch), dim3(256), 0, st, tab_dev, g,
                           reinterpret_cast<unsigned long long*>(scratch));
        REFID_LAUNCH_CHECK("assemble: scatter");
    }
    return 0;
}

// stage frames of both assemblers: n_frames u8 frames per sample
static int launch_frames(const refid_sample_desc* tab_dev, int batch, const BatchGeom& g, int n_frames, float* lq, float* gt,
                         hipStream_t st) {
    const long long plane = (long long)g.oh * g.ow;
    const bool vec = (plane & 3) == 0;                                         // planes stay 16-byte aligned
    const unsigned chunks = (unsigned)(((vec ? plane / 4 : plane) + 255) / 256);
    if (vec) hipLaunchKernelGGL(sample_frames_kernel<4>, dim3(chunks, n_frames, batch), dim3(256), 0, st, tab_dev, g, lq, gt);
    else hipLaunchKernelGGL(sample_frames_kernel<1>, dim3(chunks, n_frames, batch), dim3(256), 0, st, tab_dev, g, lq, gt);
    REFID_LAUNCH_CHECK("assemble: frames");
    return 0;
}

extern "C" int refid_assemble_batch(const refid_assemble_desc* d, int stages, void* stream) {
    REFID_CHECK(d && d->samples_host && d->samples_dev && d->batch > 0 && d->batch <= 65535 && d->crop_h > 0 && d->crop_w > 0 &&
                d->scratch && d->lq && d->voxel && d->gt, "assemble: bad arguments");
    const int bins = refid_assemble_bins(d->m, d->n, d->layout);
    if (bins < 0) return 1;
    long long max_events = 0;
    if (int rc = check_samples(d->samples_host, d->batch, d->crop_h, d->crop_w, &max_events)) return rc;
    BatchGeom g;
    g.bins = bins; g.m = d->m; g.n = d->n; g.layout = d->layout;
    g.ch = d->crop_h; g.cw = d->crop_w;
    g.oh = d->crop_h; g.ow = d->crop_w;                                        // (a transposed square keeps its shape)
    g.lq_chn = 6 + 2 * (d->m - 1);
    const long long plane = (long long)g.oh * g.ow;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = launch_zero_scatter(d->samples_dev, d->batch, g, max_events, d->scratch, stages, st)) return rc;
    if (stages & REFID_ASSEMBLE_FINISH) {
        const bool vec = (plane & 3) == 0;                                     // planes stay 16-byte aligned
        const unsigned chunks = (unsigned)(((vec ? plane / 4 : plane) + 255) / 256);
        if (vec) hipLaunchKernelGGL(sample_finish_kernel<4>, dim3(chunks, bins, d->batch), dim3(256), 0, st, g, d->scratch, d->lq, d->voxel);
        else hipLaunchKernelGGL(sample_finish_kernel<1>, dim3(chunks, bins, d->batch), dim3(256), 0, st, g, d->scratch, d->lq, d->voxel);
        REFID_LAUNCH_CHECK("assemble: finish");
    }
    if (stages & REFID_ASSEMBLE_FRAMES) return launch_frames(d->samples_dev, d->batch, g, bins + 1, d->lq, d->gt, st);
    return 0;
}

extern "C" long long refid_voxel_norm_parts(int batch, long long per_sample) {
    return (batch > 0 && per_sample > 0) ? 3 * (long long)batch * vn_chunks(per_sample) : 0;
}

extern "C" int refid_voxel_norm(const float* in, float* out, int batch, long long per_sample, void* parts, void* stream) {
    REFID_CHECK(in && out && parts && batch > 0 && batch <= 65535 && per_sample > 0 && per_sample <= (1ll << 36) &&
                ((uintptr_t)parts & 7) == 0, "voxel_norm: bad arguments (batch=%d, per_sample=%lld)", batch, per_sample);
    return voxel_norm_launch<float>(in, out, batch, per_sample, parts, true, true, (hipStream_t)stream, "voxel_norm");
}

extern "C" int refid_single_bins(int bins) {
    if (bins < 1) { refid_set_error("assemble: single layout needs num_bins >= 1 (num_bins=%d)", bins); return -1; }
    if (bins == 3) {
        refid_set_error("assemble: num_bins == 3 is not supported: the reference's img2tensor (img_util.py:23-24) takes a 3-bin "
                        "voxel for a BGR image and swaps bins 0 and 2");
        return -1;
    }
    return bins;
}

extern "C" int refid_assemble_single(const refid_single_desc* d, int stages, void* stream) {
    REFID_CHECK(d && d->samples_host && d->samples_dev && d->batch > 0 && d->batch <= 65535 && d->crop_h > 0 && d->crop_w > 0 &&
                d->scratch && d->lq && d->voxel && d->gt && (!d->norm || d->parts) && ((uintptr_t)d->parts & 7) == 0,
                "assemble: bad arguments");
    if (refid_single_bins(d->bins) < 0) return 1;
    long long max_events = 0;
    if (int rc = check_samples(d->samples_host, d->batch, d->crop_h, d->crop_w, &max_events)) return rc;
    // every event adds exactly 2^32 of magnitude to the scratch, so below 2^30 events the int64 sum S1 cannot overflow
    REFID_CHECK(!d->norm || max_events < (1ll << 30), "assemble: voxel_norm supports fewer than 2^30 events per sample (%lld)",
                max_events);
    BatchGeom g;
    g.bins = d->bins; g.m = 1; g.n = 0; g.layout = LAYOUT_SINGLE;
    g.ch = d->crop_h; g.cw = d->crop_w;
    g.oh = d->crop_h; g.ow = d->crop_w;
    g.lq_chn = 3;
    const long long per_sample = (long long)d->bins * g.oh * g.ow;             // scratch and voxel: the same flat (B, bins, h, w)
    REFID_CHECK(per_sample <= (1ll << 36), "assemble: %d bins of %dx%d are too large", d->bins, d->crop_h, d->crop_w);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = launch_zero_scatter(d->samples_dev, d->batch, g, max_events, d->scratch, stages, st)) return rc;
    const bool stats = (stages & REFID_ASSEMBLE_STATS) && d->norm, finish = (stages & REFID_ASSEMBLE_FINISH) != 0;
    if (int rc = voxel_norm_launch<long long>(d->scratch, d->voxel, d->batch, per_sample, d->norm ? d->parts : nullptr, stats,
                                              finish, st, "assemble: voxel_norm")) return rc;
    if (stages & REFID_ASSEMBLE_FRAMES) return launch_frames(d->samples_dev, d->batch, g, 2, d->lq, d->gt, st);
    return 0;
}
