// Test-time pair assembly from a resident sequence: the key frames and the event stream of a sequence are uploaded once,
// and each pair (left frame, right frame, rows [row0, row1) of the stream) becomes one sample of `lq` / `voxel` in the
// layouts of sample.hip -- what the recurrent TEST datasets' __getitem__ builds (image_sharp_npy_dataset.py:145-225,
// image_npy_dataset.py:155-232) minus the ground truth, the crop and the flips.  Three kernels per call (grid.y/z walk
// the pairs through a device-resident table), after one memset.
//
// Arithmetic: event_fixed.h, shared with sample.hip -- fp32 normalisation in three roundings, 64-bit fixed point with 32
// fractional bits by integer atomics, one rounding to fp32.  Frames are u8 -> x / 255.f, one correctly rounded division.
//
// Padding: the network takes sides that are multiples of 2^num_encoders, frames come in any size (BS-ERGB: 970x625).  The
// outputs are (out_h, out_w) planes; the finish and frames kernels write EVERY element of them, so there is no separate
// fill: rows >= height / columns >= width hold zero in voxel channels and the last row / column in image channels
// (np.pad mode="edge").  The scratch is (height, width): the scatter never sees the padding.
//
// The single-image layout (refid_seq_assemble_single; sample.hip's LAYOUT_SINGLE minus the ground truth): one blurry frame
// per item -> lq (P, 3, oh, ow), voxel (P, bins, oh, ow) = the plain bins after voxel_norm (voxel_norm.h).  The statistics
// run over the UNPADDED (bins, h, w) scratch of an item, so an element's place in the fixed summation order depends on its
// index in the unpadded sample only and an item's voxel has the bits refid_assemble_single gives at a whole-frame crop;
// seq_single_finish_kernel adds the item's partials in index order (vn_mean_std), normalises and writes the padding.
#include <cstdint>

#include "common.h"
#include "event_fixed.h"
#include "voxel_norm.h"

namespace {

constexpr int LAYOUT_SINGLE = 2;   // refid_seq_assemble_single only: frame `left` -> lq (P, 3, oh, ow)

struct SeqGeom {
    int bins, m, n, layout;
    int h, w;            // frame
    int oh, ow;          // output plane
    int lq_chn;          // blur layout: channels of lq
    int bgr, row_pitch;
    long long frame_stride;
};

// grid = (chunks of the longest window, pairs)
__global__ __launch_bounds__(256) void seq_scatter_kernel(const float4* __restrict__ ev, const refid_seq_pair* __restrict__ tab,
                                                         SeqGeom g, unsigned long long* __restrict__ scratch) {
    const refid_seq_pair s = tab[blockIdx.y];
    const long long plane = (long long)g.h * g.w;
    unsigned long long* acc = scratch + (long long)blockIdx.y * g.bins * plane;
    float dT = s.last_stamp - s.first_stamp;
    if (dT == 0.f) dT = 1.f;                                                   // event_util.py:34-35
    const float scale = (float)(g.bins - 1);
    for (long long i = s.row0 + blockIdx.x * 256ll + threadIdx.x; i < s.row1; i += (long long)gridDim.x * 256) {
        EventTerm t;
        if (!event_term(ev[i], s.first_stamp, dT, scale, g.bins, g.w, g.h, t)) continue;
        event_add(acc + (long long)t.ti * plane + (long long)t.y * g.w + t.x, plane, g.bins, t);
    }
}

// grid = (chunks of the OUTPUT plane, bins, pairs); one thread = V consecutive elements of one output row
// (V == 4 only when ow % 4 == 0, so the four never straddle a row)
template <int V>
__global__ __launch_bounds__(256) void seq_finish_kernel(SeqGeom g, const long long* __restrict__ scratch,
                                                        float* __restrict__ lq, float* __restrict__ voxel) {
    const long long oplane = (long long)g.oh * g.ow;
    const long long e = (blockIdx.x * 256ll + threadIdx.x) * V;
    if (e >= oplane) return;
    const int i = blockIdx.y, b = blockIdx.z;
    const int r = (int)(e / g.ow), c0 = (int)(e % g.ow);
    const long long* src = scratch + ((long long)b * g.bins + i) * ((long long)g.h * g.w) + (long long)r * g.w;
    float v[V];
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = (r < g.h && c0 + k < g.w) ? fixed_to_float(src[c0 + k]) : 0.f;
    float* vox = voxel + (long long)b * (g.bins - 1) * 2 * oplane + e;          // (bins-1, 2, oh, ow)
    if (i < g.bins - 1) store_v<V>(vox + ((long long)i * 2 + 0) * oplane, v);  // image_npy_dataset.py:226-232
    if (i >= 1) store_v<V>(vox + ((long long)(i - 1) * 2 + 1) * oplane, v);
    if (g.layout == REFID_LAYOUT_BLUR) {                                       // image_npy_dataset.py:211-221
        float* l = lq + (long long)b * g.lq_chn * oplane + e;
        if (i >= 1 && i <= g.m - 1) store_v<V>(l + (long long)(3 + (i - 1)) * oplane, v);
        if (i >= g.m + 2 + g.n) store_v<V>(l + (long long)(3 + (g.m - 1) + 3 + (i - (g.m + 2 + g.n))) * oplane, v);
    }
}

// grid = (chunks of the OUTPUT plane, 2 key frames, pairs); one thread = V consecutive output pixels x 3 channels
template <int V>
__global__ __launch_bounds__(256) void seq_frames_kernel(const unsigned char* __restrict__ frames,
                                                        const refid_seq_pair* __restrict__ tab, SeqGeom g,
                                                        float* __restrict__ lq) {
    const long long oplane = (long long)g.oh * g.ow;
    const long long e = (blockIdx.x * 256ll + threadIdx.x) * V;
    if (e >= oplane) return;
    const int f = blockIdx.y, b = blockIdx.z;
    const refid_seq_pair s = tab[b];
    const unsigned char* src = frames + (long long)(f == 0 ? s.left : s.right) * g.frame_stride;
    const int r = min((int)(e / g.ow), g.h - 1), c0 = (int)(e % g.ow);         // edge replication: clamp the source
    const int rch = g.bgr ? 2 : 0;
    float c[3][V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const unsigned char* px = src + (long long)r * g.row_pitch + (long long)min(c0 + k, g.w - 1) * 3;
        c[0][k] = (float)px[rch] / 255.f;                                      // img_util.py:147 (true division)
        c[1][k] = (float)px[1] / 255.f;
        c[2][k] = (float)px[2 - rch] / 255.f;
    }
    float* dst;
    if (g.layout == LAYOUT_SINGLE) dst = lq + (long long)b * 3 * oplane;       // (launched with one frame per item: f == 0)
    else if (g.layout == REFID_LAYOUT_BLUR) dst = lq + ((long long)b * g.lq_chn + (f == 0 ? 0 : 3 + (g.m - 1))) * oplane;
    else dst = lq + ((long long)b * 2 + f) * 3 * oplane;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) store_v<V>(dst + ch * oplane + e, c[ch]);
}

// grid = (chunks of the OUTPUT plane, bins, items); one thread = V consecutive elements of one output row.  Writes every
// element of voxel (P, bins, oh, ow): inside the frame v != 0 ? (v - mean_f) / std_f : 0 with the item's statistics (every
// workgroup adds the item's partials itself, in index order), zero in the padding.  parts == nullptr: conversion only.
template <int V>
__global__ __launch_bounds__(256) void seq_single_finish_kernel(SeqGeom g, const long long* __restrict__ scratch,
                                                               const unsigned long long* __restrict__ parts, int chunks,
                                                               float* __restrict__ voxel) {
    __shared__ float sh_ms[2];
    __shared__ int sh_ok;
    const int i = blockIdx.y, b = blockIdx.z;
    if (parts && threadIdx.x == 0) sh_ok = vn_mean_std<long long>(parts + (long long)b * chunks * 3, chunks, sh_ms);
    __syncthreads();
    const long long oplane = (long long)g.oh * g.ow;
    const long long e = (blockIdx.x * 256ll + threadIdx.x) * V;
    if (e >= oplane) return;
    const int r = (int)(e / g.ow), c0 = (int)(e % g.ow);
    const long long* src = scratch + ((long long)b * g.bins + i) * ((long long)g.h * g.w) + (long long)r * g.w;
    float v[V];
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = (r < g.h && c0 + k < g.w) ? fixed_to_float(src[c0 + k]) : 0.f;
    if (parts) vn_apply<V>(v, sh_ok != 0, sh_ms[0], sh_ms[1]);
    store_v<V>(voxel + ((long long)b * g.bins + i) * oplane + e, v);
}

}  // namespace

#define SEQ_CHECK(cond, ...)                      \
    do {                                          \
        if (!(cond)) {                            \
            refid_set_error(__VA_ARGS__);         \
            return -1;                            \
        }                                         \
    } while (0)

extern "C" int refid_seq_assemble(const refid_seq_desc* d, int stages, void* stream) {
    SEQ_CHECK(d, "seq_assemble: null descriptor");
    SEQ_CHECK(d->lq && d->voxel, "seq_assemble: null outputs (lq %p, voxel %p)", (void*)d->lq, (void*)d->voxel);
    SEQ_CHECK(d->scratch, "seq_assemble: null scratch");
    SEQ_CHECK(d->pairs_host && d->pairs_dev && d->n_pairs > 0 && d->n_pairs <= 65535,
              "seq_assemble: n_pairs %d needs 1..65535 pairs and both pair tables", d->n_pairs);
    const int bins = refid_assemble_bins(d->m, d->n, d->layout);               // sets the error text itself
    if (bins < 0) return -1;
    SEQ_CHECK(d->n_events >= 0 && (d->n_events == 0 || d->events) && ((uintptr_t)d->events & 15) == 0,
              "seq_assemble: events must be %lld 16-byte aligned float32 rows", d->n_events);
    SEQ_CHECK(d->frames && d->n_frames > 0 && d->height > 0 && d->width > 0, "seq_assemble: no frames (n_frames %d, %dx%d)",
              d->n_frames, d->height, d->width);
    SEQ_CHECK((long long)d->row_pitch >= 3ll * d->width &&
              d->frame_stride >= (long long)(d->height - 1) * d->row_pitch + 3ll * d->width,
              "seq_assemble: row_pitch %d / frame_stride %lld too small for %dx%d frames", d->row_pitch, d->frame_stride,
              d->height, d->width);
    SEQ_CHECK(d->out_h >= d->height, "seq_assemble: out_h %d < height %d", d->out_h, d->height);
    SEQ_CHECK(d->out_w >= d->width, "seq_assemble: out_w %d < width %d", d->out_w, d->width);
    SEQ_CHECK((long long)d->out_h * d->out_w <= (1ll << 30), "seq_assemble: out_h x out_w %dx%d too large", d->out_h, d->out_w);
    long long max_rows = 0;
    for (int p = 0; p < d->n_pairs; ++p) {
        const refid_seq_pair& s = d->pairs_host[p];
        SEQ_CHECK(s.left >= 0 && s.left < d->n_frames, "seq_assemble: pair %d: left %d outside the %d frames", p, s.left, d->n_frames);
        SEQ_CHECK(s.right >= 0 && s.right < d->n_frames, "seq_assemble: pair %d: right %d outside the %d frames", p, s.right,
                  d->n_frames);
        SEQ_CHECK(s.row0 >= 0 && s.row0 <= s.row1, "seq_assemble: pair %d: row0 %lld > row1 %lld (or negative)", p, s.row0, s.row1);
        SEQ_CHECK(s.row1 <= d->n_events, "seq_assemble: pair %d: row1 %lld > n_events %lld", p, s.row1, d->n_events);
        if (s.row1 - s.row0 > max_rows) max_rows = s.row1 - s.row0;
    }
    SeqGeom g;
    g.bins = bins; g.m = d->m; g.n = d->n; g.layout = d->layout;
    g.h = d->height; g.w = d->width; g.oh = d->out_h; g.ow = d->out_w;
    g.lq_chn = 6 + 2 * (d->m - 1);
    g.bgr = d->bgr; g.row_pitch = d->row_pitch; g.frame_stride = d->frame_stride;
    const long long plane = (long long)g.h * g.w, oplane = (long long)g.oh * g.ow;
    hipStream_t st = (hipStream_t)stream;
    if (stages & REFID_ASSEMBLE_ZERO) {
        hipError_t e = hipMemsetAsync(d->scratch, 0, sizeof(long long) * (size_t)d->n_pairs * bins * plane, st);
        SEQ_CHECK(e == hipSuccess, "seq_assemble: memset failed: %s", hipGetErrorString(e));
    }
    if ((stages & REFID_ASSEMBLE_SCATTER) && max_rows > 0) {
        long long nbx = (max_rows + 255) / 256;
        if (nbx > 2048) nbx = 2048;
        hipLaunchKernelGGL(seq_scatter_kernel, dim3((unsigned)nbx, d->n_pairs), dim3(256), 0, st,
                           reinterpret_cast<const float4*>(d->events), d->pairs_dev, g,
                           reinterpret_cast<unsigned long long*>(d->scratch));
        REFID_LAUNCH_CHECK("seq_assemble: scatter");
    }
    // four-element stores: rows are a whole number of them, and every plane of both outputs starts 16-byte aligned
    const bool vec = (g.ow & 3) == 0 && (((uintptr_t)d->lq | (uintptr_t)d->voxel) & 15) == 0;
    const unsigned chunks = (unsigned)(((vec ? oplane / 4 : oplane) + 255) / 256);
    if (stages & REFID_ASSEMBLE_FINISH) {
        if (vec) hipLaunchKernelGGL(seq_finish_kernel<4>, dim3(chunks, bins, d->n_pairs), dim3(256), 0, st, g, d->scratch, d->lq, d->voxel);
        else hipLaunchKernelGGL(seq_finish_kernel<1>, dim3(chunks, bins, d->n_pairs), dim3(256), 0, st, g, d->scratch, d->lq, d->voxel);
        REFID_LAUNCH_CHECK("seq_assemble: finish");
    }
    if (stages & REFID_ASSEMBLE_FRAMES) {
        if (vec) hipLaunchKernelGGL(seq_frames_kernel<4>, dim3(chunks, 2, d->n_pairs), dim3(256), 0, st, d->frames, d->pairs_dev, g, d->lq);
        else hipLaunchKernelGGL(seq_frames_kernel<1>, dim3(chunks, 2, d->n_pairs), dim3(256), 0, st, d->frames, d->pairs_dev, g, d->lq);
        REFID_LAUNCH_CHECK("seq_assemble: frames");
    }
    return 0;
}

extern "C" int refid_seq_assemble_single(const refid_seq_single_desc* d, int stages, void* stream) {
    SEQ_CHECK(d, "seq_assemble_single: null descriptor");
    SEQ_CHECK(d->lq && d->voxel, "seq_assemble_single: null outputs (lq %p, voxel %p)", (void*)d->lq, (void*)d->voxel);
    SEQ_CHECK(d->scratch, "seq_assemble_single: null scratch");
    SEQ_CHECK(d->items_host && d->items_dev && d->n_items > 0 && d->n_items <= 65535,
              "seq_assemble_single: n_items %d needs 1..65535 items and both item tables", d->n_items);
    if (refid_single_bins(d->bins) < 0) return -1;                             // sets the error text itself
    SEQ_CHECK(d->bins <= 65535, "seq_assemble_single: bins %d > 65535", d->bins);
    SEQ_CHECK(!d->norm || (d->parts && ((uintptr_t)d->parts & 7) == 0),
              "seq_assemble_single: parts %p must be non-null and 8-byte aligned with norm", d->parts);
    SEQ_CHECK(d->n_events >= 0 && (d->n_events == 0 || d->events) && ((uintptr_t)d->events & 15) == 0,
              "seq_assemble_single: events must be %lld 16-byte aligned float32 rows", d->n_events);
    SEQ_CHECK(d->frames && d->n_frames > 0 && d->height > 0 && d->width > 0,
              "seq_assemble_single: no frames (n_frames %d, %dx%d)", d->n_frames, d->height, d->width);
    SEQ_CHECK((long long)d->row_pitch >= 3ll * d->width &&
              d->frame_stride >= (long long)(d->height - 1) * d->row_pitch + 3ll * d->width,
              "seq_assemble_single: row_pitch %d / frame_stride %lld too small for %dx%d frames", d->row_pitch,
              d->frame_stride, d->height, d->width);
    SEQ_CHECK(d->out_h >= d->height, "seq_assemble_single: out_h %d < height %d", d->out_h, d->height);
    SEQ_CHECK(d->out_w >= d->width, "seq_assemble_single: out_w %d < width %d", d->out_w, d->width);
    SEQ_CHECK((long long)d->out_h * d->out_w <= (1ll << 30), "seq_assemble_single: out_h x out_w %dx%d too large", d->out_h,
              d->out_w);
    const long long plane = (long long)d->height * d->width, oplane = (long long)d->out_h * d->out_w;
    const long long per_sample = d->bins * plane;                              // the UNPADDED sample: what the statistics see
    SEQ_CHECK(per_sample <= (1ll << 36), "seq_assemble_single: %d bins of %dx%d are too large", d->bins, d->height, d->width);
    long long max_rows = 0;
    for (int p = 0; p < d->n_items; ++p) {
        const refid_seq_pair& s = d->items_host[p];
        SEQ_CHECK(s.left >= 0 && s.left < d->n_frames, "seq_assemble_single: item %d: left %d outside the %d frames", p, s.left,
                  d->n_frames);
        SEQ_CHECK(s.row0 >= 0 && s.row0 <= s.row1, "seq_assemble_single: item %d: row0 %lld > row1 %lld (or negative)", p, s.row0,
                  s.row1);
        SEQ_CHECK(s.row1 <= d->n_events, "seq_assemble_single: item %d: row1 %lld > n_events %lld", p, s.row1, d->n_events);
        // every event adds exactly 2^32 of magnitude to the scratch, so below 2^30 events the int64 sum S1 cannot overflow
        SEQ_CHECK(!d->norm || s.row1 - s.row0 < (1ll << 30),
                  "seq_assemble_single: item %d: voxel_norm supports fewer than 2^30 events per item (%lld)", p, s.row1 - s.row0);
        if (s.row1 - s.row0 > max_rows) max_rows = s.row1 - s.row0;
    }
    SeqGeom g;
    g.bins = d->bins; g.m = 1; g.n = 0; g.layout = LAYOUT_SINGLE;
    g.h = d->height; g.w = d->width; g.oh = d->out_h; g.ow = d->out_w;
    g.lq_chn = 3;
    g.bgr = d->bgr; g.row_pitch = d->row_pitch; g.frame_stride = d->frame_stride;
    hipStream_t st = (hipStream_t)stream;
    if (stages & REFID_ASSEMBLE_ZERO) {
        hipError_t e = hipMemsetAsync(d->scratch, 0, sizeof(long long) * (size_t)d->n_items * per_sample, st);
        SEQ_CHECK(e == hipSuccess, "seq_assemble_single: memset failed: %s", hipGetErrorString(e));
    }
    if ((stages & REFID_ASSEMBLE_SCATTER) && max_rows > 0) {
        long long nbx = (max_rows + 255) / 256;
        if (nbx > 2048) nbx = 2048;
        hipLaunchKernelGGL(seq_scatter_kernel, dim3((unsigned)nbx, d->n_items), dim3(256), 0, st,
                           reinterpret_cast<const float4*>(d->events), d->items_dev, g,
                           reinterpret_cast<unsigned long long*>(d->scratch));
        REFID_LAUNCH_CHECK("seq_assemble_single: scatter");
    }
    if ((stages & REFID_ASSEMBLE_STATS) && d->norm) {
        if (int rc = voxel_norm_launch<long long>(d->scratch, nullptr, d->n_items, per_sample, d->parts, true, false, st,
                                                  "seq_assemble_single: stats")) return rc;
    }
    // four-element stores: rows are a whole number of them, and every plane of both outputs starts 16-byte aligned
    const bool vec = (g.ow & 3) == 0 && (((uintptr_t)d->lq | (uintptr_t)d->voxel) & 15) == 0;
    const unsigned chunks = (unsigned)(((vec ? oplane / 4 : oplane) + 255) / 256);
    if (stages & REFID_ASSEMBLE_FINISH) {
        const unsigned long long* parts = d->norm ? static_cast<const unsigned long long*>(d->parts) : nullptr;
        const int vn = (int)vn_chunks(per_sample);
        if (vec) hipLaunchKernelGGL(seq_single_finish_kernel<4>, dim3(chunks, d->bins, d->n_items), dim3(256), 0, st, g, d->scratch, parts, vn, d->voxel);
        else hipLaunchKernelGGL(seq_single_finish_kernel<1>, dim3(chunks, d->bins, d->n_items), dim3(256), 0, st, g, d->scratch, parts, vn, d->voxel);
        REFID_LAUNCH_CHECK("seq_assemble_single: finish");
    }
    if (stages & REFID_ASSEMBLE_FRAMES) {
        if (vec) hipLaunchKernelGGL(seq_frames_kernel<4>, dim3(chunks, 1, d->n_items), dim3(256), 0, st, d->frames, d->items_dev, g, d->lq);
        else hipLaunchKernelGGL(seq_frames_kernel<1>, dim3(chunks, 1, d->n_items), dim3(256), 0, st, d->frames, d->items_dev, g, d->lq);
        REFID_LAUNCH_CHECK("seq_assemble_single: frames");
    }
    return 0;
}
