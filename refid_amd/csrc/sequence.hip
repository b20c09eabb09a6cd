// Test-time pair assembly from a resident sequence: the key frames and the event stream of a sequence are uploaded once,
// and each pair (left frame, right frame, rows [row0, row1) of the stream) becomes one sample of `lq` / `voxel` in the
// layouts of sample.hip -- what the recurrent TEST datasets' __getitem__ builds (image_sharp_npy_dataset.py:145-225,
// image_npy_dataset.py:155-232) minus the ground truth, the crop and the flips.  Three kernels per call (grid.y/z walk
// the pairs through a device-resident table), after one memset.
//
// Arithmetic and output layouts: event_fixed.h, shared with sample.hip -- fp32 normalisation in three roundings, 64-bit fixed
// point with 32 fractional bits by integer atomics, one rounding to fp32.  Frames are u8 -> x / 255.f, one correctly rounded
// division.  Host side: seq_plan.h has the argument checks of both entry points, seq_launch below their launch sequence.
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
#include "seq_plan.h"
#include "voxel_norm.h"

namespace {

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
    load_padded<V>(g, src, r, c0, v);
    store_bin_plane<V>(g, b, i, oplane, e, v, lq, voxel);
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
    float* dst = lq_frame_dst(g, lq, b, f, oplane);                            // (single: one frame per item, f == 0)
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
    load_padded<V>(g, src, r, c0, v);
    if (parts) vn_apply<V>(v, sh_ok != 0, sh_ms[0], sh_ms[1]);
    store_v<V>(voxel + ((long long)b * g.bins + i) * oplane + e, v);
}

}  // namespace

static int seq_launched(const char* who, const char* stage) {                  // REFID_LAUNCH_CHECK with the caller's prefix
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) refid_set_error("%s: %s: launch failed: %s", who, stage, hipGetErrorString(e));
    return e != hipSuccess ? 2 : 0;
}

static SeqGeom seq_geom(const SeqArgs& a, int bins, int m, int n, int layout) {
    SeqGeom g;
    g.bins = bins; g.m = m; g.n = n; g.layout = layout;
    g.h = a.height; g.w = a.width; g.oh = a.out_h; g.ow = a.out_w;
    g.lq_chn = layout == LAYOUT_SINGLE ? 3 : 6 + 2 * (m - 1);
    g.bgr = a.bgr; g.row_pitch = a.row_pitch; g.frame_stride = a.frame_stride;
    return g;
}

// The stages of both entry points in their order: zero, scatter, the entry point's own `finish(vec, chunks)` (its
// statistics and finish launches, which test `stages` themselves; non-zero: returned), frames (n_frames per item).
// vec: four-element stores; chunks: grid.x of the finish and frames kernels.
template <class Finish>
static int seq_launch(const SeqArgs& a, const SeqGeom& g, long long max_rows, int n_frames, int stages, hipStream_t st,
                      Finish finish) {
    const long long plane = (long long)g.h * g.w, oplane = (long long)g.oh * g.ow;
    if (stages & REFID_ASSEMBLE_ZERO) {
        hipError_t e = hipMemsetAsync(a.scratch, 0, sizeof(long long) * (size_t)a.count * g.bins * plane, st);
        SEQ_CHECK(e == hipSuccess, "%s: memset failed: %s", a.who, hipGetErrorString(e));
    }
    if ((stages & REFID_ASSEMBLE_SCATTER) && max_rows > 0) {
        hipLaunchKernelGGL(seq_scatter_kernel, dim3(scatter_grid_x(max_rows), a.count), dim3(256), 0, st,
                           reinterpret_cast<const float4*>(a.events), a.tab_dev, g,
                           reinterpret_cast<unsigned long long*>(a.scratch));
        if (int rc = seq_launched(a.who, "scatter")) return rc;
    }
    // four-element stores: rows are a whole number of them, and every plane of both outputs starts 16-byte aligned
    const bool vec = (g.ow & 3) == 0 && (((uintptr_t)a.lq | (uintptr_t)a.voxel) & 15) == 0;
    const unsigned chunks = (unsigned)(((vec ? oplane / 4 : oplane) + 255) / 256);
    if (int rc = finish(vec, chunks)) return rc;
    if (stages & REFID_ASSEMBLE_FRAMES) {
        if (vec) hipLaunchKernelGGL(seq_frames_kernel<4>, dim3(chunks, n_frames, a.count), dim3(256), 0, st, a.frames, a.tab_dev, g, a.lq);
        else hipLaunchKernelGGL(seq_frames_kernel<1>, dim3(chunks, n_frames, a.count), dim3(256), 0, st, a.frames, a.tab_dev, g, a.lq);
        return seq_launched(a.who, "frames");
    }
    return 0;
}

extern "C" int refid_seq_assemble(const refid_seq_desc* d, int stages, void* stream) {
    SEQ_CHECK(d, "seq_assemble: null descriptor");
    const SeqArgs a{d->events, d->n_events, d->frames, d->n_frames, d->frame_stride, d->row_pitch, d->height, d->width, d->bgr,
                    d->pairs_host, d->pairs_dev, d->n_pairs, d->out_h, d->out_w, d->scratch, d->lq, d->voxel,
                    "seq_assemble", "pair", "n_pairs", /*check_right*/ true, /*limit_events*/ false};
    long long max_rows = 0;
    if (seq_check(a, &max_rows)) return -1;
    const int bins = refid_assemble_bins(d->m, d->n, d->layout);               // sets the error text itself
    if (bins < 0) return -1;
    const SeqGeom g = seq_geom(a, bins, d->m, d->n, d->layout);
    hipStream_t st = (hipStream_t)stream;
    return seq_launch(a, g, max_rows, 2, stages, st, [&](bool vec, unsigned chunks) {
        if (!(stages & REFID_ASSEMBLE_FINISH)) return 0;
        if (vec) hipLaunchKernelGGL(seq_finish_kernel<4>, dim3(chunks, bins, a.count), dim3(256), 0, st, g, a.scratch, a.lq, a.voxel);
        else hipLaunchKernelGGL(seq_finish_kernel<1>, dim3(chunks, bins, a.count), dim3(256), 0, st, g, a.scratch, a.lq, a.voxel);
        return seq_launched(a.who, "finish");
    });
}

extern "C" int refid_seq_assemble_single(const refid_seq_single_desc* d, int stages, void* stream) {
    SEQ_CHECK(d, "seq_assemble_single: null descriptor");
    const SeqArgs a{d->events, d->n_events, d->frames, d->n_frames, d->frame_stride, d->row_pitch, d->height, d->width, d->bgr,
                    d->items_host, d->items_dev, d->n_items, d->out_h, d->out_w, d->scratch, d->lq, d->voxel,
                    "seq_assemble_single", "item", "n_items", /*check_right*/ false, /*limit_events*/ d->norm != 0};
    long long max_rows = 0;
    if (seq_check(a, &max_rows)) return -1;
    if (refid_single_bins(d->bins) < 0) return -1;                             // sets the error text itself
    SEQ_CHECK(d->bins <= 65535, "seq_assemble_single: bins %d > 65535", d->bins);
    SEQ_CHECK(!d->norm || (d->parts && ((uintptr_t)d->parts & 7) == 0),
              "seq_assemble_single: parts %p must be non-null and 8-byte aligned with norm", d->parts);
    const long long per_sample = (long long)d->bins * d->height * d->width;   // the UNPADDED sample: what the statistics see
    SEQ_CHECK(per_sample <= (1ll << 36), "seq_assemble_single: %d bins of %dx%d are too large", d->bins, d->height, d->width);
    const SeqGeom g = seq_geom(a, d->bins, 1, 0, LAYOUT_SINGLE);
    hipStream_t st = (hipStream_t)stream;
    return seq_launch(a, g, max_rows, 1, stages, st, [&](bool vec, unsigned chunks) {
        if ((stages & REFID_ASSEMBLE_STATS) && d->norm) {
            if (int rc = voxel_norm_launch<long long>(a.scratch, nullptr, a.count, per_sample, d->parts, true, false, st,
                                                      "seq_assemble_single: stats")) return rc;
        }
        if (!(stages & REFID_ASSEMBLE_FINISH)) return 0;
        const unsigned long long* parts = d->norm ? static_cast<const unsigned long long*>(d->parts) : nullptr;
        const int vn = (int)vn_chunks(per_sample);
        if (vec) hipLaunchKernelGGL(seq_single_finish_kernel<4>, dim3(chunks, d->bins, a.count), dim3(256), 0, st, g, a.scratch, parts, vn, a.voxel);
        else hipLaunchKernelGGL(seq_single_finish_kernel<1>, dim3(chunks, d->bins, a.count), dim3(256), 0, st, g, a.scratch, parts, vn, a.voxel);
        return seq_launched(a.who, "finish");
    });
}
