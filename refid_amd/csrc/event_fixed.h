// What the two assemblers share (sample.hip: training batches, sequence.hip: frame pairs of a resident sequence): the
// event arithmetic -- the fp32 time normalisation of event_util.py:37, the frame test, the 64-bit fixed-point bilinear
// weights -- and where a bin plane and a frame go in `lq` / `voxel`.  One definition: the same bits by construction.
#pragma once
#include "common.h"

constexpr float REFID_TWO32 = 4294967296.f;

struct EventTerm {
    int x, y;            // pixel in frame coordinates (truncated)
    int ti;              // left bin, 0 <= ti < bins
    long long q;         // (ts - ti) * 2^32: the right bin's weight; the left bin's is 2^32 - q
    bool pos;            // polarity > 0 counts as +1, everything else as -1
};

// e = [t, x, y, p].  False: the event is dropped (negative or NaN normalised time, ti >= bins, outside the frame).
__device__ __forceinline__ bool event_term(const float4 e, float first_stamp, float dT, float scale, int bins, int width,
                                           int height, EventTerm& o) {
#pragma clang fp contract(off)
    const float ts = (scale * (e.x - first_stamp)) / dT;                       // event_util.py:37, three fp32 roundings
    if (!(ts >= 0.f && ts < (float)bins)) return false;
    if (!(e.y > -1.f && e.y < (float)width && e.z > -1.f && e.z < (float)height)) return false;
    o.x = (int)e.y;                                                            // astype(int): truncation
    o.y = (int)e.z;
    o.ti = (int)ts;
    const float dts = ts - (float)o.ti;                                        // exact
    o.q = (long long)(dts * REFID_TWO32);                                      // exact product, < 2^32
    o.pos = e.w > 0.f;
    return true;
}

// right bin += pol*q, left bin += pol*(2^32 - q), by integer atomics: the sums do not depend on arrival order
__device__ __forceinline__ void event_add(unsigned long long* p, long long plane, int bins, const EventTerm& t) {
    const long long one = 1ll << 32;
    atomicAdd(p, (unsigned long long)(t.pos ? one - t.q : t.q - one));         // left bin: ti < bins holds
    if (t.ti + 1 < bins) atomicAdd(p + plane, (unsigned long long)(t.pos ? t.q : -t.q));
}

__device__ __forceinline__ float fixed_to_float(long long a) { return (float)a * (1.f / REFID_TWO32); }   // RNE, then exact

template <int V>
__device__ __forceinline__ void store_v(float* p, const float* v) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else p[0] = v[0];
}

// The output layouts both assemblers write.  `G` is their geometry (BatchGeom, SeqGeom): bins, m, n, layout, lq_chn.
constexpr int LAYOUT_SINGLE = 2;   // the single-image entry points only: one frame -> lq (B, 3, h, w), plain bins -> voxel

// V elements at offset e of bin plane i of sample b -> its slots of the sliding pairs voxel (B, bins-1, 2, h, w) and, in
// the blur layout, its event channel of lq
template <int V, class G>
__device__ __forceinline__ void store_bin_plane(const G g, int b, int i, long long plane, long long e, const float* v,
                                                float* lq, float* voxel) {
    float* vox = voxel + (long long)b * (g.bins - 1) * 2 * plane + e;
    if (i < g.bins - 1) store_v<V>(vox + ((long long)i * 2 + 0) * plane, v);   // image_npy_dataset.py:226-232
    if (i >= 1) store_v<V>(vox + ((long long)(i - 1) * 2 + 1) * plane, v);
    if (g.layout == REFID_LAYOUT_BLUR) {                                       // image_npy_dataset.py:211-221
        float* l = lq + (long long)b * g.lq_chn * plane + e;
        if (i >= 1 && i <= g.m - 1) store_v<V>(l + (long long)(3 + (i - 1)) * plane, v);
        if (i >= g.m + 2 + g.n) store_v<V>(l + (long long)(3 + (g.m - 1) + 3 + (i - (g.m + 2 + g.n))) * plane, v);
    }
}

// where the three channel planes of input frame f (0: left / blurry, 1: right) of sample b start in lq
template <class G>
__device__ __forceinline__ float* lq_frame_dst(const G g, float* lq, int b, int f, long long plane) {
    if (g.layout == LAYOUT_SINGLE) return lq + (long long)b * 3 * plane;
    if (g.layout == REFID_LAYOUT_BLUR) return lq + ((long long)b * g.lq_chn + (f == 0 ? 0 : 3 + (g.m - 1))) * plane;
    return lq + ((long long)b * 2 + f) * 3 * plane;
}

// v = columns c0 .. c0+V-1 of row r of an (h, w) scratch plane (`row`: where that row starts); zero outside the plane
template <int V, class G>
__device__ __forceinline__ void load_padded(const G g, const long long* row, int r, int c0, float* v) {
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = (r < g.h && c0 + k < g.w) ? fixed_to_float(row[c0 + k]) : 0.f;
}

// grid.x of the scatter kernels: at most 2048 workgroups of 256 striding over the longest event list of the launch
static inline unsigned scatter_grid_x(long long rows) { return (unsigned)(rows > 2047 * 256ll ? 2048 : (rows + 255) / 256); }
