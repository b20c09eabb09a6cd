// The event arithmetic shared by the two assemblers (sample.hip: training batches, sequence.hip: frame pairs of a
// resident sequence): the fp32 time normalisation of event_util.py:37, the frame test, and the 64-bit fixed-point
// bilinear weights.  One definition, so that both produce the same bits by construction.
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
