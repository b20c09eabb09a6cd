// The event-based double integral: latent frames from key frames and events without a network, by the formulas of
// include/refid_hip.h ("Double integral"); tests/edi_ref.py restates them and the device is compared bit for bit.
//
// One launch per minibatch: blockIdx.y is the item, a lane owns one pixel of it.  The pixel's events are one contiguous,
// time-sorted segment of the packed stream (refid_amd.edi.EdiStream sorts the rows by pixel once per sequence).  The lane
//   1. finds its first event after s0 by binary search in the segment;
//   2. walks the segment merged with the sample instants of both exposures (or, for a continuous shutter, integrates the
//      piecewise-constant gain between the events) and keeps S_left, the level at s1 and S_right;
//   3. walks the segment again, which the first walk left in the cache, merged with the output instants, and writes the
//      three bytes of its pixel in every output frame.
// Levels are 64-bit integers in units of 2^-16 (a hot pixel with 2^31 events of the largest threshold stays below 2^51); the
// gain is the product of three float64 table entries held in LDS, so no transcendental runs here, and every float64
// operation is rounded once: contraction is off for the whole file.  Lanes of a wave walk segments of different lengths
// and meet again at every output frame, where a wave stores 192 contiguous bytes with each of its three byte stores: the
// frames may start at any byte, and a pixel's 3 bytes never fill a dword on their own.  No atomics: a workgroup counts its
// held pixels by ballot and writes one word of its own.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int EDI_THREADS = REFID_EDI_THREADS;
constexpr int EDI_T0 = 2 * REFID_EDI_CLAMP + 1;             // entries of exp(i)
constexpr long long EDI_LIMIT = (long long)REFID_EDI_CLAMP << 16;
static_assert(EDI_T0 + 512 == REFID_EDI_TABLE, "the three tables");

struct EdiArgs {
    const uint8_t* frames;
    const float* ev_t;
    const int8_t* ev_p;
    const int32_t* seg;
    const int32_t* items;
    const float* bounds;
    const float* samples;
    const float* instants;
    const double* tables;
    uint8_t* out;
    int32_t* clamped;
    double eps255;
    long long hw;
    int n_events, n_frames, n_instants, m, c_pos, c_neg;
};

__device__ __forceinline__ double edi_gain(long long level, const double* tab, bool& held) {
    const long long ec = level < -EDI_LIMIT ? -EDI_LIMIT : level > EDI_LIMIT ? EDI_LIMIT : level;
    held |= ec != level;
    const int v = (int)ec;
    const double first = tab[(v >> 16) + REFID_EDI_CLAMP] * tab[EDI_T0 + ((v >> 8) & 255)];
    return first * tab[EDI_T0 + 256 + (v & 255)];
}

// a pixel's segment [pos, end) and the level after the events before pos
struct EdiWalk {
    const float* t;
    const int8_t* p;
    int pos, end, c_pos, c_neg;
    long long level;
    __device__ __forceinline__ void step() { level += p[pos] > 0 ? c_pos : -c_neg, ++pos; }
    __device__ __forceinline__ void to(float tau) {
        while (pos < end && t[pos] <= tau) step();
    }
    // the integral of the gain over (from, until], levels relative to `base`, by the events in between
    __device__ __forceinline__ double integrate(float from, float until, long long base, const double* tab, bool& held) {
        double at = (double)from, acc = 0.0;
        while (pos < end && t[pos] <= until) {
            const double here = (double)t[pos];
            const double term = edi_gain(level - base, tab, held) * (here - at);
            acc = acc + term, at = here;
            step();
        }
        const double term = edi_gain(level - base, tab, held) * ((double)until - at);
        return acc + term;
    }
};

template <bool CONTINUOUS>
__global__ __launch_bounds__(EDI_THREADS) void edi_kernel(EdiArgs a) {
    __shared__ double s_tab[REFID_EDI_TABLE];
    __shared__ int s_held[EDI_THREADS / 64];
    const int tid = (int)threadIdx.x, item = (int)blockIdx.y;
    for (int i = tid; i < REFID_EDI_TABLE; i += EDI_THREADS) s_tab[i] = a.tables[i];
    __syncthreads();

    const long long pix = (long long)blockIdx.x * EDI_THREADS + tid;
    const int left = a.items[2 * item], right = a.items[2 * item + 1];
    const bool pair = right >= 0;
    // the entry checked the host's copy of the table; a device copy that differs must not lead outside `frames`
    const bool active = pix < a.hw && left >= 0 && left < a.n_frames && right < a.n_frames;
    bool held = false;
    if (active) {
        const float s0 = a.bounds[4 * item], e0 = a.bounds[4 * item + 1], s1 = a.bounds[4 * item + 2], e1 = a.bounds[4 * item + 3];
        int begin = a.seg[pix], end = a.seg[pix + 1];                   // (kept inside the stream whatever the table holds)
        begin = begin < 0 ? 0 : begin > a.n_events ? a.n_events : begin;
        end = end < begin ? begin : end > a.n_events ? a.n_events : end;
        int lo = begin, hi = end;                                       // the first event with t > s0
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (a.ev_t[mid] <= s0) lo = mid + 1;
            else hi = mid;
        }
        const int first = lo;
        EdiWalk w{a.ev_t, a.ev_p, first, end, a.c_pos, a.c_neg, 0ll};

        double s_left = 1.0, s_right = 1.0;
        long long base = 0ll;                                           // the level at s1
        if (CONTINUOUS) {
            const double area = w.integrate(s0, e0, 0ll, s_tab, held);
            if (s0 != e0) s_left = area / ((double)e0 - (double)s0);
            if (pair) {
                w.to(s1);
                base = w.level;
                const double other = w.integrate(s1, e1, base, s_tab, held);
                if (s1 != e1) s_right = other / ((double)e1 - (double)s1);
            }
        } else {
            const float* smp = a.samples + (long long)item * 2 * a.m;
            double acc = 0.0;
            for (int j = 0; j < a.m; ++j) {
                w.to(smp[j]);
                acc = acc + edi_gain(w.level, s_tab, held);
            }
            if (s0 != e0) s_left = acc / (double)a.m;
            if (pair) {
                w.to(s1);
                base = w.level;
                acc = 0.0;
                for (int j = 0; j < a.m; ++j) {
                    w.to(smp[a.m + j]);
                    acc = acc + edi_gain(w.level - base, s_tab, held);
                }
                if (s1 != e1) s_right = acc / (double)a.m;
            }
        }

        double key_l[3], key_r[3] = {0.0, 0.0, 0.0};
        const uint8_t* fl = a.frames + ((long long)left * a.hw + pix) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) key_l[c] = (double)fl[c] + a.eps255;
        if (pair) {
            const uint8_t* fr = a.frames + ((long long)right * a.hw + pix) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) key_r[c] = (double)fr[c] + a.eps255;
        }
        const double span = (double)s1 - (double)e0;
        w.pos = first, w.level = 0ll;
        for (int f = 0; f < a.n_instants; ++f) {
            const float tau = a.instants[(long long)item * a.n_instants + f];
            w.to(tau);
            const double g_l = edi_gain(w.level, s_tab, held);
            double g_r = 0.0, wgt = 0.0;
            if (pair) {
                g_r = edi_gain(w.level - base, s_tab, held);
                wgt = tau <= e0 ? 0.0 : tau >= s1 ? 1.0 : ((double)tau - (double)e0) / span;
            }
            uint8_t* o = a.out + (((long long)item * a.n_instants + f) * a.hw + pix) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double lat = key_l[c] * g_l;
                lat = lat / s_left;
                if (pair) {
                    double other = key_r[c] * g_r;
                    other = other / s_right;
                    lat = (1.0 - wgt) * lat;
                    other = wgt * other;
                    lat = lat + other;
                }
                lat = lat - a.eps255;
                o[c] = (uint8_t)fmin(fmax(rint(lat), 0.0), 255.0);
            }
        }
    }
    const unsigned long long votes = __ballot(held);
    if ((tid & 63) == 0) s_held[tid >> 6] = __popcll(votes);
    __syncthreads();
    if (tid == 0) {
        int total = 0;
#pragma unroll
        for (int i = 0; i < EDI_THREADS / 64; ++i) total += s_held[i];
        a.clamped[(long long)item * gridDim.x + blockIdx.x] = total;
    }
}

bool edi_aligned(const void* p, unsigned long long to) { return ((unsigned long long)p & (to - 1ull)) == 0; }
bool edi_finite(double v) { return v - v == 0.0; }

}  // namespace

extern "C" int refid_edi(const refid_edi_desc* d, void* stream) {
    REFID_CHECK(d, "edi: null descriptor");
    REFID_CHECK(d->n_items >= 1 && d->n_items <= REFID_EDI_MAX_ITEMS, "edi: n_items %d is not 1 .. %d", d->n_items, REFID_EDI_MAX_ITEMS);
    REFID_CHECK(d->n_instants >= 1 && d->n_instants <= REFID_EDI_MAX_INSTANTS, "edi: n_instants %d is not 1 .. %d", d->n_instants,
                REFID_EDI_MAX_INSTANTS);
    REFID_CHECK(d->exposure == REFID_EDI_SAMPLES || d->exposure == REFID_EDI_CONTINUOUS,
                "edi: exposure %d is neither REFID_EDI_SAMPLES (0) nor REFID_EDI_CONTINUOUS (1)", d->exposure);
    const bool sampled = d->exposure == REFID_EDI_SAMPLES;
    REFID_CHECK(!sampled || (d->m >= 1 && d->m <= REFID_BLUR_MAX_COUNT), "edi: m %d is not 1 .. %d", d->m, REFID_BLUR_MAX_COUNT);
    REFID_CHECK(d->height >= 1 && d->width >= 1, "edi: height %d and width %d must be positive", d->height, d->width);
    const long long hw = (long long)d->height * d->width;
    REFID_CHECK(hw <= REFID_EDI_MAX_PIXELS, "edi: height %d * width %d = %lld pixels exceed %d", d->height, d->width, hw, REFID_EDI_MAX_PIXELS);
    REFID_CHECK(d->n_frames >= 1, "edi: n_frames %d must be at least 1", d->n_frames);
    REFID_CHECK(d->n_events >= 0 && d->n_events < (1ll << 31), "edi: n_events %lld is not 0 .. 2^31 - 1", (long long)d->n_events);
    REFID_CHECK(d->c_pos >= 1 && d->c_pos <= REFID_EDI_MAX_THRESHOLD, "edi: c_pos %d is not 1 .. %d (units of 2^-16)", d->c_pos,
                REFID_EDI_MAX_THRESHOLD);
    REFID_CHECK(d->c_neg >= 1 && d->c_neg <= REFID_EDI_MAX_THRESHOLD, "edi: c_neg %d is not 1 .. %d (units of 2^-16)", d->c_neg,
                REFID_EDI_MAX_THRESHOLD);
    REFID_CHECK(edi_finite(d->eps255) && d->eps255 >= 0.0, "edi: eps255 %g must be finite and not negative", d->eps255);
    const struct { const void* p; const char* name; unsigned align; bool needed; } ptrs[] = {
        {d->frames, "frames", 1, true}, {d->ev_t, "ev_t", 4, d->n_events > 0}, {d->ev_p, "ev_p", 1, d->n_events > 0}, {d->seg, "seg", 4, true},
        {d->items_host, "items_host", 4, true}, {d->items, "items", 4, true}, {d->bounds_host, "bounds_host", 4, true},
        {d->bounds, "bounds", 4, true}, {d->samples_host, "samples_host", 4, false}, {d->samples, "samples", 4, false},
        {d->instants_host, "instants_host", 4, true}, {d->instants, "instants", 4, true}, {d->tables, "tables", 8, true},
        {d->out, "out", 1, true}, {d->clamped, "clamped", 4, true}};
    for (const auto& q : ptrs) {
        REFID_CHECK(q.p || !q.needed, "edi: %s is null", q.name);
        REFID_CHECK(edi_aligned(q.p, q.align), "edi: %s is not aligned to %u bytes", q.name, q.align);
    }
    REFID_CHECK((d->samples_host != nullptr) == (d->samples != nullptr), "edi: %s is null but %s is not (pass both copies of the table, or neither)",
                !d->samples_host ? "samples_host" : "samples", !d->samples_host ? "samples" : "samples_host");
    REFID_CHECK(!sampled || d->samples, "edi: samples is null in REFID_EDI_SAMPLES mode");
    REFID_CHECK(sampled || !d->samples, "edi: samples is given in REFID_EDI_CONTINUOUS mode, which reads none");
    for (int k = 0; k < d->n_items; ++k) {
        const int left = d->items_host[2 * k], right = d->items_host[2 * k + 1];
        REFID_CHECK(left >= 0 && left < d->n_frames, "edi: items[%d]: left %d lies outside the n_frames %d", k, left, d->n_frames);
        REFID_CHECK(right < d->n_frames, "edi: items[%d]: right %d lies outside the n_frames %d", k, right, d->n_frames);
        const bool pair = right >= 0;
        const float* b = d->bounds_host + 4 * k;
        for (int i = 0; i < (pair ? 4 : 2); ++i) REFID_CHECK(edi_finite(b[i]), "edi: bounds[%d][%d] is not finite", k, i);
        REFID_CHECK(b[0] <= b[1] && (!pair || (b[1] <= b[2] && b[2] <= b[3])),
                    "edi: bounds[%d] = [%.9g, %.9g, %.9g, %.9g] is not ordered s0 <= e0 <= s1 <= e1", k, b[0], b[1], b[2], b[3]);
        const float last = pair ? b[3] : b[1];
        const float* tau = d->instants_host + (long long)k * d->n_instants;
        for (int f = 0; f < d->n_instants; ++f) {
            REFID_CHECK(edi_finite(tau[f]) && tau[f] >= b[0] && tau[f] <= last, "edi: instants[%d][%d] = %.9g lies outside [%.9g, %.9g]", k, f,
                        tau[f], b[0], last);
            REFID_CHECK(f == 0 || tau[f] >= tau[f - 1], "edi: instants[%d] is not ascending: [%d] = %.9g after %.9g", k, f, tau[f], tau[f - 1]);
        }
        if (sampled) {
            for (int half = 0; half < (pair ? 2 : 1); ++half) {
                const float* smp = d->samples_host + ((long long)k * 2 + half) * d->m;
                const float from = b[2 * half], until = b[2 * half + 1];
                for (int j = 0; j < d->m; ++j) {
                    REFID_CHECK(edi_finite(smp[j]) && smp[j] >= from && smp[j] <= until, "edi: samples[%d][%d] = %.9g lies outside [%.9g, %.9g]", k,
                                half * d->m + j, smp[j], from, until);
                    REFID_CHECK(j == 0 || smp[j] >= smp[j - 1], "edi: samples[%d] is not ascending: [%d] = %.9g after %.9g", k, half * d->m + j,
                                smp[j], smp[j - 1]);
                }
            }
        }
    }
    EdiArgs a;
    a.frames = d->frames, a.ev_t = d->ev_t, a.ev_p = d->ev_p, a.seg = d->seg, a.items = d->items, a.bounds = d->bounds;
    a.samples = d->samples, a.instants = d->instants, a.tables = d->tables, a.out = d->out, a.clamped = d->clamped;
    a.eps255 = d->eps255, a.hw = hw, a.n_events = (int)d->n_events, a.n_frames = d->n_frames, a.n_instants = d->n_instants;
    a.m = d->m, a.c_pos = d->c_pos, a.c_neg = d->c_neg;
    const dim3 grid((unsigned)((hw + EDI_THREADS - 1) / EDI_THREADS), (unsigned)d->n_items);
    hipStream_t st = (hipStream_t)stream;
    if (sampled) hipLaunchKernelGGL(edi_kernel<false>, grid, dim3(EDI_THREADS), 0, st, a);
    else hipLaunchKernelGGL(edi_kernel<true>, grid, dim3(EDI_THREADS), 0, st, a);
    REFID_LAUNCH_CHECK("edi");
    return 0;
}
