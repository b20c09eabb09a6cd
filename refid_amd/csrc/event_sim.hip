// Events from high-frame-rate frames: the ESIM contrast-threshold model of include/refid_hip.h ("Simulated events"), in
// integers, restated in tests/event_sim_ref.py and compared bit for bit.
//
// One entry, refid_event_sim, whose `stage` names the launch (the caller puts a prefix sum, one synchronisation and a sort
// between them; refid_amd/ops.py::event_sim does):
//   RESET   state[pix] = lut[Y8(frame 0)]
//   COUNT   a lane per pixel walks the chunk's intervals with `ref` in a register and writes the pixel's number of rows;
//           a wave sums an interval's rows over its lanes and adds them to the workgroup's LDS table, which the workgroup
//           adds to totals[k] at its end.  `state` is not touched.
//   EMIT    the same walk (one __device__ body, esim_walk<EMIT>): each row leaves as one 16-byte store into the pixel's
//           slots [ends[pix-1], ends[pix]), with its 64-bit sort key beside it; the final `ref` goes to `state`.
//   GATHER  sorted[i] = rows[perm[i]], 16 bytes per lane.
// Integer atomics only (the per-interval totals and the flag word: sums and ORs of integers do not depend on arrival
// order); no floating-point atomics.  The loop over a pixel's events ends at REFID_EVENT_SIM_CAP whatever it reads, and an
// EMIT lane never stores outside its slots: bad data raises a flag bit instead.
//
// Launch shape: 256 lanes, a pixel each.  A wave reads 192 consecutive bytes of a frame with three byte loads per lane
// (any alignment of `frames`); a 1280x720 frame gives 3600 workgroups, 14 per CU, and the walk needs few registers, so
// occupancy is bounded by the grid, not by registers or LDS (3 KiB).  The time goes to the frames' bytes (read once per
// pass) and, where events are dense, to the 64-bit division per event and the scattered 16-byte row stores.
#include "common.h"
#include "workgroup.h"

namespace {

constexpr int ESIM_THREADS = 256;
constexpr int ESIM_MAX_FRAMES = REFID_EVENT_SIM_MAX_FRAMES;
constexpr int ESIM_CAP = REFID_EVENT_SIM_CAP;

__device__ __forceinline__ int esim_y8(const uint8_t* __restrict__ px, int bgr) {
    const int c0 = px[0], g = px[1], c2 = px[2];
    const int r = bgr ? c2 : c0, b = bgr ? c0 : c2;
    return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
}

struct EsimArgs {
    const uint8_t* frames;
    const double* stamps;
    const int32_t* lut;
    const int32_t* c_pos_map;
    const int32_t* c_neg_map;
    int32_t* state;
    int32_t* counts;
    unsigned long long* totals;
    const long long* ends;
    float4* rows;
    long long* keys;
    long long hw, n_rows;
    int n_frames,width, bgr, c_pos, c_neg;
};

// t = fl32(t0 + (t1 - t0) * (double(tick) * 2^-20)): three float64 operations, each rounded once (the scaling of tick is exact)
__device__ __forceinline__ float esim_stamp(double t0, double t1, long long tick) {
#pragma clang fp contract(off)
    const double dt = t1 - t0;
    const double frac = (double)tick * 0x1p-20;
    const double part = dt * frac;
    const double t = t0 + part;
    return (float)t;
}

template <bool EMIT>
__global__ __launch_bounds__(ESIM_THREADS) void esim_walk(const EsimArgs p) {
    __shared__ int32_t s_lut[256];
    __shared__ unsigned s_rows[ESIM_MAX_FRAMES];                // rows per interval of this workgroup (COUNT)
    const int tid = threadIdx.x;
    s_lut[tid] = p.lut[tid];                                   // (ESIM_THREADS == 256)
    if (!EMIT)
        for (int k = tid; k < p.n_frames - 1; k += ESIM_THREADS) s_rows[k] = 0u;
    __syncthreads();
    const long long pix = (long long)blockIdx.x * ESIM_THREADS + tid;
    const bool on = pix < p.hw;
    long long ref = 0, a = 0, cp = 1, cn = 1, slot = 0, slot_end = 0;
    const uint8_t* px = p.frames;
    float fx = 0.f, fy = 0.f;
    unsigned flag = 0u;
    if (on) {
        px += pix * 3;
        cp = p.c_pos_map ? p.c_pos_map[pix] : p.c_pos;
        cn = p.c_neg_map ? p.c_neg_map[pix] : p.c_neg;
        ref = p.state[pix];
        a = s_lut[esim_y8(px, p.bgr)];
        if (EMIT) {
            slot = max(pix ? p.ends[pix - 1] : 0ll, 0ll);      // (clamped: a wrong `ends` raises the flag, it moves no store)
            slot_end = min(p.ends[pix], p.n_rows);
            const long long y = pix / p.width;
            fy = (float)y, fx = (float)(pix - y * p.width);
        }
    }
    unsigned total = 0u;
    for (int k = 0; k + 1 < p.n_frames; ++k) {                 // (uniform: every lane of a wave takes part in the sum below)
        unsigned cnt = 0u;
        if (on) {
            px += p.hw * 3;
            const long long b = s_lut[esim_y8(px, p.bgr)];
            if (b != a) {
                const bool up = b > a;
                const long long c = up ? cp : cn;
                const unsigned long long den = (unsigned long long)(up ? b - a : a - b);
                double t0 = 0.0, t1 = 0.0;
                if (EMIT) t0 = p.stamps[k], t1 = p.stamps[k + 1];
                while (up ? ref + c <= b : ref - c >= b) {
                    if (cnt == (unsigned)ESIM_CAP) {           // bad data: neither spins nor writes on
                        flag |= REFID_EVENT_SIM_FLAG_OVERFLOW;
                        break;
                    }
                    ref += up ? c : -c;
                    if (EMIT) {
                        const unsigned long long num = (unsigned long long)(up ? ref - a : a - ref);
                        const long long tick = (long long)(((num << 20) / den) & 0x1fffffull);
                        if (slot < slot_end) {
                            p.rows[slot] = make_float4(esim_stamp(t0, t1, tick), fx, fy, up ? 1.f : -1.f);
                            p.keys[slot] = ((long long)k << 54) | (tick << 33) | (pix << 8) | (long long)cnt;
                            ++slot;
                        } else {
                            flag |= REFID_EVENT_SIM_FLAG_SLOTS;    // the frames changed between the passes
                        }
                    }
                    ++cnt;
                }
                a = b;
            }
        }
        if (!EMIT) {
            const unsigned sum = refid_wave_sum(cnt);
            if ((tid & 63) == 0 && sum) atomicAdd(&s_rows[k], sum);
        }
        total += cnt;
    }
    if (on) {
        if (EMIT) {
            p.state[pix] = (int32_t)ref;
            if (slot != slot_end) flag |= REFID_EVENT_SIM_FLAG_SLOTS;
        } else {
            p.counts[pix] = (int32_t)total;
        }
    }
    if (flag) atomicOr(&p.totals[p.n_frames - 1], (unsigned long long)flag);
    if (!EMIT) {
        __syncthreads();
        for (int k = tid; k < p.n_frames - 1; k += ESIM_THREADS)
            if (s_rows[k]) atomicAdd(&p.totals[k], (unsigned long long)s_rows[k]);
    }
}

__global__ __launch_bounds__(ESIM_THREADS) void esim_reset_kernel(const uint8_t* __restrict__ frame, const int32_t* __restrict__ lut,
                                                                  int32_t* __restrict__ state, long long hw, int bgr) {
    const long long pix = (long long)blockIdx.x * ESIM_THREADS + threadIdx.x;
    if (pix < hw) state[pix] = lut[esim_y8(frame + pix * 3, bgr)];
}

__global__ __launch_bounds__(ESIM_THREADS) void esim_gather_kernel(const float4* __restrict__ rows, const long long* __restrict__ perm,
                                                                   float4* __restrict__ sorted, long long n) {
    const long long i = (long long)blockIdx.x * ESIM_THREADS + threadIdx.x;
    if (i >= n) return;
    const long long j = perm[i];
    if (j >= 0 && j < n) sorted[i] = rows[j];
}

bool esim_aligned(const void* p, unsigned long long to) { return ((unsigned long long)p & (to - 1ull)) == 0; }

}  // namespace

extern "C" int32_t refid_event_sim_min_threshold(int32_t lut_min, int32_t lut_max) {
    if (lut_max < lut_min) return 0;
    const long long c = ((long long)lut_max - (long long)lut_min) / ESIM_CAP + 1;      // the least c with span / c + 1 <= 255
    return c > 0x7fffffffll ? 0 : (int32_t)c;
}

extern "C" int refid_event_sim(const refid_event_sim_desc* d, void* stream) {
    REFID_CHECK(d, "event_sim: null descriptor");
    const int stage = d->stage;
    REFID_CHECK(stage == REFID_EVENT_SIM_RESET || stage == REFID_EVENT_SIM_COUNT || stage == REFID_EVENT_SIM_EMIT ||
                stage == REFID_EVENT_SIM_GATHER,
                "event_sim: stage %d is none of REFID_EVENT_SIM_RESET (1), _COUNT (2), _EMIT (4), _GATHER (8)", stage);
    hipStream_t st = (hipStream_t)stream;
    if (stage == REFID_EVENT_SIM_GATHER) {
        REFID_CHECK(d->n_rows >= 1 && d->n_rows < (1ll << 31), "event_sim: n_rows %lld is not 1 .. 2^31 - 1 (use a smaller chunk)",
                    (long long)d->n_rows);
        REFID_CHECK(d->rows && d->perm && d->sorted, "event_sim: %s is null", !d->rows ? "rows" : !d->perm ? "perm" : "sorted");
        REFID_CHECK(esim_aligned(d->rows, 16) && esim_aligned(d->sorted, 16) && esim_aligned(d->perm, 8),
                    "event_sim: %s is not aligned to %d bytes", !esim_aligned(d->rows, 16) ? "rows" : !esim_aligned(d->sorted, 16) ? "sorted" : "perm",
                    esim_aligned(d->rows, 16) && esim_aligned(d->sorted, 16) ? 8 : 16);
        const unsigned groups = (unsigned)((d->n_rows + ESIM_THREADS - 1) / ESIM_THREADS);
        hipLaunchKernelGGL(esim_gather_kernel, dim3(groups), dim3(ESIM_THREADS), 0, st, (const float4*)d->rows, (const long long*)d->perm,
                           (float4*)d->sorted, (long long)d->n_rows);
        REFID_LAUNCH_CHECK("event_sim (gather)");
        return 0;
    }
    REFID_CHECK(d->height >= 1 && d->width >= 1, "event_sim: height %d and width %d must be positive", d->height, d->width);
    const long long hw = (long long)d->height * d->width;
    REFID_CHECK(hw <= REFID_EVENT_SIM_MAX_PIXELS, "event_sim: height %d * width %d = %lld pixels exceed %lld, what the sort key holds", d->height,
                d->width, hw, (long long)REFID_EVENT_SIM_MAX_PIXELS);
    REFID_CHECK(d->frames && d->lut && d->state, "event_sim: %s is null", !d->frames ? "frames" : !d->lut ? "lut" : "state");
    REFID_CHECK(esim_aligned(d->lut, 4) && esim_aligned(d->state, 4), "event_sim: %s is not aligned to 4 bytes",
                !esim_aligned(d->lut, 4) ? "lut" : "state");
    const unsigned groups = (unsigned)((hw + ESIM_THREADS - 1) / ESIM_THREADS);
    if (stage == REFID_EVENT_SIM_RESET) {
        hipLaunchKernelGGL(esim_reset_kernel, dim3(groups), dim3(ESIM_THREADS), 0, st, d->frames, d->lut, d->state, hw, d->bgr ? 1 : 0);
        REFID_LAUNCH_CHECK("event_sim (reset)");
        return 0;
    }
    REFID_CHECK(d->n_frames >= 2, "event_sim: n_frames %d must be at least 2", d->n_frames);
    REFID_CHECK(d->n_frames <= ESIM_MAX_FRAMES, "event_sim: n_frames %d exceeds %d in one call, what the sort key holds (use a smaller chunk)",
                d->n_frames, ESIM_MAX_FRAMES);
    REFID_CHECK(d->stamps_host && d->stamps_dev && d->totals, "event_sim: %s is null",
                !d->stamps_host ? "stamps_host" : !d->stamps_dev ? "stamps_dev" : "totals");
    REFID_CHECK(esim_aligned(d->stamps_dev, 8) && esim_aligned(d->totals, 8), "event_sim: %s is not aligned to 8 bytes",
                !esim_aligned(d->stamps_dev, 8) ? "stamps_dev" : "totals");
    for (int k = 0; k < d->n_frames; ++k) {
        const double s = d->stamps_host[k];
        REFID_CHECK(s - s == 0.0, "event_sim: stamps[%d] is not finite", k);
        REFID_CHECK(k == 0 || s > d->stamps_host[k - 1], "event_sim: stamps are not strictly increasing: stamps[%d] = %.17g after stamps[%d] = %.17g", k,
                    s, k - 1, d->stamps_host[k - 1]);
    }
    REFID_CHECK(d->c_pos_map || d->c_pos >= 1, "event_sim: c_pos %d must be at least 1 (units of 2^-16)", d->c_pos);
    REFID_CHECK(d->c_neg_map || d->c_neg >= 1, "event_sim: c_neg %d must be at least 1 (units of 2^-16)", d->c_neg);
    REFID_CHECK(esim_aligned(d->c_pos_map, 4) && esim_aligned(d->c_neg_map, 4), "event_sim: %s is not aligned to 4 bytes",
                !esim_aligned(d->c_pos_map, 4) ? "c_pos_map" : "c_neg_map");
    long long c_min = 0x7fffffffll;
    if (!d->c_pos_map) c_min = d->c_pos;
    if (!d->c_neg_map && d->c_neg < c_min) c_min = d->c_neg;
    if (d->c_pos_map || d->c_neg_map) {
        REFID_CHECK(d->c_min >= 1, "event_sim: c_min %d, the smallest threshold of the maps, must be at least 1 (units of 2^-16)", d->c_min);
        if (d->c_min < c_min) c_min = d->c_min;
    }
    REFID_CHECK(d->lut_max >= d->lut_min, "event_sim: lut_max %d is below lut_min %d", d->lut_max, d->lut_min);
    const long long span = (long long)d->lut_max - (long long)d->lut_min;
    REFID_CHECK(span / c_min + 1 <= ESIM_CAP,
                "event_sim: the smallest threshold %lld allows %lld events per pixel and interval over the table's span %lld, the cap is %d: "
                "thresholds must be at least %lld (units of 2^-16)", c_min, span / c_min + 1, span, ESIM_CAP, span / ESIM_CAP + 1);
    EsimArgs a;
    a.frames = d->frames, a.stamps = d->stamps_dev, a.lut = d->lut, a.c_pos_map = d->c_pos_map, a.c_neg_map = d->c_neg_map;
    a.state = d->state, a.counts = d->counts, a.totals = (unsigned long long*)d->totals, a.ends = (const long long*)d->ends;
    a.rows = (float4*)d->rows, a.keys = (long long*)d->keys;
    a.hw = hw, a.n_rows = d->n_rows, a.n_frames = d->n_frames, a.width = d->width, a.bgr = d->bgr ? 1 : 0, a.c_pos = d->c_pos, a.c_neg = d->c_neg;
    if (stage == REFID_EVENT_SIM_COUNT) {
        REFID_CHECK(d->counts, "event_sim: counts is null");
        REFID_CHECK(esim_aligned(d->counts, 4), "event_sim: counts is not aligned to 4 bytes");
        hipLaunchKernelGGL(esim_walk<false>, dim3(groups), dim3(ESIM_THREADS), 0, st, a);
        REFID_LAUNCH_CHECK("event_sim (count)");
        return 0;
    }
    REFID_CHECK(d->n_rows >= 1 && d->n_rows < (1ll << 31), "event_sim: n_rows %lld is not 1 .. 2^31 - 1 (use a smaller chunk)", (long long)d->n_rows);
    REFID_CHECK(d->ends && d->rows && d->keys, "event_sim: %s is null", !d->ends ? "ends" : !d->rows ? "rows" : "keys");
    REFID_CHECK(esim_aligned(d->rows, 16), "event_sim: rows is not aligned to 16 bytes");
    REFID_CHECK(esim_aligned(d->ends, 8) && esim_aligned(d->keys, 8), "event_sim: %s is not aligned to 8 bytes", !esim_aligned(d->ends, 8) ? "ends" : "keys");
    hipLaunchKernelGGL(esim_walk<true>, dim3(groups), dim3(ESIM_THREADS), 0, st, a);
    REFID_LAUNCH_CHECK("event_sim (emit)");
    return 0;
}
