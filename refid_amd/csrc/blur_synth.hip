// Blurry key frames from high-frame-rate frames: window k of the table averages `count` consecutive uint8 frames into one,
// byte by byte, by the integer formulas of include/refid_hip.h ("Blur synthesis"); tests/blur_ref.py restates them and the
// device is compared bit for bit.  Integers only, no atomics: every output byte has one writer.
//
//   plain      out = (sum_j f[first+j][b] + count/2) / count                        (GoPro's blur/)
//   response   v = (sum_j L[f[first+j][b]] + count/2) / count, out = #{c in 1..255 : thr[c] <= v},
//              thr[c] = (L[c-1] + L[c] + 1) >> 1                                    (GoPro's blur_gamma: linear light)
// L is strictly increasing (the entry checks it), so thr[c] <= L[c] < thr[c+1]: a window of identical frames, whose v is
// L[c] for every count ((count L[c] + count/2) / count = L[c]), returns that frame exactly.
//
// One launch for all K windows.  A frame of S = 3 H W bytes is cut into units of 16 bytes (the last one of a frame may be
// shorter); a lane owns one unit of one window: it reads the unit of each of the window's frames, BLUR_BATCH frames' loads
// issued before the first add, and writes 16 bytes.  A tile is 256 consecutive units of one window, a workgroup's wave
// instruction covers 1 KiB of contiguous bytes of one frame; workgroups walk the K * ceil(units / 256) tiles with a stride
// of the grid, which is capped at BLUR_GROUPS = 4096 workgroups (16 per CU of a 256-CU chip: two rounds of the 8 that are
// resident at once; a 1280x720 window alone has 675 tiles).
//   ALIGNED (frames, S and out all multiples of 16): one 16-byte load per frame and one 16-byte store per lane.
//   general: the same units at the same offsets, read and written with 16-byte copies the compiler is told nothing about the
//   alignment of, as png_filter.hip reads its windows; the short unit at the end of a frame goes byte by byte with every
//   index checked.  Both forms compute a byte from the same operands, so they give the same bytes.
// Plain mode keeps two 16-bit sums per register (64 * 255 < 2^16).  Response mode gathers L from LDS once per input byte
// (ds_read_b32 at a data-dependent address: bank conflicts are the rule) and finds the code by an 8-step binary search
// over thr in LDS.  The division by count is a multiplication: with l = ceil(log2 count), s = 31 + l and
// m = floor(2^s / count) + 1 <= 2^32, (x m) >> s = x / count for every x < 2^31 (Granlund and Montgomery 1994, theorem
// 4.2: 1 <= m count - 2^s <= 2^l); the sums stay below 64 * 2^24 + 32.  The 64 pairs (m, s) are built once per workgroup,
// by long division in integers, into LDS.  The window of a tile, tile / tiles_per_window with tile < 2^31, is found the same
// way with a pair the launcher computes, so the device code holds no division and no floating-point instruction at all
// (the compiler expands an integer division through a float reciprocal).
#include "common.h"

namespace {

constexpr int BLUR_THREADS = 256;
constexpr int BLUR_UNIT = 16;
constexpr int BLUR_BATCH = 4;                   // frames whose loads are in flight before the first add
constexpr int BLUR_GROUPS = 4096;               // the grid cap (see above)
constexpr int BLUR_MAX_COUNT = REFID_BLUR_MAX_COUNT;

struct BlurArgs {
    const uint8_t* frames;
    const int32_t* windows;
    const uint32_t* to_linear;
    uint8_t* out;
    long long frame_bytes;                      // S
    unsigned units, tiles_per_window, tiles;    // units of a frame, tiles of a window, tiles of the launch
    unsigned tpw_mul, tpw_shift;                // tile / tiles_per_window = (tile tpw_mul) >> tpw_shift, tile < 2^31
    int n_frames;
};

struct BlurUnit { unsigned w[4]; };             // 16 bytes of a frame, byte i = (w[i >> 2] >> 8 (i & 3)) & 255

template <bool ALIGNED>
__device__ __forceinline__ BlurUnit blur_load(const uint8_t* __restrict__ p, int nb) {
    BlurUnit v;
    if (ALIGNED) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        v.w[0] = q.x, v.w[1] = q.y, v.w[2] = q.z, v.w[3] = q.w;
    } else if (nb == BLUR_UNIT) {
        __builtin_memcpy(&v, p, BLUR_UNIT);
    } else {
        v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0u;
#pragma unroll
        for (int i = 0; i < BLUR_UNIT - 1; ++i)
            if (i < nb) v.w[i >> 2] |= (unsigned)p[i] << (8 * (i & 3));
    }
    return v;
}

template <bool ALIGNED>
__device__ __forceinline__ void blur_store(uint8_t* __restrict__ p, const BlurUnit& v, int nb) {
    if (ALIGNED) {
        *reinterpret_cast<uint4*>(p) = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
    } else if (nb == BLUR_UNIT) {
        __builtin_memcpy(p, &v, BLUR_UNIT);
    } else {
#pragma unroll
        for (int i = 0; i < BLUR_UNIT - 1; ++i)
            if (i < nb) p[i] = (uint8_t)(v.w[i >> 2] >> (8 * (i & 3)));
    }
}

// the sums of a unit: plain mode packs bytes 0 and 2 of word d into lo[d], bytes 1 and 3 into hi[d]; response mode has a
// word per byte
template <bool RESPONSE>
struct BlurAcc;
template <>
struct BlurAcc<false> {
    unsigned lo[4], hi[4];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int d = 0; d < 4; ++d) lo[d] = hi[d] = 0u;
    }
    __device__ __forceinline__ void add(const BlurUnit& v, const unsigned*) {
#pragma unroll
        for (int d = 0; d < 4; ++d) lo[d] += v.w[d] & 0x00ff00ffu, hi[d] += (v.w[d] >> 8) & 0x00ff00ffu;
    }
    __device__ __forceinline__ unsigned sum(int i) const {
        const unsigned pair = (i & 1) ? hi[i >> 2] : lo[i >> 2];
        return (i & 2) ? pair >> 16 : pair & 0xffffu;
    }
};
template <>
struct BlurAcc<true> {
    unsigned s[BLUR_UNIT];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < BLUR_UNIT; ++i) s[i] = 0u;
    }
    __device__ __forceinline__ void add(const BlurUnit& v, const unsigned* lin) {
#pragma unroll
        for (int i = 0; i < BLUR_UNIT; ++i) s[i] += lin[(v.w[i >> 2] >> (8 * (i & 3))) & 0xffu];
    }
    __device__ __forceinline__ unsigned sum(int i) const { return s[i]; }
};

template <bool ALIGNED, bool RESPONSE>
__global__ __launch_bounds__(BLUR_THREADS) void blur_synth_kernel(BlurArgs a) {
    __shared__ unsigned s_lin[256], s_thr[256];
    __shared__ unsigned s_mul[BLUR_MAX_COUNT + 1], s_shift[BLUR_MAX_COUNT + 1];
    const int tid = (int)threadIdx.x;
    if (RESPONSE) {
        const unsigned here = a.to_linear[tid];
        s_lin[tid] = here;
        s_thr[tid] = tid == 0 ? 0u : (a.to_linear[tid - 1] + here + 1u) >> 1;      // thr[0] = 0 <= every v
    }
    if (tid >= 1 && tid <= BLUR_MAX_COUNT) {
        const unsigned cnt = (unsigned)tid;
        int l = 0;
        while ((1u << l) < cnt) ++l;
        const int s = 31 + l;
        unsigned long long q = 0ull, rem = 0ull;                                  // q = floor(2^s / cnt), bit by bit
        for (int bit = s; bit >= 0; --bit) {
            rem = (rem << 1) | (bit == s ? 1ull : 0ull);
            if (rem >= cnt) rem -= cnt, q |= 1ull << bit;
        }
        s_mul[tid] = (unsigned)(q + 1ull);
        s_shift[tid] = (unsigned)s;
    }
    __syncthreads();

    const long long S = a.frame_bytes;
    for (unsigned tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {           // (no barrier inside: lanes may leave)
        const unsigned k = (unsigned)(((unsigned long long)tile * a.tpw_mul) >> a.tpw_shift);     // tile / tiles_per_window
        const unsigned u = (tile - k * a.tiles_per_window) * BLUR_THREADS + (unsigned)tid;
        const int first = a.windows[2 * k], count = a.windows[2 * k + 1];
        // the entry checked the host's copy of the table; a device copy that differs must not lead outside `frames`
        if (first < 0 || count < 1 || count > BLUR_MAX_COUNT || first > a.n_frames - count) continue;
        if (u >= a.units) continue;
        const long long off = (long long)u * BLUR_UNIT;
        const int nb = ALIGNED ? BLUR_UNIT : (int)(S - off < BLUR_UNIT ? S - off : BLUR_UNIT);
        const uint8_t* __restrict__ src = a.frames + (long long)first * S + off;

        BlurAcc<RESPONSE> acc;
        acc.clear();
        for (int j = 0; j < count; j += BLUR_BATCH) {
            BlurUnit v[BLUR_BATCH];
#pragma unroll
            for (int b = 0; b < BLUR_BATCH; ++b)
                if (j + b < count) v[b] = blur_load<ALIGNED>(src + (long long)(j + b) * S, nb);
#pragma unroll
            for (int b = 0; b < BLUR_BATCH; ++b)
                if (j + b < count) acc.add(v[b], s_lin);
        }

        const unsigned half = (unsigned)count >> 1, mul = s_mul[count], shift = s_shift[count];
        BlurUnit r;
        r.w[0] = r.w[1] = r.w[2] = r.w[3] = 0u;
#pragma unroll
        for (int i = 0; i < BLUR_UNIT; ++i) {
            const unsigned x = acc.sum(i) + half;
            unsigned code = (unsigned)(((unsigned long long)x * mul) >> shift);       // x / count
            if (RESPONSE) {
                const unsigned v = code;
                code = 0u;
#pragma unroll
                for (unsigned bit = 128u; bit; bit >>= 1)
                    if (s_thr[code | bit] <= v) code |= bit;                         // the largest c with thr[c] <= v
            }
            r.w[i >> 2] |= code << (8 * (i & 3));
        }
        blur_store<ALIGNED>(a.out + (long long)k * S + off, r, nb);
    }
}

bool blur_aligned(const void* p, unsigned long long to) { return ((unsigned long long)p & (to - 1ull)) == 0; }

}  // namespace

extern "C" int refid_blur_synth(const refid_blur_synth_desc* d, void* stream) {
    REFID_CHECK(d, "blur_synth: null descriptor");
    REFID_CHECK(d->n_windows >= 1, "blur_synth: n_windows %d must be at least 1", d->n_windows);
    REFID_CHECK(d->height >= 1 && d->width >= 1, "blur_synth: height %d and width %d must be positive", d->height, d->width);
    REFID_CHECK((long long)d->height * d->width <= (1ll << 40), "blur_synth: height %d * width %d exceed 2^40 pixels", d->height, d->width);
    REFID_CHECK(d->n_frames >= 1, "blur_synth: n_frames %d must be at least 1", d->n_frames);
    REFID_CHECK(d->max_groups >= 0, "blur_synth: max_groups %d must not be negative (0: the default cap of %d workgroups)", d->max_groups,
                BLUR_GROUPS);
    REFID_CHECK(d->frames && d->out && d->windows_host && d->windows, "blur_synth: %s is null",
                !d->frames ? "frames" : !d->out ? "out" : !d->windows_host ? "windows_host" : "windows");
    REFID_CHECK(blur_aligned(d->windows_host, 4) && blur_aligned(d->windows, 4), "blur_synth: %s is not aligned to 4 bytes",
                !blur_aligned(d->windows_host, 4) ? "windows_host" : "windows");
    REFID_CHECK((d->to_linear_host != nullptr) == (d->to_linear != nullptr), "blur_synth: %s is null but %s is not (pass both copies of the table, or neither)",
                !d->to_linear_host ? "to_linear_host" : "to_linear", !d->to_linear_host ? "to_linear" : "to_linear_host");
    REFID_CHECK(blur_aligned(d->to_linear_host, 4) && blur_aligned(d->to_linear, 4), "blur_synth: %s is not aligned to 4 bytes",
                !blur_aligned(d->to_linear_host, 4) ? "to_linear_host" : "to_linear");
    for (int k = 0; k < d->n_windows; ++k) {
        const long long first = d->windows_host[2 * k], count = d->windows_host[2 * k + 1];
        REFID_CHECK(count >= 1 && count <= BLUR_MAX_COUNT, "blur_synth: windows[%d]: count %lld is not 1 .. %d", k, count, BLUR_MAX_COUNT);
        REFID_CHECK(first >= 0 && first + count <= d->n_frames, "blur_synth: windows[%d]: frames %lld .. %lld lie outside the n_frames %d", k, first,
                    first + count - 1, d->n_frames);
    }
    if (d->to_linear_host) {
        const uint32_t* L = d->to_linear_host;
        for (int c = 1; c < 256; ++c)
            REFID_CHECK(L[c] > L[c - 1], "blur_synth: to_linear is not strictly increasing: to_linear[%d] = %u after to_linear[%d] = %u", c, L[c],
                        c - 1, L[c - 1]);
        REFID_CHECK(L[255] <= (1u << 24), "blur_synth: to_linear[255] = %u exceeds 2^24 = 16777216 (a sum of %d entries must stay below 2^31)", L[255],
                    BLUR_MAX_COUNT);
    }
    const long long S = 3ll * d->height * d->width;
    const long long units = (S + BLUR_UNIT - 1) / BLUR_UNIT;
    const long long tiles_per_window = (units + BLUR_THREADS - 1) / BLUR_THREADS;
    const long long tiles = tiles_per_window * d->n_windows;
    REFID_CHECK(tiles < (1ll << 31), "blur_synth: n_windows %d of height %d * width %d make %lld tiles, 2^31 - 1 are the most of one call", d->n_windows,
                d->height, d->width, tiles);
    BlurArgs a;
    a.frames = d->frames, a.windows = d->windows, a.to_linear = d->to_linear, a.out = d->out;
    a.frame_bytes = S, a.units = (unsigned)units, a.tiles_per_window = (unsigned)tiles_per_window, a.tiles = (unsigned)tiles;
    a.n_frames = d->n_frames;
    int l = 0;                                                  // the same multiplier as the kernel's for count (see the top)
    while ((1ll << l) < tiles_per_window) ++l;
    a.tpw_shift = (unsigned)(31 + l), a.tpw_mul = (unsigned)((1ull << (31 + l)) / (unsigned long long)tiles_per_window + 1ull);
    const long long cap = d->max_groups ? d->max_groups : BLUR_GROUPS;
    const unsigned groups = (unsigned)(tiles < cap ? tiles : cap);
    const bool aligned = blur_aligned(d->frames, BLUR_UNIT) && blur_aligned(d->out, BLUR_UNIT) && S % BLUR_UNIT == 0;
    hipStream_t st = (hipStream_t)stream;
    if (d->to_linear) {
        if (aligned) hipLaunchKernelGGL((blur_synth_kernel<true, true>), dim3(groups), dim3(BLUR_THREADS), 0, st, a);
        else hipLaunchKernelGGL((blur_synth_kernel<false, true>), dim3(groups), dim3(BLUR_THREADS), 0, st, a);
    } else {
        if (aligned) hipLaunchKernelGGL((blur_synth_kernel<true, false>), dim3(groups), dim3(BLUR_THREADS), 0, st, a);
        else hipLaunchKernelGGL((blur_synth_kernel<false, false>), dim3(groups), dim3(BLUR_THREADS), 0, st, a);
    }
    REFID_LAUNCH_CHECK("blur_synth");
    return 0;
}
