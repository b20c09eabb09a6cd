// Weight packing: reference layouts (Conv2d OIHW, ConvTranspose2d IOHW) -> what the conv tiles read.  One record (PackEntry)
// describes one packing; ONE host builder (pack_entry_build) states every geometry check and fills it, ONE size function
// (pack_entry_size) gives its bytes, ONE device body (pack_entry_run) writes it -- from the batched launch (a table of records in
// device memory) and from the lone launch (one record by value) alike.  A new form is a plane writer, a row in the builder and
// a row in ops.py's table.
#include "conv_planes.h"
#include <cstring>

namespace {

// packed[cls][chunk][tap][row][k] = W[src index] or 0.
struct PackArgs {
    const float* w; float* dst; const float* oscale;   // oscale: optional per-output-channel factor
    int role, O, I, KH, KW, KC, rows, rowsPad, K, nchunks, ntaps, ncls;
    int bf16;                  // write __bf16 (RNE) instead of float
};

struct PackEntry {
    PackArgs p;
    int kind;                  // 0 tile layout (planes = 0: fp32, 1: bf16), 1 split bf16 planes (modes 0-2), 2 1x1 split planes,
                               // 3 Winograd x six (three bf16 planes), 4 out = a * b (vectors), 5 Winograd fp16 planes (planes = 2:
                               // three products, 1: one product), 6 split tile with two fp16 planes (modes 0-2).  Kinds 5 and 6
                               // keep a scale exponent in their header: the prepass writes it before the pack kernel reads it
    int planes, mode;
    int blk0, nblk;            // this entry's workgroups in the batched launch: [blk0, blk0 + nblk)
    long long total;           // elements; kinds 3 and 5: WEIGHTS (one thread writes all planes of a weight's 16 points)
};

// One point (i, j) of U = G g G^T, g(t) = tap t of the 3x3 kernel.  The ONE statement of the transform: its order of additions
// is what every Winograd packing (fp32, bf16 planes, fp16 planes) holds.
template <class TAPS>
__device__ __forceinline__ float wino_point(const TAPS& g, int i, int j) {
    const float G[4][3] = {{1.f, 0.f, 0.f}, {0.5f, 0.5f, 0.5f}, {0.5f, -0.5f, 0.5f}, {0.f, 0.f, 1.f}};
    float u = 0.f;
#pragma unroll
    for (int aa = 0; aa < 3; ++aa)
#pragma unroll
        for (int bb = 0; bb < 3; ++bb) u += G[i][aa] * G[j][bb] * g(aa * 3 + bb);
    return u;
}

__device__ __forceinline__ float pack_fetch(const PackArgs& p, int cls, int tap, int row, int k) {
    const int KK = p.KH * p.KW;
    switch (p.role) {
        case REFID_ROLE_FWD:            // rows = O, k = I ; W[o][i][tap]
            return p.w[((long long)row * p.I + k) * KK + tap] * (p.oscale ? p.oscale[row] : 1.f);
        case REFID_ROLE_DGRAD:          // rows = I, k = O ; flipped taps
            return p.w[((long long)k * p.I + row) * KK + (KK - 1 - tap)] * (p.oscale ? p.oscale[k] : 1.f);
        case REFID_ROLE_CONVT: {        // W is (I=Ci, O=Co, 2, 2); rows = (q, co), k = ci
            const int Co = p.O;
            const int qd = row / Co, co = row - qd * Co;
            return p.w[((long long)k * Co + co) * 4 + qd];
        }
        case REFID_ROLE_CONVT_DGRAD:    // rows = ci, k = co, tap = dy*2+dx
            return p.w[((long long)row * p.O + k) * 4 + tap];
        case REFID_ROLE_CONVT_DGRAD_PW: // rows = ci, k = (dy, dx, co): the patch GEMM of the pointwise tile
            return p.w[((long long)row * p.O + k % p.O) * 4 + k / p.O];
        case REFID_ROLE_WINO_FWD:       // U[xi=(i,j)] = sum_ab G[i][a] G[j][b] g[a][b]
        case REFID_ROLE_WINO_DGRAD: {
            const bool fwd = p.role == REFID_ROLE_WINO_FWD;
            const float* g = fwd ? p.w + ((long long)row * p.I + k) * 9 : p.w + ((long long)k * p.I + row) * 9;
            const float u = wino_point([&](int t) { return fwd ? g[t] : g[8 - t]; }, tap >> 2, tap & 3);   // dgrad: flipped taps
            return u * (p.oscale ? p.oscale[fwd ? row : k] : 1.f);
        }
        case REFID_ROLE_DOWN_DGRAD: {   // W (O,I,4,4); rows = i, k = o; class (py,px), tap (ta,tb)
            const int py = cls >> 1, px = cls & 1, ta = tap >> 1, tb = tap & 1;
            const int ky = (ta == 0) ? (py ? 2 : 1) : (py ? 0 : 3);
            const int kx = (tb == 0) ? (px ? 2 : 1) : (px ? 0 : 3);
            return p.w[((long long)k * p.I + row) * 16 + ky * 4 + kx];
        }
    }
    return 0.f;
}

// ---- the plane writers: the only per-form device code ---------------------------------------------------------------------------
// Plane `plane` of v in T (bf16 / fp16): h = rne(v), m = rne(v - h), l = rne(v - h - m).  Three bf16 planes sum to v exactly;
// the fp16 forms keep h and m of a value already scaled into fp16's range.
template <class T>
__device__ __forceinline__ T plane_of(float v, int plane) {
    const T h = (T)v;
    const float r1 = v - (float)h;
    const T m = (T)r1;
    const T l = (T)(r1 - (float)m);
    return plane == 0 ? h : (plane == 1 ? m : l);
}

// The fp16 forms (kinds 5, 6) live behind a 64-byte header (conv_planes.h) whose int at byte 0 is the packing's scale exponent
template <bool F16>
__device__ __forceinline__ int pack_scale_exp(const PackArgs& p) { return F16 ? *reinterpret_cast<const int*>(p.dst) : 0; }
template <class T, bool F16>
__device__ __forceinline__ T* pack_planes(const PackArgs& p) {
    return reinterpret_cast<T*>(reinterpret_cast<char*>(p.dst) + (F16 ? PACK_HEADER_BYTES : 0));
}

// (IDX: the element index type -- unsigned where the packing has < 2^31 elements: a 64-bit division by a run-time value costs
//  ~4x a 32-bit one, and the index decode is most of this kernel's instructions)
template <class IDX>
__device__ __forceinline__ void pack_elem(const PackArgs& p, IDX e) {
    IDX r = e;
    const int kk = r % p.KC; r /= p.KC;
    const int row = r % p.rowsPad; r /= p.rowsPad;
    const int tap = r % p.ntaps; r /= p.ntaps;
    const int chunk = r % p.nchunks;
    const int cls = r / p.nchunks;
    const int k = chunk * p.KC + kk;
    float v = 0.f;
    if (row < p.rows && k < p.K) v = pack_fetch(p, cls, tap, row, k);
    if (p.bf16) reinterpret_cast<__bf16*>(p.dst)[e] = (__bf16)v;
    else p.dst[e] = v;
}

// Planes for conv_split.hip (8-channel sub-chunks, `planes` numbers per weight):
//   mode 0 (3x3 s1):        [chunk8][plane][tap 0..9][rowsPad][8]            the tenth tap is zero (tap pairs fill K = 16)
//   mode 1 (4x4 s2 forward): [chunk8][sy][sx][plane][tap (ty,tx)][rowsPad][8]  = W[row][k][2ty+sy][2tx+sx]  (2x2 input blocks)
//   mode 2 (its dgrad):      [class][chunk8][plane][tap (ta,tb)][rowsPad][8]   (REFID_ROLE_DOWN_DGRAD's classes / taps)
// T = __bf16: up to three planes of v (refid_conv2d algo 4).  T = _Float16: two planes of v 2^eW behind the header, eW from the
// prepass (the three-fp16-product form, mfma_terms 19).
template <class T, class IDX>
__device__ __forceinline__ void pack_split_elem(const PackArgs& p, int planes, int mode, IDX e) {
    constexpr bool F16 = !__is_same(T, __bf16);
    const int ntp = mode == 0 ? p.ntaps + 1 : 4;
    const int nsub = mode == 1 ? 4 : 1;
    IDX r = e;
    const int k8 = r % 8; r /= 8;
    const int row = r % p.rowsPad; r /= p.rowsPad;
    const int tap = r % ntp; r /= ntp;
    const int plane = r % planes; r /= planes;
    const int sub = r % nsub; r /= nsub;
    const int chunk = r % p.nchunks;
    const int cls = r / p.nchunks;
    const int k = chunk * 8 + k8;
    float v = 0.f;
    if (row < p.rows && k < p.K) {
        if (mode == 0) { if (tap < p.ntaps) v = pack_fetch(p, 0, tap, row, k); }
        else if (mode == 1) v = pack_fetch(p, 0, (2 * (tap >> 1) + (sub >> 1)) * 4 + 2 * (tap & 1) + (sub & 1), row, k);
        else v = pack_fetch(p, cls, tap, row, k);
    }
    if (F16) v = ldexpf(v, pack_scale_exp<F16>(p));
    pack_planes<T, F16>(p)[e] = plane_of<T>(v, plane);
}

// 1x1 (conv_pw.hip, six products): [chunk16][plane][rowsPad][16]; the 16 channels of a row are stored as the two MFMA K
// halves of the pointwise tile's lanes: slot 8h + t = channel 4h + t (t < 4) or 8 + 4h + (t - 4)
template <class IDX>
__device__ __forceinline__ void pack_pw6_elem(const PackArgs& p, int planes, IDX e) {
    IDX r = e;
    const int slot = r % 16; r /= 16;
    const int row = r % p.rowsPad; r /= p.rowsPad;
    const int plane = r % planes;
    const int chunk = r / planes;
    const int h = slot >> 3, t = slot & 7;
    const int k = chunk * 16 + (t < 4 ? 4 * h + t : 8 + 4 * h + (t - 4));
    float v = 0.f;
    if (row < p.rows && k < p.K) v = pack_fetch(p, 0, 0, row, k);
    reinterpret_cast<__bf16*>(p.dst)[e] = plane_of<__bf16>(v, plane);
}

// Winograd-domain weights U = G g G^T as NPL planes of T for conv_wino6.hip: [chunk16][xi][plane][rowsPad][16].
//   T = __bf16, NPL = 3: three planes that sum to U exactly (six bf16 products).
//   T = _Float16: planes of U 2^eU behind the header.  fp16 keeps 11 significand bits, so h = rne16(v), l = rne16(v - h) carry 22
//   and  u v = uh vh + uh vl + ul vh + O(2^-22 |u v|)  needs three MFMAs and two planes (NPL = 2) where bf16 needs six and three;
//   NPL = 1 is the high plane alone (the one-product form).  The price is fp16's RANGE (2^-14 .. 2^16; the low plane of a value
//   below 2^-3 is subnormal): both operands travel multiplied by an exact power of two.  U's is per packing: 2^eU with
//   max |U| 2^eU in [2^12, 2^15) -- |U| <= 2.25 max |w| --, found by the prepass; the conv tile undoes it in its output transform.
// One thread per WEIGHT (chunk, row, k16): nine loads, the 16 transform points once, 16 NPL two-byte stores -- a wave's 64 threads
// (4 rows x 16 k) write 128 contiguous bytes per (xi, plane).  (The first form had one thread per OUTPUT element: 48 x the
// loads and transforms and five 64-bit divisions each -- 0.05 of HBM for the model's 238 MB of these planes.)
template <class T, int NPL>
__device__ __forceinline__ void pack_wino_weight(const PackArgs& p, unsigned f) {
    constexpr bool F16 = !__is_same(T, __bf16);
    const unsigned k16 = f & 15, r = f >> 4;
    const unsigned row = r % (unsigned)p.rowsPad, chunk = r / (unsigned)p.rowsPad;
    const int k = chunk * 16 + k16;
    const int eU = pack_scale_exp<F16>(p);
    float u[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) u[t] = 0.f;
    if ((int)row < p.rows && k < p.K) {
        const bool fwd = p.role == REFID_ROLE_WINO_FWD;
        const float* g = fwd ? p.w + ((long long)row * p.I + k) * 9 : p.w + ((long long)k * p.I + row) * 9;
        float gv[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) gv[t] = fwd ? g[t] : g[8 - t];              // dgrad: flipped taps
        const float sc = p.oscale ? p.oscale[fwd ? row : k] : 1.f;
#pragma unroll
        for (int xi = 0; xi < 16; ++xi) {
            const float v = wino_point([&](int t) { return gv[t]; }, xi >> 2, xi & 3) * sc;     // the fp32 U
            u[xi] = F16 ? ldexpf(v, eU) : v;                                   // exact: a power of two, inside the fp32 range
        }
    }
    const long long plane = (long long)p.rowsPad * 16;
    T* dst = pack_planes<T, F16>(p) + ((long long)chunk * (16 * NPL) * p.rowsPad + row) * 16 + k16;
#pragma unroll
    for (int xi = 0; xi < 16; ++xi)
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) dst[(xi * NPL + pl) * plane] = plane_of<T>(u[xi], pl);
}

// ---- the scale exponent of an fp16 packing: a reduction over the tensor (one workgroup, any size that is a multiple of 64;
// max is order independent => deterministic), written with the rest of the header
__device__ __forceinline__ int pack_scale_exp_of(float maxabs) {
    if (!(maxabs > 0.f)) return 0;
    const int ew = (int)(__float_as_uint(maxabs) >> 23) - 127;                 // max |w| < 2^(ew+1), max |U| < 2^(ew+2.17)
    const int e = 12 - ew;
    return e < -110 ? -110 : (e > 110 ? 110 : e);
}

__device__ __forceinline__ void pack_absmax_block(const PackArgs& p) {
    __shared__ float part[16];
    const long long total = (long long)p.O * p.I * p.KH * p.KW;
    const int per_o = p.I * p.KH * p.KW;
    float m = 0.f;
    if (p.oscale == nullptr && total % 4 == 0 && (reinterpret_cast<uintptr_t>(p.w) & 15) == 0) {
        const f32x4* w4 = reinterpret_cast<const f32x4*>(p.w);
        for (long long e = threadIdx.x; e < total / 4; e += blockDim.x) {
            const f32x4 v = w4[e];
            m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
        }
    } else {
        for (long long e = threadIdx.x; e < total; e += blockDim.x)
            m = fmaxf(m, fabsf(p.w[e] * (p.oscale ? p.oscale[e / per_o] : 1.f)));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < (int)(blockDim.x >> 6); ++k) m = fmaxf(m, part[k]);
        int* hdr = reinterpret_cast<int*>(p.dst);            // the whole header is defined: the exponent, then zeros
        hdr[0] = pack_scale_exp_of(m);
        for (int k = 1; k < PACK_HEADER_BYTES / 4; ++k) hdr[k] = 0;
    }
}

// ---- the device body: this thread's share of one record, elements e0, e0 + stride, ... ------------------------------------
template <class IDX>
__device__ __forceinline__ void pack_entry_elems(const PackEntry& en, IDX e0, IDX stride) {
    const PackArgs& p = en.p;
    for (IDX e = e0; e < (IDX)en.total; e += stride) {
        switch (en.kind) {
            case 0: pack_elem<IDX>(p, e); break;
            case 1: pack_split_elem<__bf16, IDX>(p, en.planes, en.mode, e); break;
            case 2: pack_pw6_elem<IDX>(p, en.planes, e); break;
            case 6: pack_split_elem<_Float16, IDX>(p, 2, en.mode, e); break;
            default: p.dst[e] = p.w[e] * p.oscale[e]; break;
        }
    }
}

__device__ __forceinline__ void pack_entry_run(const PackEntry& en, long long e0, long long stride) {
    const PackArgs& p = en.p;
    const unsigned total = (unsigned)en.total;               // (kinds 3, 5: weights, < 2^31 / 48 -- pack_entry_build)
    if (en.kind == 3) {
        for (unsigned f = (unsigned)e0; f < total; f += (unsigned)stride) pack_wino_weight<__bf16, 3>(p, f);
    } else if (en.kind == 5 && en.planes == 1) {
        for (unsigned f = (unsigned)e0; f < total; f += (unsigned)stride) pack_wino_weight<_Float16, 1>(p, f);
    } else if (en.kind == 5) {
        for (unsigned f = (unsigned)e0; f < total; f += (unsigned)stride) pack_wino_weight<_Float16, 2>(p, f);
    } else if (en.total < 0x7fffffffLL) {
        pack_entry_elems<unsigned>(en, (unsigned)e0, (unsigned)stride);
    } else {
        pack_entry_elems<long long>(en, e0, stride);
    }
}

// one record by value (the one-by-one entry points)
__global__ __launch_bounds__(256) void pack_lone_kernel(const PackEntry en) {
    pack_entry_run(en, blockIdx.x * 256ll + threadIdx.x, (long long)gridDim.x * 256);
}

// ---- all packings of a model in ONE launch (refid_pack_batch): the table lives in device memory, a workgroup finds its
// entry by binary search over the entries' first block.  ~220 dependent 6-20 us launches per optimiser step become one.
__global__ __launch_bounds__(256) void pack_batch_kernel(const PackEntry* __restrict__ table, int n) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {                                       // last entry with blk0 <= blockIdx.x
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].blk0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const PackEntry en = table[lo];
    pack_entry_run(en, (long long)(blockIdx.x - en.blk0) * 256 + threadIdx.x, (long long)en.nblk * 256);
}

__global__ __launch_bounds__(1024) void pack_absmax_kernel(const PackArgs p) { pack_absmax_block(p); }

// the scale exponents of every kind-5 / kind-6 record of a table (one workgroup per record; the others leave at once)
__global__ __launch_bounds__(1024) void pack_prepass_kernel(const PackEntry* __restrict__ table, int n) {
    const PackEntry& en = table[blockIdx.x];
    if (en.kind != 5 && en.kind != 6) return;
    const PackArgs p = en.p;
    pack_absmax_block(p);
}

// ---- host: one record builder, one size function ---------------------------------------------------------------------------------
// error paths of the builder return -1 (a positive value is a workgroup count), never REFID_CHECK's 1
#define REFID_FILL_CHECK(cond, ...)               \
    do {                                          \
        if (!(cond)) {                            \
            refid_set_error(__VA_ARGS__);         \
            return -1;                            \
        }                                         \
    } while (0)

int pack_geometry(int role, int o, int i, int kh, int kw, int kc, int bn, PackArgs* p) {
    p->role = role; p->O = o; p->I = i; p->KH = kh; p->KW = kw; p->KC = kc;
    p->ncls = 1;
    switch (role) {
        case REFID_ROLE_FWD: p->rows = o; p->K = i; p->ntaps = kh * kw; break;
        case REFID_ROLE_DGRAD: p->rows = i; p->K = o; p->ntaps = kh * kw; break;
        case REFID_ROLE_CONVT: p->rows = 4 * o; p->K = i; p->ntaps = 1; break;
        case REFID_ROLE_CONVT_DGRAD: p->rows = i; p->K = o; p->ntaps = 4; break;
        case REFID_ROLE_CONVT_DGRAD_PW: p->rows = i; p->K = 4 * o; p->ntaps = 1; break;
        case REFID_ROLE_DOWN_DGRAD: p->rows = i; p->K = o; p->ntaps = 4; p->ncls = 4; break;
        case REFID_ROLE_WINO_FWD: p->rows = o; p->K = i; p->ntaps = 16; break;
        case REFID_ROLE_WINO_DGRAD: p->rows = i; p->K = o; p->ntaps = 16; break;
        default: return 1;
    }
    p->rowsPad = round_up(p->rows, bn);
    p->nchunks = cdiv(p->K, kc);
    return 0;
}

int split_pack_mode(int role, int kh, int kw) {
    if ((role == REFID_ROLE_FWD || role == REFID_ROLE_DGRAD) && kh == 3 && kw == 3) return 0;
    if (role == REFID_ROLE_FWD && kh == 4 && kw == 4) return 1;
    if (role == REFID_ROLE_DOWN_DGRAD && kh == 4 && kw == 4) return 2;
    if ((role == REFID_ROLE_FWD || role == REFID_ROLE_DGRAD) && kh == 1 && kw == 1) return 3;
    return -1;
}

bool role_is_wino(int role) { return role == REFID_ROLE_WINO_FWD || role == REFID_ROLE_WINO_DGRAD; }
// (the engine scales conv-kind FWD / DGRAD / Winograd packings only)
bool role_takes_scale(int role) { return role == REFID_ROLE_FWD || role == REFID_ROLE_DGRAD || role_is_wino(role); }

// Every geometry condition of every packing, stated once: role / kernel-size pairs, plane counts, the split modes, the 32-bit
// ranges.  Fills the record's PackArgs (but for its pointers: pack_entry_bind), mode, total and workgroups; returns the
// workgroup count of the batched launch, -1 with a message otherwise.  (kc is the caller's for kind 0; the plane forms have their
// own: 8-channel sub-chunks for the split tile, 16 for the 1x1 and Winograd planes.)
int pack_entry_build(PackEntry& en, int kind, int planes, int role, int o, int i, int kh, int kw, int kc, int bn, int blk0) {
    memset(&en, 0, sizeof(en));
    REFID_FILL_CHECK(kind >= 0 && kind <= 6, "pack: unknown kind %d", kind);
    REFID_FILL_CHECK(blk0 >= 0, "pack: negative first block %d", blk0);
    REFID_FILL_CHECK(o > 0 && (kind == 4 || i > 0), "pack: empty packing (o=%d, i=%d)", o, i);
    en.kind = kind; en.planes = planes; en.blk0 = blk0;
    PackArgs& p = en.p;
    if (kind == 4) {                                        // out[e] = w[e] * oscale[e], e < o
        en.total = o;
    } else {
        const bool wino = role_is_wino(role), planes16 = kind == 3 || kind == 5, split = kind == 1 || kind == 2 || kind == 6;
        if (planes16) kc = 16;
        if (split) kc = 8;
        REFID_FILL_CHECK(kh > 0 && kw > 0 && kc > 0 && bn > 0, "pack: kernel %dx%d, kc %d, bn %d must be positive", kh, kw, kc, bn);
        REFID_FILL_CHECK(pack_geometry(role, o, i, kh, kw, kc, bn, &p) == 0, "pack: unknown role %d", role);
        const bool convt = role == REFID_ROLE_CONVT || role == REFID_ROLE_CONVT_DGRAD || role == REFID_ROLE_CONVT_DGRAD_PW;
        REFID_FILL_CHECK(!convt || (kh == 2 && kw == 2), "pack: convT roles need a 2x2 kernel");
        REFID_FILL_CHECK(role != REFID_ROLE_DOWN_DGRAD || (kh == 4 && kw == 4), "pack: down-dgrad needs a 4x4 kernel");
        REFID_FILL_CHECK(!wino || (kh == 3 && kw == 3), "pack: Winograd roles need a 3x3 kernel");
        REFID_FILL_CHECK(wino || !planes16, "pack: the Winograd plane forms take the Winograd roles only");
        p.bf16 = 1;
        if (kind == 0) {
            REFID_FILL_CHECK(planes == 0 || planes == 1, "pack: kind 0 takes planes = 0 (fp32) or 1 (bf16), got %d", planes);
            REFID_FILL_CHECK(!wino || (kc == 8 && planes == 0), "pack: the Winograd tile layout needs kc = 8 and fp32 output");
            p.bf16 = planes;
            en.total = (long long)p.ncls * p.nchunks * p.ntaps * p.rowsPad * p.KC;
        } else if (split) {
            const int mode = split_pack_mode(role, kh, kw);
            REFID_FILL_CHECK(mode >= 0 && (kind == 2) == (mode == 3),
                             "pack: split planes: FWD / DGRAD of a 3x3 kernel, FWD / DOWN_DGRAD of a 4x4 (stride 2) kernel; 1x1 (bf16 planes only) is kind 2");
            if (kind == 6) en.planes = planes = 2;
            REFID_FILL_CHECK(planes >= 1 && planes <= 3, "pack: split planes: 1, 2 or 3 planes (got %d)", planes);
            en.mode = mode;
            en.total = mode == 3 ? (long long)cdiv(p.K, 16) * planes * p.rowsPad * 16
                                 : (long long)p.ncls * p.nchunks * (mode == 1 ? 4 : 1) * planes * (mode == 0 ? p.ntaps + 1 : 4) * p.rowsPad * 8;
        } else {
            if (kind == 3) en.planes = planes = 3;
            REFID_FILL_CHECK(kind == 3 || planes == 1 || planes == 2, "pack: kind 5 takes planes = 2 (three fp16 products) or 1 (one), got %d", planes);
            en.total = (long long)p.nchunks * p.rowsPad * 16;
            // one thread per weight indexes its planes with 32 bits: the largest form of the kind must fit (bf16: 48 per weight;
            // fp16: 32, for both plane counts)
            REFID_FILL_CHECK(en.total * 16 * (kind == 3 ? 3 : 2) < 0x7fffffffLL, "pack: Winograd planes of %lld weights exceed the 32-bit index range", en.total);
        }
    }
    REFID_FILL_CHECK(en.total > 0, "pack: empty packing (o=%d, i=%d)", o, i);
    const long long nb = (en.total + 255) / 256;
    en.nblk = (int)(nb > 1024 ? 1024 : nb);
    return en.nblk;
}

// bytes of a built record's packing: elements x element size + header
size_t pack_entry_size(const PackEntry& en) {
    const size_t t = (size_t)en.total;
    switch (en.kind) {
        case 0: return t * (en.planes ? 2 : 4);
        case 1: case 2: return t * 2;
        case 3: return t * 16 * 3 * 2;
        case 5: return PACK_HEADER_BYTES + t * 16 * en.planes * 2;
        case 6: return PACK_HEADER_BYTES + t * 2;
        default: return t * 4;
    }
}

size_t pack_size(int kind, int planes, int role, int o, int i, int kh, int kw, int kc, int bn) {
    PackEntry en;
    return pack_entry_build(en, kind, planes, role, o, i, kh, kw, kc, bn, 0) < 0 ? 0 : pack_entry_size(en);
}

// the pointers of a built record: none null, the fp16 forms' header aligned, a scale only where the packing applies one
int pack_entry_bind(PackEntry& en, const float* w, const float* oscale, void* dst) {
    const int role = en.p.role;
    REFID_FILL_CHECK(w && dst, "pack: null pointer");
    if (en.kind == 4) REFID_FILL_CHECK(oscale != nullptr, "pack: the vector product needs both factors");
    else REFID_FILL_CHECK(oscale == nullptr || role_takes_scale(role), "pack: only FWD/DGRAD roles take a scale");
    REFID_FILL_CHECK((en.kind != 5 && en.kind != 6) || (reinterpret_cast<uintptr_t>(dst) & 15) == 0,
                     "pack: an fp16 packing (header + planes) must be 16-byte aligned");
    en.p.w = w; en.p.oscale = oscale; en.p.dst = reinterpret_cast<float*>(dst);
    return 0;
}

// the one-by-one entry points: a record, its prepass where it has a header, the lone kernel
int pack_lone(int kind, int planes, const float* w, const float* oscale, void* dst, int role, int o, int i, int kh, int kw, int kc,
              int bn, void* stream) {
    PackEntry en;
    if (pack_entry_build(en, kind, planes, role, o, i, kh, kw, kc, bn, 0) < 0 || pack_entry_bind(en, w, oscale, dst) < 0) return 1;
    if (kind == 5 || kind == 6) {
        hipLaunchKernelGGL(pack_absmax_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, en.p);
        REFID_LAUNCH_CHECK("pack_conv_weights/absmax");
    }
    hipLaunchKernelGGL(pack_lone_kernel, dim3(grid_for(en.total)), dim3(256), 0, (hipStream_t)stream, en);
    REFID_LAUNCH_CHECK("pack_conv_weights");
    return 0;
}

int split_kind(int kh, int kw) { return kh == 1 && kw == 1 ? 2 : 1; }

}  // namespace

extern "C" size_t refid_packed_weight_floats(int role, int o, int i, int kh, int kw, int kc, int bn) {
    return pack_size(0, 0, role, o, i, kh, kw, kc, bn) / 4;
}
extern "C" size_t refid_packed_weight_split_bytes(int role, int o, int i, int kh, int kw, int bn, int planes) {
    return pack_size(split_kind(kh, kw), planes, role, o, i, kh, kw, 8, bn);
}
extern "C" size_t refid_packed_weight_split_f16_bytes(int role, int o, int i, int kh, int kw, int bn) {
    return pack_size(6, 2, role, o, i, kh, kw, 8, bn);
}
extern "C" size_t refid_packed_weight_wino6_bytes(int role, int o, int i, int bn) { return pack_size(3, 3, role, o, i, 3, 3, 16, bn); }
extern "C" size_t refid_packed_weight_wino3h_bytes(int role, int o, int i, int bn) { return pack_size(5, 2, role, o, i, 3, 3, 16, bn); }
extern "C" size_t refid_packed_weight_wino1h_bytes(int role, int o, int i, int bn) { return pack_size(5, 1, role, o, i, 3, 3, 16, bn); }

extern "C" int refid_pack_conv_weights(const float* w, float* packed, int role, int o, int i, int kh, int kw, int kc, int bn,
                                       void* stream) {
    return pack_lone(0, 0, w, nullptr, packed, role, o, i, kh, kw, kc, bn, stream);
}
extern "C" int refid_pack_conv_weights_scaled(const float* w, const float* oscale, float* packed, int role, int o, int i, int kh,
                                              int kw, int kc, int bn, void* stream) {
    REFID_CHECK(role_takes_scale(role), "pack_scaled: only FWD/DGRAD roles take a scale");
    return pack_lone(0, 0, w, oscale, packed, role, o, i, kh, kw, kc, bn, stream);
}
// same layout with bf16 elements (kc = twice the fp32 tile's chunk); used by refid_conv2d algo 2
extern "C" int refid_pack_conv_weights_bf16(const float* w, const float* oscale, void* packed_bf16, int role, int o, int i, int kh,
                                            int kw, int kc, int bn, void* stream) {
    return pack_lone(0, 1, w, oscale, packed_bf16, role, o, i, kh, kw, kc, bn, stream);
}
extern "C" int refid_pack_conv_weights_split(const float* w, const float* oscale, void* packed, int role, int o, int i, int kh,
                                             int kw, int bn, int planes, void* stream) {
    return pack_lone(split_kind(kh, kw), planes, w, oscale, packed, role, o, i, kh, kw, 8, bn, stream);
}
extern "C" int refid_pack_conv_weights_split_f16(const float* w, const float* oscale, void* packed, int role, int o, int i, int kh,
                                                 int kw, int bn, void* stream) {
    return pack_lone(6, 2, w, oscale, packed, role, o, i, kh, kw, 8, bn, stream);
}
extern "C" int refid_pack_conv_weights_wino6(const float* w, const float* oscale, void* packed, int role, int o, int i, int bn,
                                             void* stream) {
    return pack_lone(3, 3, w, oscale, packed, role, o, i, 3, 3, 16, bn, stream);
}
extern "C" int refid_pack_conv_weights_wino3h(const float* w, const float* oscale, void* packed, int role, int o, int i, int bn,
                                              void* stream) {
    return pack_lone(5, 2, w, oscale, packed, role, o, i, 3, 3, 16, bn, stream);
}
extern "C" int refid_pack_conv_weights_wino1h(const float* w, const float* oscale, void* packed, int role, int o, int i, int bn,
                                              void* stream) {
    return pack_lone(5, 1, w, oscale, packed, role, o, i, 3, 3, 16, bn, stream);
}

// ---- batched packing ------------------------------------------------------------------------------------------------
extern "C" size_t refid_pack_entry_bytes(void) { return sizeof(PackEntry); }

extern "C" int refid_pack_entry_fill(void* entry_host, int kind, const float* w, const float* oscale, void* dst, int role, int o,
                                     int i, int kh, int kw, int kc, int bn, int planes, int blk0) {
    REFID_FILL_CHECK(entry_host != nullptr, "pack_entry_fill: null record");
    PackEntry en;
    if (pack_entry_build(en, kind, planes, role, o, i, kh, kw, kc, bn, blk0) < 0 || pack_entry_bind(en, w, oscale, dst) < 0) return -1;
    memcpy(entry_host, &en, sizeof(en));
    return en.nblk;
}

// Host-side check of a finished table (before it is copied to the device): kinds valid, first blocks strictly increasing from
// 0 with blk0[k+1] = blk0[k] + nblk[k] (the kernel's binary search relies on it).  Returns the total workgroup count, -1 on error.
extern "C" int refid_pack_table_check(const void* table_host, int n) {
    REFID_FILL_CHECK(table_host != nullptr && n > 0, "pack_table_check: empty table");
    const PackEntry* t = reinterpret_cast<const PackEntry*>(table_host);
    long long blk = 0;
    for (int k = 0; k < n; ++k) {
        REFID_FILL_CHECK(t[k].kind >= 0 && t[k].kind <= 6 && t[k].total > 0 && t[k].nblk >= 1,
                         "pack_table_check: record %d was never filled (kind %d, total %lld)", k, t[k].kind, t[k].total);
        REFID_FILL_CHECK(t[k].blk0 == blk, "pack_table_check: record %d starts at block %d, expected %lld", k, t[k].blk0, blk);
        blk += t[k].nblk;
    }
    REFID_FILL_CHECK(blk < 0x7fffffffLL, "pack_table_check: too many workgroups");
    return (int)blk;
}

// The scale exponents of the table's kind-5 / kind-6 records (max |w| per tensor): one launch, BEFORE refid_pack_batch on the
// same stream, whenever the table holds such records (a no-op for the others).
extern "C" int refid_pack_batch_prepass(const void* table_dev, int n, void* stream) {
    REFID_CHECK(table_dev != nullptr && n > 0, "pack_batch_prepass: empty table");
    hipLaunchKernelGGL(pack_prepass_kernel, dim3(n), dim3(1024), 0, (hipStream_t)stream,
                       reinterpret_cast<const PackEntry*>(table_dev), n);
    REFID_LAUNCH_CHECK("pack_batch_prepass");
    return 0;
}

extern "C" int refid_pack_batch(const void* table_dev, int n, int nblocks, void* stream) {
    REFID_CHECK(table_dev != nullptr && n > 0 && nblocks > 0, "pack_batch: empty table");
    hipLaunchKernelGGL(pack_batch_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const PackEntry*>(table_dev), n);
    REFID_LAUNCH_CHECK("pack_batch");
    return 0;
}
