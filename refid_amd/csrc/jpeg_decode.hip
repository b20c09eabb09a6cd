// Baseline JPEG decode behind the host entropy stage (jpeg_entropy.h): quantised coefficients -> uint8 RGB frames.  The
// arithmetic is libjpeg's with its defaults and is stated in include/refid_hip.h and restated in tests/jpeg_decode_ref.py.
//
// Two launches that meet at the kernel boundary; no atomics, nothing spins, nothing is allocated.
//   jpeg_idct_kernel    one lane per 8x8 block.  The lane reads its 64 coefficients (128 contiguous bytes, eight 16-byte
//     loads) and its component's table, dequantises, runs both islow passes in registers and stores the clamped samples as
//     eight 8-byte rows into its component's plane in `work`.  A plane is padded to whole MCUs, so its pitch is a multiple
//     of 8 and every block lies inside it.
//   jpeg_colour_kernel  one lane per 4 output pixels of a row: a dword of Y, the chroma samples its pixels need (fancy
//     upsampling reads one neighbour on each side and, for 4:2:0, the row above or below: edges replicate inside the
//     CROPPED plane, the padding is never read as a neighbour), colour conversion, 12 bytes out.  A row whose first byte
//     is 4-aligned leaves as whole dwords, other rows and a row's last incomplete group byte by byte; only the frame's
//     bytes are written.
#include "common.h"
#include "jpeg_entropy.h"

namespace {

constexpr int JDEC_THREADS = 256;

struct JdecGeom {
    int n_frames, height, width, sampling, ncomp;
    int hs, vs;                                                // luma sampling factors (chroma is 1x1)
    int rows, cols;                                            // MCU rows and columns
    int pw[3], ph[3];                                          // padded plane sizes in samples
    long long blocks[3], total_blocks;                         // per frame
    long long plane_at[3], frame_bytes;                        // a plane's offset in a frame's scratch, a frame's scratch
};

bool jdec_geometry(long long height, long long width, long long sampling, JdecGeom* g) {
    if (height < 1 || height > 65535 || width < 1 || width > 65535) return false;
    if (sampling < REFID_JPEG_DEC_GREY || sampling > REFID_JPEG_DEC_420) return false;
    g->height = (int)height, g->width = (int)width, g->sampling = (int)sampling;
    g->ncomp = sampling == REFID_JPEG_DEC_GREY ? 1 : 3;
    g->hs = sampling >= REFID_JPEG_DEC_422 ? 2 : 1, g->vs = sampling == REFID_JPEG_DEC_420 ? 2 : 1;
    g->rows = (g->height + 8 * g->vs - 1) / (8 * g->vs), g->cols = (g->width + 8 * g->hs - 1) / (8 * g->hs);
    g->total_blocks = 0, g->frame_bytes = 0;
    for (int c = 0; c < 3; ++c) {
        const int h = c ? 1 : g->hs, v = c ? 1 : g->vs;
        const bool on = c < g->ncomp;
        g->pw[c] = on ? g->cols * h * 8 : 0, g->ph[c] = on ? g->rows * v * 8 : 0;
        g->blocks[c] = (long long)(g->pw[c] / 8) * (g->ph[c] / 8);
        g->plane_at[c] = g->frame_bytes;
        g->total_blocks += g->blocks[c];
        g->frame_bytes += g->blocks[c] * 64;
    }
    return true;
}

// libjpeg's jpeg_idct_islow on eight values, in 32-bit two's complement with wrap-around (unsigned: nothing is undefined).
// SHIFT 11 for the column pass, 18 for the row pass; the arithmetic shift is done on the signed reinterpretation.
template <int SHIFT>
__device__ __forceinline__ void jdec_idct8(const uint32_t* in, int* out) {
    uint32_t z2 = in[2], z3 = in[6];
    uint32_t z1 = (z2 + z3) * 4433u;
    uint32_t tmp2 = z1 - z3 * 15137u;
    uint32_t tmp3 = z1 + z2 * 6270u;
    uint32_t tmp0 = (in[0] + in[4]) << 13;
    uint32_t tmp1 = (in[0] - in[4]) << 13;
    const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7], tmp1 = in[5], tmp2 = in[3], tmp3 = in[1];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
    uint32_t z4 = tmp1 + tmp3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u, tmp1 *= 16819u, tmp2 *= 25172u, tmp3 *= 12299u;
    z1 *= 0u - 7373u, z2 *= 0u - 20995u, z3 *= 0u - 16069u, z4 *= 0u - 3196u;
    z3 += z5, z4 += z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    constexpr uint32_t half = 1u << (SHIFT - 1);
    out[0] = (int)(tmp10 + tmp3 + half) >> SHIFT, out[7] = (int)(tmp10 - tmp3 + half) >> SHIFT;
    out[1] = (int)(tmp11 + tmp2 + half) >> SHIFT, out[6] = (int)(tmp11 - tmp2 + half) >> SHIFT;
    out[2] = (int)(tmp12 + tmp1 + half) >> SHIFT, out[5] = (int)(tmp12 - tmp1 + half) >> SHIFT;
    out[3] = (int)(tmp13 + tmp0 + half) >> SHIFT, out[4] = (int)(tmp13 - tmp0 + half) >> SHIFT;
}

__device__ __forceinline__ unsigned jdec_clamp(int v) { return (unsigned)min(max(v, 0), 255); }

__global__ __launch_bounds__(JDEC_THREADS) void jpeg_idct_kernel(const int16_t* __restrict__ coefs, const uint16_t* __restrict__ quant,
                                                                 uint8_t* __restrict__ work, const JdecGeom g) {
    const long long i = (long long)blockIdx.x * JDEC_THREADS + threadIdx.x;    // the block among all frames' blocks
    if (i >= (long long)g.n_frames * g.total_blocks) return;
    const long long f = i / g.total_blocks;
    long long b = i - f * g.total_blocks;
    int c = 0;
    if (b >= g.blocks[0]) b -= g.blocks[0], c = 1;
    if (c == 1 && b >= g.blocks[1]) b -= g.blocks[1], c = 2;
    const int bw = g.pw[c] >> 3;                               // blocks per row of the plane
    const int by = (int)(b / bw), bx = (int)(b - (long long)by * bw);
    const uint4* src = reinterpret_cast<const uint4*>(coefs + i * 64);          // (coefs is 16-byte aligned, a block is 128 bytes)
    const uint16_t* q = quant + (f * g.ncomp + c) * 64;
    uint32_t x[64];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint4 v = src[k];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            x[8 * k + 2 * j] = (uint32_t)(int)(int16_t)(w[j] & 0xffffu) * (uint32_t)q[8 * k + 2 * j];
            x[8 * k + 2 * j + 1] = (uint32_t)(int)(int16_t)(w[j] >> 16) * (uint32_t)q[8 * k + 2 * j + 1];
        }
    }
    // columns, then rows
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        uint32_t col[8];
        int o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) col[k] = x[8 * k + u];
        jdec_idct8<11>(col, o);
#pragma unroll
        for (int k = 0; k < 8; ++k) x[8 * k + u] = (uint32_t)o[k];
    }
    uint8_t* plane = work + f * g.frame_bytes + g.plane_at[c];
    uint8_t* dst = plane + ((long long)by * 8) * g.pw[c] + bx * 8;              // (8-byte aligned: work is 16-byte aligned, pw a multiple of 8)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int o[8];
        jdec_idct8<18>(&x[8 * k], o);
        uint2 v;
        v.x = jdec_clamp(o[0] + 128) | (jdec_clamp(o[1] + 128) << 8) | (jdec_clamp(o[2] + 128) << 16) | (jdec_clamp(o[3] + 128) << 24);
        v.y = jdec_clamp(o[4] + 128) | (jdec_clamp(o[5] + 128) << 8) | (jdec_clamp(o[6] + 128) << 16) | (jdec_clamp(o[7] + 128) << 24);
        *reinterpret_cast<uint2*>(dst + (long long)k * g.pw[c]) = v;
    }
}

// The upsampled chroma sample of component plane `p` (pitch `pitch`, cropped to ch x cw) at output pixel (y, x)
__device__ __forceinline__ int jdec_chroma(const uint8_t* __restrict__ p, int pitch, int ch, int cw, int y, int x, int hs, int vs) {
    if (hs == 1) return p[(long long)y * pitch + x];
    const int i = x >> 1;
    if (cw <= 2) return p[(long long)(y >> (vs - 1)) * pitch + i];              // narrow planes are replicated
    if (vs == 1) {
        const uint8_t* s = p + (long long)y * pitch;
        if (x & 1) return i == cw - 1 ? s[i] : (3 * s[i] + s[i + 1] + 2) >> 2;
        return i == 0 ? s[0] : (3 * s[i] + s[i - 1] + 1) >> 2;
    }
    const int j = y >> 1;
    const uint8_t* near = p + (long long)j * pitch;
    const uint8_t* far = p + (long long)((y & 1) ? min(j + 1, ch - 1) : max(j - 1, 0)) * pitch;
    const int t = 3 * near[i] + far[i];
    if (x & 1) return i == cw - 1 ? (4 * t + 7) >> 4 : (3 * t + 3 * near[i + 1] + far[i + 1] + 7) >> 4;
    return i == 0 ? (4 * t + 8) >> 4 : (3 * t + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}

__global__ __launch_bounds__(JDEC_THREADS) void jpeg_colour_kernel(const uint8_t* __restrict__ work, uint8_t* __restrict__ frames, const JdecGeom g) {
    const int x0 = (blockIdx.x * JDEC_THREADS + threadIdx.x) * 4;
    const int y = blockIdx.y, f = blockIdx.z;
    if (x0 >= g.width) return;
    const uint8_t* planes = work + (long long)f * g.frame_bytes;
    const unsigned yy = *reinterpret_cast<const unsigned*>(planes + (long long)y * g.pw[0] + x0);    // (x0 + 3 < pw[0]: a multiple of 8)
    const int n = min(4, g.width - x0);
    const int ch = (g.height + g.vs - 1) / g.vs, cw = (g.width + g.hs - 1) / g.hs;
    uint8_t rgb[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int lum = (int)((yy >> (8 * k)) & 0xffu);
        int r = lum, gr = lum, b = lum;
        if (g.ncomp == 3 && k < n) {
            const int cb = jdec_chroma(planes + g.plane_at[1], g.pw[1], ch, cw, y, x0 + k, g.hs, g.vs) - 128;
            const int cr = jdec_chroma(planes + g.plane_at[2], g.pw[2], ch, cw, y, x0 + k, g.hs, g.vs) - 128;
            r = lum + ((91881 * cr + 32768) >> 16);
            b = lum + ((116130 * cb + 32768) >> 16);
            gr = lum + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
        }
        rgb[3 * k] = (uint8_t)jdec_clamp(r), rgb[3 * k + 1] = (uint8_t)jdec_clamp(gr), rgb[3 * k + 2] = (uint8_t)jdec_clamp(b);
    }
    uint8_t* row = frames + ((long long)f * g.height + y) * g.width * 3;
    uint8_t* o = row + (long long)x0 * 3;
    if (n == 4 && ((unsigned long long)row & 3ull) == 0) {     // (x0 * 3 is a multiple of 4)
        unsigned* o4 = reinterpret_cast<unsigned*>(o);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o4[k] = (unsigned)rgb[4 * k] | ((unsigned)rgb[4 * k + 1] << 8) | ((unsigned)rgb[4 * k + 2] << 16) | ((unsigned)rgb[4 * k + 3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < 3 * n) o[k] = rgb[k];
    }
}

thread_local char jdec_err[refid_jpeg::ERR_BYTES];

}  // namespace

extern "C" int refid_jpeg_probe(const uint8_t* file, size_t len, refid_jpeg_info* info) {
    if (refid_jpeg::probe(file, len, info, jdec_err) == 0) return 0;
    refid_set_error("%s", jdec_err);
    return 1;
}

extern "C" int refid_jpeg_entropy_decode(const uint8_t* file, size_t len, const refid_jpeg_info* expect, int16_t* coefs, uint16_t* quant) {
    if (refid_jpeg::entropy_decode(file, len, expect, coefs, quant, jdec_err) == 0) return 0;
    refid_set_error("%s", jdec_err);
    return 1;
}

extern "C" int32_t refid_jpeg_decode_blocks(int32_t height, int32_t width, int32_t sampling, int32_t* blocks) {
    JdecGeom g;
    if (!jdec_geometry(height, width, sampling, &g)) return 0;
    if (blocks)
        for (int c = 0; c < 3; ++c) blocks[c] = (int32_t)g.blocks[c];
    return (int32_t)g.total_blocks;                            // (<= 8192 * 8192 * 3 / 2 ... below 2^31)
}

extern "C" size_t refid_jpeg_decode_work_bytes(int32_t n_frames, int32_t height, int32_t width, int32_t sampling) {
    JdecGeom g;
    if (n_frames < 1 || n_frames > 65535 || !jdec_geometry(height, width, sampling, &g)) return 0;
    if (((long long)n_frames * g.total_blocks + JDEC_THREADS - 1) / JDEC_THREADS > 0x7fffffffll) return 0;
    return (size_t)n_frames * (size_t)g.frame_bytes;
}

extern "C" int refid_jpeg_decode(const refid_jpeg_decode_desc* d, void* stream) {
    REFID_CHECK(d, "jpeg_decode: null descriptor");
    REFID_CHECK(d->coefs && d->quant && d->frames && d->work, "jpeg_decode: %s is null",
                !d->coefs ? "coefs" : !d->quant ? "quant" : !d->frames ? "frames" : "work");
    REFID_CHECK(d->n_frames > 0, "jpeg_decode: n_frames %d must be positive", d->n_frames);
    REFID_CHECK(d->height >= 1 && d->height <= 65535, "jpeg_decode: height %d is not 1 .. 65535", d->height);
    REFID_CHECK(d->width >= 1 && d->width <= 65535, "jpeg_decode: width %d is not 1 .. 65535", d->width);
    REFID_CHECK(d->sampling >= REFID_JPEG_DEC_GREY && d->sampling <= REFID_JPEG_DEC_420,
                "jpeg_decode: sampling %d is none of REFID_JPEG_DEC_GREY (0), _444 (1), _422 (2), _420 (3)", d->sampling);
    REFID_CHECK(((unsigned long long)d->coefs & 15ull) == 0, "jpeg_decode: coefs is not aligned to 16 bytes");
    REFID_CHECK(((unsigned long long)d->quant & 1ull) == 0, "jpeg_decode: quant is not aligned to 2 bytes");
    REFID_CHECK(((unsigned long long)d->work & 15ull) == 0, "jpeg_decode: work is not aligned to 16 bytes");
    JdecGeom g;
    jdec_geometry(d->height, d->width, d->sampling, &g);
    g.n_frames = d->n_frames;
    const long long idct_groups = ((long long)d->n_frames * g.total_blocks + JDEC_THREADS - 1) / JDEC_THREADS;
    REFID_CHECK(d->n_frames <= 65535 && idct_groups <= 0x7fffffffll, "jpeg_decode: n_frames %d of %lld blocks exceed the grid (split the call)",
                d->n_frames, g.total_blocks);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)idct_groups), dim3(JDEC_THREADS), 0, st, d->coefs, d->quant, d->work, g);
    REFID_LAUNCH_CHECK("jpeg_decode (idct)");
    const unsigned strips = (unsigned)((d->width + 4 * JDEC_THREADS - 1) / (4 * JDEC_THREADS));
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3(strips, (unsigned)d->height, (unsigned)d->n_frames), dim3(JDEC_THREADS), 0, st,
                       (const uint8_t*)d->work, d->frames, g);
    REFID_LAUNCH_CHECK("jpeg_decode (colour)");
    return 0;
}
