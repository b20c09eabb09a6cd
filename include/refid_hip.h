/*
 * refid_hip.h -- C ABI of the MI355X-native REFID hot path (librefid_hip.so).
 *
 * The reference (AHupuJR/REFID) is pure Python/PyTorch and has no FFI of its own:
 * every arithmetic op on its hot path is a torch.nn call that lands in cuDNN/ATen
 * ("Native / CUDA kernel inventory: empty").  The entry points
 * below are therefore the operator-level boundary a maintainer would bind instead of
 * those torch.nn calls; each one cites the reference call site(s) it replaces
 * (paths relative to /root/reference/basicsr/models/archs unless noted).
 *
 * Conventions
 *  - plain C: raw DEVICE pointers, ints, floats; no torch types.
 *  - activations are NHWC fp32 ("pixel-major": channel is the fastest axis), every
 *    tensor is described by a base pointer and a pixel pitch `ld` (floats) so channel
 *    slices of wider buffers can be addressed; base pointers and pitches are multiples
 *    of 4 floats (16 B).
 *  - every function is asynchronous on the caller's `stream` (a hipStream_t passed as
 *    void*), allocates nothing, never synchronises, keeps no global mutable state and is
 *    re-entrant: scratch memory is always the CALLER's (refid_conv_workspace_bytes,
 *    refid_wgrad_workspace_bytes), so launches on different streams use different buffers.
 *  - return value: 0 = ok, non-zero = error; refid_last_error() returns a thread-local
 *    message for the last failing call on this thread.
 */
#ifndef REFID_HIP_H
#define REFID_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define REFID_ABI_VERSION 9     /* 9: refid_conv_desc.algo 5 with mfma_terms 3 (Winograd x three fp16 products) / algo 4 with mfma_terms 19 (conv_down on three fp16 products), refid_pack_conv_weights_wino3h / _split_f16, pack-table kinds 5 / 6 + refid_pack_batch_prepass; 8: refid_wgrad_desc.phase 4 + refid_wgrad_finish_flush (batched slab reductions), refid_*_tb layout conversions, REFID_ROLE_CONVT_DGRAD_PW, refid_wgrad_desc.algo 8, refid_rows_sum_defer / _flush; 7: refid_wgrad_desc.algo 5 (2x4 Winograd tiles) / 6; thin-output 3x3 weight gradient */

const char* refid_last_error(void);
int refid_abi_version(void);
/* Always 0 since ABI 9: the tiles that were measured and lost (the persistent and the wide Winograd tiles, the six-product /
 * LDS-DMA / F(3x3,4x4) weight gradients; REFID_EXPERIMENTAL_TILES=1 builds of ABI <= 8) are no longer in the tree.  Kept so that
 * callers written against earlier versions still link. */
int refid_experimental_tiles(void);

/* Device facts used by the host-side scheduler (CU count etc.); -1 on failure. */
int refid_device_cu_count(void);

/* ------------------------------------------------------------------------------------
 * Fused convolution tile:   out = mask( post( pre(conv(src) + bias) + res ) )
 *
 *   src   = in_a                    (c_b == 0)
 *         = [in_a | in_b]           channel concatenation WITHOUT materialising the cat
 *   pre   = LeakyReLU(slope_pre)    (1.0 = identity, 0.0 = ReLU)
 *   post  = LeakyReLU(slope_post)   applied after the residual add
 *   mask  = multiply by (mask_src > 0 ? 1 : slope_mask)   (activation derivative, backward)
 *
 * Replaces (forward): nn.Conv2d + LeakyReLU/ReLU + residual adds + torch.cat at
 *   recurrent_sub_modules.py:41-49 (ImageEncoderConvBlock), :74-84 (ConvLayer),
 *   :270-296 (EvR level: conv, cat+fuse_two_dir, down), :386-408 (decoder: ConvTranspose2d,
 *   cat), :488-503 (ResidualBlock), :659-678 + :719-726 + :755-758 (EvR hidden-state
 *   update trunk), fusion_modules.py:300-331 (the 1x1 convs of EGACA),
 *   XXNet_final_attenfusion_arch.py:147-149,215 (heads, pred).
 * Replaces (backward): the autograd conv-backward "input gradient" of the same calls
 *   (SURVEY.md Appendix A.2): dgrad is the same tile run on the transposed/flipped
 *   packed weights (refid_pack_conv_weights with role=REFID_ROLE_DGRAD).
 *
 * mode 0: ordinary conv, kh x kw, stride 1 or 2, zero padding `pad`.
 * mode 1: ConvTranspose2d(k=2,s=2) forward as a 1x1 GEMM with 4*Co columns and a
 *         pixel-shuffle store (column j -> (dy,dx)=(j/Co/2, j/Co%2), channel j%Co);
 *         `cout` is 4*Co, (h,w) the INPUT size, output is (2h,2w).
 * mode 2: input-gradient of conv4x4/stride2/pad1 (`conv_down`): four output-parity
 *         classes, each a 2x2-tap conv over the (h,w) gradient, stored at (2y+py,2x+px).
 * ---------------------------------------------------------------------------------- */
/* Fusions around a POINTWISE conv (algo 3, more than 32 output channels) -- the non-GEMM steps of EGACA
 * (fusion_modules.py:290-333) folded into its 1x1 convs; every member is optional (NULL / 0 = off):
 *   ln_*   LayerNorm2d PROLOGUE (fm:97-108,300,302,323-325): the operand is normalised over its (<= 64, one source)
 *          channels -- mean / biased variance, eps inside the root, times ln_gamma plus ln_beta -- before the GEMM;
 *          ln_out (pitch ld_ln_out) receives the normalised tensor (the training stash conv's weight gradient needs).
 *   se_*   SQUEEZE-EXCITE in the kernel (fm:253-260,309-315): `pool` holds the per-workgroup partial sums of the
 *          depthwise kernel, (n, pool_parts, se_c); every workgroup derives its sample's
 *          s = sigmoid(W2 relu(W1 mean + b1) + b2) and multiplies operand channel k by s[k mod se_c] as it is loaded
 *          ([xi*s | xe*s] is never materialised; xs_out optionally receives it for conv3's weight gradient);
 *          se_m / se_z1 / se_s (n,se_c) / (n,se_c/2) / (n,se_c) optionally receive the vectors SE's backward needs.
 *          hw = pixels per sample, must be a multiple of 128.
 *   res2   second residual tensor added with `res` (y = ev + img + beta*conv3(.), fm:319).
 *   out2   receives GELU_erf(out) (fm:327-329); `out` keeps the pre-activation for the backward pass. */
typedef struct refid_pw_extras {
    const float* ln_gamma; const float* ln_beta; float ln_eps; float* ln_out; int ld_ln_out;
    const float* pool; int pool_parts; float inv_hw; int hw; int se_c;
    const float* se_w1; const float* se_b1; const float* se_w2; const float* se_b2;
    float* se_m; float* se_z1; float* se_s;
    float* xs_out; int ld_xs_out;
    const float* res2; int ld_res2;
    float* out2; int ld_out2;
} refid_pw_extras;

typedef struct refid_conv_desc {
    const float* in_a;  const float* in_b;      /* NHWC sources                         */
    int ld_a, ld_b;                             /* pixel pitch (floats)                 */
    int c_a, c_b;                               /* channels taken from each source      */
    const float* w_packed;                      /* see refid_pack_conv_weights          */
    const float* bias;                          /* [cout] or NULL                       */
    float* out;          int ld_out;
    const float* res;    int ld_res;            /* NULL = none                          */
    const float* mask;   int ld_mask;           /* NULL = none                          */
    int n, h, w;                                /* input batch / height / width         */
    int ho, wo;                                 /* GEMM pixel grid (output h,w; mode 1/2: = h,w) */
    int cout;                                   /* GEMM columns computed by this call   */
    int cout_pad;                               /* rows per tap in w_packed             */
    int co_base;                                /* first row of w_packed / bias used    */
    int kh, kw, stride, pad;
    int mode;
    float slope_pre, slope_post, slope_mask;
    int algo;                                   /* 0 = direct implicit GEMM; 1 = Winograd F(2x2,3x3)
                                                   (3x3, stride 1, mode 0 only; w_packed must come
                                                   from the REFID_ROLE_WINO_* packings);
                                                   3 = register-operand pointwise tile (1x1, stride 1,
                                                   mode 0; w_packed = REFID_ROLE_FWD/DGRAD packing with
                                                   kc = 8) -- and mode 1, ConvTranspose2d(2,2) as the 1x1
                                                   GEMM over its 4 Co columns with a pixel-shuffle store
                                                   (REFID_ROLE_CONVT packing, kc = 8, bn = 32; bias / res /
                                                   slopes only; Co a multiple of 4, 4 Co > 32) -- and the 2x2
                                                   stride-2 conv (ConvTranspose2d's input gradient: non-
                                                   overlapping patches) as one GEMM with K = 4 c_a: a pixel's
                                                   patch is two contiguous runs of 2 c_a floats (dense pixels:
                                                   ld_a == c_a, one source; REFID_ROLE_CONVT_DGRAD_PW packing;
                                                   out2 / add2 supported);
                                                   2 = direct tile with bf16 MFMA operands (fp32
                                                   accumulate/epilogue/tensors; w_packed from
                                                   refid_pack_conv_weights_bf16 with kc doubled);
                                                   4 = direct 3x3 / stride-1 tile with SPLIT fp32 operands on
                                                   the bf16 matrix cores (mode 0; w_packed from
                                                   refid_pack_conv_weights_split with the same number of
                                                   planes): every fp32 operand is the exact sum of three bf16
                                                   numbers, six bf16 MFMAs give the fp32 product to one
                                                   rounding (see `mfma_terms`);
                                                   5 = Winograd F(2x2,3x3) with the transform-domain products on the bf16
                                                   matrix cores, six bf16 MFMAs per fp32 product on exactly split
                                                   operands (3x3, stride 1, mode 0; a 64-channel workgroup tile above 32 output
                                                   channels, a 32-channel one up to 32, thin outputs included --, two
                                                   sources: c_a a multiple of 16; w_packed from
                                                   refid_pack_conv_weights_wino6): the fp32 Winograd tile's result to
                                                   fp32 rounding at 2.67x fewer matrix-pipe cycles -- or, with
                                                   mfma_terms = 3, THREE fp16 products on two-plane operands (22 bits;
                                                   w_packed from refid_pack_conv_weights_wino3h): half the MFMAs again -- or, with
                                                   mfma_terms = 1, ONE fp16 product on one-plane operands (11 bits: a reduced-
                                                   precision form; w_packed from refid_pack_conv_weights_wino1h): a third of
                                                   those MFMAs, half the weight bytes  */
    int split_k;                                /* small problems (few output tiles, long K): split K over the grid into
                                                   `ws` partial sums + a finishing pass.  0 = never; 1 = decided by the
                                                   per-sample geometry (a sample's bits do not depend on the batch
                                                   size); 2 = decided by the total grid size (best at 1-2 samples per
                                                   GPU).  Used by algo 1 / 5 and by algo 0's 4x4/s2 tiles (mode 0 and 2).  */
    int wino_tile;                              /* algo 5: 0 = the library chooses between the 64- and the 32-output-channel
                                                   workgroup tile; 1 = the 64-channel tile wherever cout > 32; 4 = the
                                                   32-channel tile everywhere (an A/B switch: measured 9-35 % slower on the
                                                   64-channel layers); 5 = the library's choice of tile as under 0, but a
                                                   plan of exactly two K ranges (split_k) runs as two launch rows + the
                                                   finishing pass through `ws` instead of as the two four-wave groups of one
                                                   512-thread workgroup per tile (the routing before that form existed: an
                                                   A/B switch).  Same results whichever runs.  (2 / 3 selected tiles
                                                   that were removed with ABI 9 -- a persistent and a wide one, both measured
                                                   slower -- and are ignored.)                                          */
    const refid_pw_extras* pw;                  /* algo 3 only: fusions around the pointwise conv, or NULL               */
    int mfma_terms;                             /* algo 3: 0 = fp32 MFMA products; 6 = six bf16 products on exactly split
                                                   operands (w_packed from refid_pack_conv_weights_split with kh = kw = 1,
                                                   three planes; channel counts multiples of 16, more than 32 outputs).
                                                   algo 4: 0 / 6 = three bf16 planes per operand, six products
                                                   (error <= 2^-23 per product: fp32 class, closer to the fp64 result
                                                   than the fp32 Winograd tile); 3 = two planes, three products
                                                   (2^-16 per product: explicit opt-in, still finer than TF32); 19 (16 + 3;
                                                   4x4 stride 2 forward / input gradient only) = three fp16 products on
                                                   two-plane operands scaled by exact powers of two (w_packed from
                                                   refid_pack_conv_weights_split_f16): ~2^-22 per product, the fp32 class
                                                   at half of 6's MFMAs.
                                                   algo 5: 0 / 6 = six bf16 products on three-plane operands; 3 = three
                                                   fp16 products on two-plane operands h = rne16(v), l = rne16(v - h)
                                                   (~2^-22 per product, below the fp32 accumulation's own error at
                                                   K >= 144; both operands travel scaled by exact powers of two -- U per
                                                   packing, V per Winograd tile and online along K -- so any finite fp32
                                                   magnitude keeps the same relative error)                         */
    float* ws;  size_t ws_bytes;                /* caller's scratch, >= refid_conv_workspace_bytes(d) bytes, 16-byte
                                                   aligned, private to this stream until the call's work has run;
                                                   NULL: never split                                            */
    const float* add2; int ld_add2;             /* second output (algo 0 / 1 / 2 / 4 / 5; NULL = off): out2 = out + add2, same shape */
    float* out2;       int ld_out2;             /* as `out` -- the skip sum the reference forms right after this conv
                                                   (XXNet_final_attenfusion_arch.py:16-17,199-203,211) or, in BPTT, the sum of
                                                   this input gradient with another branch's, written by the producing tile
                                                   instead of a separate add kernel.  `out` is still written.            */
    int mask_mode;                              /* 0: the activation-derivative mask above.  1 (algo 3 only): multiply by
                                                   GELU_erf'(mask) instead -- the input gradient of conv5 leaves the tile as
                                                   the gradient of conv4's output (fusion_modules.py:327-329 backward)   */
} refid_conv_desc;

/* Scratch bytes refid_conv2d(d) wants in d->ws (0 = none); depends on the geometry fields and split_k only. */
size_t refid_conv_workspace_bytes(const refid_conv_desc* d);
int refid_conv2d(const refid_conv_desc* d, void* stream);

/* Channel-chunk width (KC) and row padding (BN) the conv tile for this geometry wants
 * its packed weights in. */
int refid_conv_kc(int kh, int kw, int stride, int mode);
/* "Cfg<...>" template signature of the tile refid_conv2d launches for this geometry (matches the
 * kernel name rocprofv3 reports); used by bench.py to attribute time to the dominant kernel. */
const char* refid_conv_tile_name(int kh, int kw, int stride, int mode, int cout);
int refid_conv_bn(int kh, int kw, int stride, int mode, int cout);

/* ------------------------------------------------------------------------------------
 * Weight gradient + bias gradient of the same convolutions (autograd's conv-backward
 * "weight gradient"):
 *   dW[o][i][ky][kx] (+)= sum_{n,y,x} g[n,y,x,o] * src[n, y*s+ky-pad, x*s+kx-pad, i]
 *   db[o]            (+)= sum_{n,y,x} g[n,y,x,o]
 * written in the reference's own parameter layout (OIHW for Conv2d; for
 * ConvTranspose2d pass g := the layer input, src := the output gradient, which yields
 * IOHW).  Two stages: partial products per pixel split into `slabs`, then a reduction
 * that ACCUMULATES into dw/db (gradients of weights shared over the T steps add up,
 * SURVEY.md A.2 first row).
 * ---------------------------------------------------------------------------------- */
#define REFID_WGRAD_MAX_GROUPS 24
typedef struct refid_wgrad_desc {
    const float* g;      int ld_g;   int c_o;   /* output-gradient, (n,ho,wo,c_o)       */
    const float* in_a;   const float* in_b;     /* conv input sources, (n,h,w,c_a|c_b)  */
    int ld_a, ld_b;
    int c_a, c_b;
    float* dw;                                  /* (c_o, c_a+c_b, kh, kw) accumulated   */
    float* db;                                  /* (c_o) accumulated, or NULL           */
    float* slabs;                               /* workspace, refid_wgrad_workspace_bytes */
    int n, h, w, ho, wo;
    int kh, kw, stride, pad;
    int i_base, i_total;                        /* dw second-dim offset / full size (slices) */
    int o_real;                                 /* rows of dw/db actually written (<= c_o); the
                                                   rest of g's channels is padding        */
    int algo;                                   /* 0 = direct; 1 = Winograd F(2x2,3x3) (3x3 stride 1);
                                                   2 = direct with bf16 MFMA operands (3x3 stride 1 pad 1, more than 32
                                                   output and input channels; fp32 accumulation / slabs / dw; slab
                                                   geometry and phases identical to algo 0);
                                                   (3, 4, 6: experiments of ABI <= 8 -- six bf16 products, LDS-DMA staging,
                                                   F(3x3,4x4) -- that did not beat algo 1 / 5: rejected with a message);
                                                   5 = Winograd over 2x4 tiles of g (3x3 stride 1): F(3,2) down the rows,
                                                   F(3,4) along them -- 24 instead of 32 fp32 MFMAs per 8 pixels, packed
                                                   transforms (wgrad_wino24.hip; slabs [split][24][o][i]; pitches / channel
                                                   counts multiples of 4 floats, 16-byte aligned tensors, c_a % 32 == 0 for two
                                                   sources); deviation from the float64 gradient 3e-6 .. 6e-6 of scale;
                                                   7 = conv_down (4x4 stride 2 pad 1, even input size): Winograd F(2,3) x F(2,4) tiles on the
                                                   four parity phases of the input (a stride-2 conv is four 2x2-tap stride-1
                                                   convs on them): 6.67 instead of 16 fp32 MFMA-units per output pixel; slabs
                                                   [split][phase][20][o][i];
                                                   8 = the 2x2 stride-2 pad-0 weight gradient over NON-overlapping patches
                                                   (ConvTranspose2d(2,2) with the roles swapped, see above) as one streaming 1x1
                                                   weight gradient (wgrad_pws.hip): K = (dy, dx, c) over the even / odd rows of
                                                   the source, which must have dense pixels (ld_a == c_a; one source, no db,
                                                   c_o >= 64 and a multiple of 32, c_a a multiple of 16, wo a multiple of 32);
                                                   the reduction permutes the columns into dw's [o][c][dy][dx] layout  */
    int phase;                                  /* 0 = partial products + reduction in one call;
                                                   weights shared over the T recurrent steps can instead
                                                   keep accumulating in their own `slabs`:
                                                   1 = partial products, OVERWRITE slabs (first step),
                                                   2 = partial products, ADD into slabs (later steps),
                                                   3 = reduction of the slabs into dw/db only (after BPTT);
                                                   4 = as 3, but only the streaming first stage runs now: the element-wise
                                                   stage is QUEUED and refid_wgrad_finish_flush issues every queued stage as
                                                   one launch per kernel family (a step's ~130 small reductions are
                                                   independent of each other; the caller must not touch `slabs`, dw or db
                                                   between the call and the flush; two queued calls on the same dw block
                                                   flush the queue in between);
                                                   the slab geometry depends on (c_o, i_total), not on c_a/c_b */
    int groups;                                 /* phases 0-2 (not the thin / 1x1 register tiles): 2..REFID_WGRAD_MAX_GROUPS = this launch also adds the
                                                   partial products of groups-1 MORE time steps of the same convolution
                                                   (weights are shared over the T steps; same geometry, pitches and
                                                   source split): one pass over the slabs instead of one per step.
                                                   0 / 1 = just (g, in_a, in_b).                                        */
    const float* g_more[REFID_WGRAD_MAX_GROUPS - 1];
    const float* in_a_more[REFID_WGRAD_MAX_GROUPS - 1];
    const float* in_b_more[REFID_WGRAD_MAX_GROUPS - 1];
} refid_wgrad_desc;

size_t refid_wgrad_workspace_bytes(const refid_wgrad_desc* d);
int refid_conv2d_wgrad(const refid_wgrad_desc* d, void* stream);
/* Issues the element-wise reduction stages queued by phase-4 calls (of this host thread) on `stream`: one launch per kernel
 * family and 40 jobs (autograd's accumulation of the T steps' weight gradients, twoImage_event_recurrent_model.py:303; the
 * reference has no counterpart -- its 2T per-step gradients are added by autograd one by one).  No queued job: no launch. */
int refid_wgrad_finish_flush(void* stream);

/* ------------------------------------------------------------------------------------
 * Weight packing: reference layouts (Conv2d OIHW, ConvTranspose2d IOHW) -> the tile's
 * [chunk][tap][row][KC] layout, rows/chunks zero padded.
 *   role FWD   : rows = O, k = I, taps in order
 *   role DGRAD : rows = I, k = O, taps flipped (stride-1 convs), or 2x2/s2 (convT input
 *                gradient), or the four parity classes of conv4x4/s2 (mode 2)
 *   role CONVT : ConvTranspose2d forward (mode 1): rows = (dy,dx,Co), k = Ci
 * Every entry point below -- the size functions, the one-by-one calls, refid_pack_entry_fill --
 * builds the same record with the same conditions (csrc/pack.hip): o, i, kc, bn positive; the
 * convT roles take a 2x2 kernel, DOWN_DGRAD a 4x4, the Winograd roles a 3x3 (kc = 8 in the fp32
 * tile layout, no bf16 form); a scale only with the FWD / DGRAD / Winograd roles; the Winograd
 * plane forms below 2^31 plane entries.  A size function answers 0 where a call would refuse.
 * ---------------------------------------------------------------------------------- */
enum { REFID_ROLE_FWD = 0, REFID_ROLE_DGRAD = 1, REFID_ROLE_CONVT = 2, REFID_ROLE_CONVT_DGRAD = 3,
       REFID_ROLE_DOWN_DGRAD = 4,
       /* Winograd-domain weights U = G g G^T, 16 "taps" (algo 1; kc = 8): */
       REFID_ROLE_WINO_FWD = 5, REFID_ROLE_WINO_DGRAD = 6,
       /* ConvTranspose2d(2,2) input gradient as ONE GEMM over 2x2 patches (refid_conv2d algo 3 on a 2x2 stride-2 conv): rows = Ci,
          k = (dy, dx, co) = 4 Co columns, one "tap"; kc = 8, bn = 32: */
       REFID_ROLE_CONVT_DGRAD_PW = 7 };
size_t refid_packed_weight_floats(int role, int o, int i, int kh, int kw, int kc, int bn);
int refid_pack_conv_weights(const float* w, float* packed, int role, int o, int i, int kh, int kw,
                            int kc, int bn, void* stream);

/* Same as refid_pack_conv_weights with a per-OUTPUT-channel factor folded in (FWD/DGRAD
 * roles).  Used to fold EGACA's beta / gamma (fusion_modules.py:287-288,319,331:
 * `y = ev + img + x*beta`, `return y + x*gamma`) into conv3 / conv5 so the scaled branch
 * and the residual add run in the conv tile's epilogue. */
int refid_pack_conv_weights_scaled(const float* w, const float* oscale, float* packed, int role, int o,
                                   int i, int kh, int kw, int kc, int bn, void* stream);
/* bf16 copy of the same packed layout (RNE), kc = 2 * refid_conv_kc(...); oscale may be NULL (and must be, but for the FWD / DGRAD
 * roles).  No Winograd roles. */
int refid_pack_conv_weights_bf16(const float* w, const float* oscale, void* packed_bf16, int role, int o, int i,
                                 int kh, int kw, int kc, int bn, void* stream);
/* Split-bf16 packing for refid_conv2d algo 4: every weight (times oscale[row] when given) is written as `planes` bf16
 * numbers h = rne(v), m = rne(v - h), l = v - h - m (planes = 3: exact; 2: h, m; 1: h), in 8-channel sub-chunks:
 *   3x3 (REFID_ROLE_FWD / REFID_ROLE_DGRAD):     [chunk8][plane][tap 0..9][rows padded to bn][8]   (tap 9 = zeros)
 *   4x4 stride 2, REFID_ROLE_FWD (conv_down):     [chunk8][in-block row sy][in-block column sx][plane][block tap (ty,tx)]
 *                                                 [rows][8] = W[row][k][2ty+sy][2tx+sx]
 *   4x4 stride 2, REFID_ROLE_DOWN_DGRAD:          [parity class][chunk8][plane][tap (ta,tb)][rows][8]
 *   1x1 (REFID_ROLE_FWD / REFID_ROLE_DGRAD, refid_conv2d algo 3 with mfma_terms 6, bn = 32):
 *                                                 [chunk16][plane][rows padded to bn][16], a row's 16 channels stored as the
 *                                                 two K halves of the pointwise tile's lanes: slot 8h + t = channel 4h + t
 *                                                 (t < 4) or 8 + 4h + (t - 4)
 * refid_packed_weight_split_bytes gives the buffer size. */
size_t refid_packed_weight_split_bytes(int role, int o, int i, int kh, int kw, int bn, int planes);
/* The 3x3 / 4x4 layouts above with TWO fp16 planes h = rne16(w 2^eW), l = rne16(w 2^eW - h) behind a 64-byte header (int eW at
 * byte 0: max |w| 2^eW in [2^12, 2^13), found by a reduction over the tensor that the call launches first), for refid_conv2d
 * algo 4 with mfma_terms = 19.  `packed` must be 16-byte aligned. */
size_t refid_packed_weight_split_f16_bytes(int role, int o, int i, int kh, int kw, int bn);
int refid_pack_conv_weights_split_f16(const float* w, const float* oscale, void* packed, int role, int o, int i,
                                      int kh, int kw, int bn, void* stream);
int refid_pack_conv_weights_split(const float* w, const float* oscale, void* packed, int role, int o, int i,
                                  int kh, int kw, int bn, int planes, void* stream);
/* Winograd-domain weights U = G g G^T (times oscale[row] when given) for refid_conv2d algo 5: computed in fp32 like
 * REFID_ROLE_WINO_FWD / REFID_ROLE_WINO_DGRAD, then written as three bf16 planes that sum to U exactly:
 *   [chunk of 16 input channels][xi = 0..15][plane][rows padded to bn = 64][16]  (bf16). */
size_t refid_packed_weight_wino6_bytes(int role, int o, int i, int bn);
int refid_pack_conv_weights_wino6(const float* w, const float* oscale, void* packed, int role, int o, int i, int bn,
                                  void* stream);
/* The same U for refid_conv2d algo 5 with mfma_terms = 3: a 64-byte header (int eU at byte 0: the packing's power-of-two
 * scale, max |U| 2^eU in [2^12, 2^15), found by a reduction over the tensor that the call launches first) followed by
 *   [chunk of 16 input channels][xi = 0..15][plane h / l][rows padded to bn = 64][16]  (fp16),
 * h = rne16(U 2^eU), l = rne16(U 2^eU - h).  `packed` must be 16-byte aligned. */
size_t refid_packed_weight_wino3h_bytes(int role, int o, int i, int bn);
int refid_pack_conv_weights_wino3h(const float* w, const float* oscale, void* packed, int role, int o, int i, int bn,
                                   void* stream);
/* The same U for refid_conv2d algo 5 with mfma_terms = 1: the same 64-byte header and scale, followed by the high plane only,
 *   [chunk of 16 input channels][xi = 0..15][rows padded to bn = 64][16]  (fp16),  rne16(U 2^eU).
 * Half the bytes of the two-plane packing after the header.  `packed` must be 16-byte aligned. */
size_t refid_packed_weight_wino1h_bytes(int role, int o, int i, int bn);
int refid_pack_conv_weights_wino1h(const float* w, const float* oscale, void* packed, int role, int o, int i, int bn,
                                   void* stream);
/* All packings of a model in ONE launch.  The caller builds a table of refid_pack_entry_bytes()-sized records in host
 * memory with refid_pack_entry_fill (kind 0: refid_pack_conv_weights[_scaled / _bf16] -- `planes` = 1 selects bf16 output;
 * 1: refid_pack_conv_weights_split, 3x3 / 4x4; 2: the same, 1x1; 3: refid_pack_conv_weights_wino6; 4: dst[e] = w[e] *
 * oscale[e] for e < o (refid_mul_vec); 5: refid_pack_conv_weights_wino3h, or -- `planes` = 1 -- refid_pack_conv_weights_wino1h; 6: refid_pack_conv_weights_split_f16), copies it to
 * device memory once, and calls
 * refid_pack_batch whenever the weights have changed -- after refid_pack_batch_prepass on the same stream when the table holds
 * kind-5 / kind-6 records (their scale exponents: one workgroup per record, a no-op for the other kinds).  `blk0` = the sum of the values returned for the records before this one (each call returns its record's
 * workgroup count >= 1, -1 on error -- the one-by-one entry points build their record the same way); nblocks = the sum over
 * all records.  refid_pack_table_check walks a finished HOST table (every record filled, first blocks consecutive from 0:
 * the kernel finds a workgroup's record by binary search over them) and returns that sum, -1 on error.  Same bits as the
 * one-by-one calls. */
size_t refid_pack_entry_bytes(void);
int refid_pack_table_check(const void* table_host, int n);
int refid_pack_entry_fill(void* entry_host, int kind, const float* w, const float* oscale, void* dst, int role, int o, int i,
                          int kh, int kw, int kc, int bn, int planes, int blk0);
int refid_pack_batch_prepass(const void* table_dev, int n, void* stream);
int refid_pack_batch(const void* table_dev, int n, int nblocks, void* stream);
int refid_mul_vec(const float* a, const float* b, float* out, int n, void* stream);
/* After BPTT, turn the gradient of the FOLDED conv (scale[r]*W[r,:], scale[r]*b[r]) of THIS backward pass
 * (gw_folded, gb_folded: private buffers, zero before BPTT) into gradients of (W, b, scale) and ACCUMULATE them:
 *   dscale[r] += <W[r,:],Gf[r,:]> + b[r]*gbf[r];  gw[r,:] += scale[r]*Gf[r,:];  gb[r] += scale[r]*gbf[r].
 * (gw/gb may already hold gradients of earlier backward passes: gradient accumulation stays exact.) */
int refid_fold_back(const float* w, const float* b, const float* scale, const float* gw_folded,
                    const float* gb_folded, float* gw, float* gb, float* dscale, int rows, int k, void* stream);

/* ------------------------------------------------------------------------------------
 * EGACA non-GEMM pieces (fusion_modules.py:290-333) and LayerNorm2d (fusion_modules.py:97-134).
 * c in {16,32,64,128}.  Parameter gradients ACCUMULATE into dw/db (deterministic: per-workgroup partial rows in the
 * caller's scratch, finished in index order -- no floating-point atomics).
 * ---------------------------------------------------------------------------------- */
int refid_layernorm2d_fwd(const float* x, int ld_x, const float* w, const float* b, float* out,
                          int ld_out, long long npix, int c, float eps, void* stream);
/* LayerNormFunction.backward, fusion_modules.py:110-122; gx = (res ? res : 0) + dL/dx.  res may be
 * NULL or alias gx (in-place accumulate); pass a distinct gx when another stream still reads res. */
/* parts: scratch of refid_layernorm2d_bwd_parts(npix, c) * 2c floats (per-workgroup partial sums of dw / db, added in a
 * fixed order: the parameter gradients are deterministic, no floating-point atomics). */
int refid_layernorm2d_bwd_parts(long long npix, int c);
int refid_layernorm2d_bwd(const float* g, int ld_g, const float* x, int ld_x, const float* w, float* gx,
                          int ld_gx, const float* res, int ld_res, float* dw, float* db, float* parts, long long npix,
                          int c, float eps, void* stream);
/* ------------------------------------------------------------------------------------
 * SingleMultiConnectEVHINet non-GEMM pieces (SURVEY.md 8f row 4;
 * archs/single_multiconnect_evhinet_arch.py:233-237 HIN + LeakyReLU, archs/arch_util.py:421-426 FAC_bias).
 * Deterministic (two-stage reductions, no atomics).
 * ---------------------------------------------------------------------------------- */
int refid_hin_parts(int hw);                 /* partial-sum rows the scratch buffers must hold per sample */
/* out = LeakyReLU( [ InstanceNorm(x[:, :ch]) * gamma + beta | x[:, ch:] ] ); biased variance, eps inside the
 * root; stats (n,2,ch) receives mean / rstd; parts = scratch (n, refid_hin_parts(hw), 2, ch).  ch = 0: plain
 * LeakyReLU.  ch must be 4 * 2^k. */
int refid_hin_lrelu_fwd(const float* x, int ld_x, const float* gamma, const float* beta, float* out, int ld_out,
                        float* stats, float* parts, int n, int hw, int c, int ch, float eps, float slope,
                        void* stream);
/* gx = d/dx of the above given g = dL/dout; dgamma/dbeta ACCUMULATE; sums = scratch (n,2,ch). */
int refid_hin_lrelu_bwd(const float* g, int ld_g, const float* out, int ld_out, const float* x, int ld_x,
                        const float* gamma, const float* stats, float* gx, int ld_gx, float* dgamma,
                        float* dbeta, float* sums, float* parts, int n, int hw, int c, int ch, float slope,
                        void* stream);
/* FAC_bias: out = feat * filt[:, :c] + filt[:, c:2c]  and its backward (gfilt = [g*feat | g]). */
int refid_fac_fwd(const float* feat, int ld_feat, const float* filt, int ld_filt, float* out, int ld_out,
                  long long npix, int c, void* stream);
int refid_fac_bwd(const float* g, int ld_g, const float* feat, int ld_feat, const float* filt, int ld_filt,
                  float* gfeat, int ld_gfeat, float* gfilt, int ld_gfilt, long long npix, int c, void* stream);

/* pre = dwconv3x3(in)+b ; act = GELU(pre) ; pool[n][part][c] = per-workgroup partial sums of act
 * (fm:304-309 + se_1's AdaptiveAvgPool2d, fm:253-254; pool may be NULL; parts =
 * refid_dwconv_pool_parts(h,w,c); deterministic, no atomics).  w is the reference (c,1,3,3) tensor. */
int refid_dwconv_pool_parts(int h, int wd, int c);
int refid_dwconv3x3_gelu_fwd(const float* in, int ld_in, const float* w, const float* b, float* pre,
                             float* act, float* pool, int n, int h, int wd, int c, void* stream);
/* gd = gradient w.r.t. `pre`; gin = input gradient; dw/db accumulate.  parts: scratch of
 * n * refid_dwconv3x3_bwd_parts(h,wd,c) * 10c floats (deterministic two-stage reduction; required). */
int refid_dwconv3x3_bwd_parts(int h, int wd, int c);
int refid_dwconv3x3_bwd(const float* gd, const float* in, int ld_in, const float* w, float* gin,
                        float* dw, float* db, float* parts, int n, int h, int wd, int c, void* stream);
/* se_1 (fm:253-260): m = (sum_parts pool)*inv_hw ; z1 = relu(W1 m + b1) ; s = sigmoid(W2 z1 + b2) */
int refid_se_fwd(const float* pool, int n_parts, float inv_hw, const float* w1, const float* b1, const float* w2,
                 const float* b2, float* m, float* z1, float* s, int n, int c, void* stream);
/* scratch: n * (c + c/2) floats; the samples' contributions to dw1 / db1 / dw2 / db2 are added in sample order */
int refid_se_bwd(const float* gs, const float* s, const float* z1, const float* m, const float* w1,
                 const float* w2, float* gm, float* dw1, float* db1, float* dw2, float* db2, float* scratch, int n,
                 int c, void* stream);
/* out[n,p,0:c] = xi*s[n] ; out[n,p,c:2c] = xe*s[n]   (fm:312-315, no cat temporary) */
int refid_scale_cat(const float* xi, const float* xe, const float* s, float* out, int n, int hw, int c,
                    void* stream);
/* gs[n][c] = sum_p gxs[n,p,c]*xi + gxs[n,p,c+C]*xe  (dL/ds of the two products) */
/* parts: scratch of n * refid_egaca_gs_reduce_parts(hw, c) * c floats (fixed-order two-stage reduction) */
int refid_egaca_gs_reduce_parts(int hw, int c);
int refid_egaca_gs_reduce(const float* gxs, const float* xi, const float* xe, float* gs, float* parts, int n, int hw,
                          int c, void* stream);
/* gdwe = (gxs_e*s + gm*inv_hw) * GELU'(dwe) ; gxi (+)= gxs_i*s */
int refid_egaca_bwd_elem(const float* gxs, const float* s, const float* gm, float inv_hw, const float* dwe,
                         float* gdwe, float* gxi, int accumulate_xi, int n, int hw, int c, void* stream);
int refid_gelu_fwd(const float* in, float* out, long long count, void* stream);
int refid_gelu_bwd(const float* g, const float* in, float* out, long long count, void* stream);
/* db[c] += sum_p g[p][c]   (bias gradient where the wgrad call does not carry it); parts: scratch of
 * refid_colsum_parts(npix, c) * c floats (fixed-order two-stage reduction) */
int refid_colsum_parts(long long npix, int c);
int refid_colsum(const float* g, int ld_g, float* db, float* parts, long long npix, int c, void* stream);

/* ------------------------------------------------------------------------------------
 * Train-step tail (twoImage_event_recurrent_model.py:273-310; losses/losses.py:28-30,143-173).
 * ---------------------------------------------------------------------------------- */
/* Every scalar reduction of this section and of the validation tail below is TWO-STAGE and deterministic (no floating-point
 * atomics: a logged loss / PSNR / SSIM does not depend on workgroup arrival order): per-workgroup partial sums go to the
 * caller's `parts` scratch (refid_*_parts(...) doubles), a second launch adds them in index order. */
/* *loss_sum = sum sqrt((pred-gt)^2+eps); grad = (pred-gt)/sqrt(.)*grad_scale (grad may be NULL);
 * parts: refid_charbonnier_parts(count) doubles. */
int refid_charbonnier_parts(long long count);
int refid_charbonnier(const float* pred, const float* gt, float* grad, double* loss_sum, double* parts, long long count,
                      float eps, float grad_scale, void* stream);
/* PSNRLoss (losses.py:95-120, toY = False; image_event_restoration_model.py uses it for the HINet network):
 * *loss = weight * 10/ln10 * mean_b log(mse_b + 1e-8), mse_b over the per_sample elements of sample b;
 * grad (may be NULL) = d loss / d pred; sq = n_samples doubles (receives the per-sample squared errors);
 * parts: refid_psnr_loss_parts(n_samples, per_sample) doubles. */
int refid_psnr_loss_parts(int n_samples, long long per_sample);
int refid_psnr_loss(const float* pred, const float* gt, float* grad, double* sq, double* loss, double* parts, int n_samples,
                    long long per_sample, float weight, void* stream);
/* out[0] = sum g^2 (deterministic two-stage reduction: replicas of a data-parallel job must agree bit for
 * bit); `out` must hold REFID_SQNORM_WORDS doubles (out[1..] is scratch). */
#define REFID_SQNORM_WORDS 2049
int refid_grad_sqnorm(const float* g, double* out, long long count, void* stream);
/* clip_grad_norm_(max_norm) (max_norm <= 0: off) + AdamW step over flat arenas; gradients are
 * pre-multiplied by grad_scale (1/world_size after a SUM all-reduce). */
int refid_clip_adamw(float* p, const float* g, float* m, float* v, const double* sqnorm, float max_norm,
                     float grad_scale, float lr, float beta1, float beta2, float eps, float weight_decay,
                     int step, long long count, void* stream);

/* The same step with the per-iteration scalars in DEVICE memory: hyper[0] = lr, hyper[1] = 1 - beta1^t,
 * hyper[2] = sqrt(1 - beta2^t).  A train step captured in a hipGraph is replayed with different lr / t every
 * iteration; kernel arguments are frozen at capture time, device memory is not. */
int refid_clip_adamw_dev(float* p, const float* g, float* m, float* v, const double* sqnorm, float max_norm,
                         float grad_scale, const float* hyper, float beta1, float beta2, float eps,
                         float weight_decay, long long count, void* stream);

/* ------------------------------------------------------------------------------------
 * Layout / elementwise helpers on the boundary.
 * ---------------------------------------------------------------------------------- */
/* NCHW (n,c,h,w) -> NHWC (n,h,w,c_pad), channels >= c zero filled.  Replaces the
 * einops.rearrange calls at XXNet_final_attenfusion_arch.py:140-143 (layout change only). */
int refid_nchw_to_nhwc(const float* src, long long src_batch_stride, float* dst, int n, int c, int h, int w,
                       int c_pad, void* stream);
/* The same conversion of sum_t src[:, t]: src is (n, t_count, c, h, w) with the given batch / time strides (floats).
 * Gradient of a tensor every time step reads (`head` in `pred(z_t + head)`, XXNet_final_attenfusion_arch.py:215):
 * autograd sums the T per-step gradients. */
int refid_nchw_tsum_to_nhwc(const float* src, long long src_batch_stride, long long t_stride, int t_count, float* dst,
                            int n, int c, int h, int w, int c_pad, void* stream);
/* NHWC (n,h,w,ld) first c channels -> NCHW (n,c,h,w) with an output batch stride (so a
 * (B,T,3,H,W) stack is written in place: XXNet_final_attenfusion_arch.py:218). */
int refid_nhwc_to_nchw(const float* src, int ld, float* dst, long long dst_batch_stride,
                       int n, int c, int h, int w, void* stream);
/* The two conversions for a whole (B, T, C, H, W) stack in ONE launch, TIME-MAJOR on the NHWC side: NHWC sample t nb + b
 * <-> the stack's (b, t) block at b b_stride + t t_stride floats.  The event stack in (XXNet_final_attenfusion_arch.py:149,
 * 172-176: the recurrent loops read e[:, t]), the output stack out and its gradient back in (arch:218). */
int refid_nchw_to_nhwc_tb(const float* src, long long b_stride, long long t_stride, float* dst, int nb, int nt, int c, int h,
                          int w, int c_pad, void* stream);
int refid_nhwc_to_nchw_tb(const float* src, int ld, float* dst, long long b_stride, long long t_stride, int nb, int nt, int c,
                          int h, int w, void* stream);
/* Deferred per-channel parameter-gradient sums.  refid_layernorm2d_bwd, refid_dwconv3x3_bwd and refid_colsum each end with a
 * small launch that adds their per-workgroup partial rows into dw / db (autograd's accumulation of the T steps' gradients,
 * twoImage_event_recurrent_model.py:303).  refid_rows_sum_defer(1) makes these calls (of this host thread) QUEUE that sum
 * instead; refid_rows_sum_flush issues the queued sums grouped by destination, in call order within a destination (the bits of
 * the one-by-one launches), as one launch per ~160 sums, and turns deferral off.  Between the two the caller keeps every `parts`
 * buffer alive and the destinations untouched.  refid_rows_sum_defer also drops whatever an aborted pass left queued. */
int refid_rows_sum_defer(int on);
int refid_rows_sum_flush(void* stream);
/* out = a + b (skip sums: XXNet_final_attenfusion_arch.py:16-17,199-203,211,215;
 * recurrent_sub_modules.py:278). count = number of floats, multiple of 4. */
int refid_add(const float* a, const float* b, float* out, long long count, void* stream);
/* out = in[0] + ... + in[n-1] in index order (n <= REFID_SUM_MAX host pointers to device tensors of `count` floats; out may
 * alias in[0]).  The sums autograd accumulates over the T steps that share a tensor (x_blocks, head, the final backward
 * states: SURVEY.md A.2 "residual / skip adds") in one launch after BPTT. */
#define REFID_SUM_MAX 48
int refid_sum_n(const float* const* in, int n, float* out, long long count, void* stream);
/* out = (acc ? out : 0) + g * (y > 0 ? 1 : slope): activation derivative. */
int refid_act_bwd(const float* g, const float* y, float* out, float slope, int accumulate,
                  long long count, void* stream);

/* ------------------------------------------------------------------------------------
 * Callers either side of the path.
 * ---------------------------------------------------------------------------------- */
/* events_to_voxel_grid (basicsr/data/event_util.py:6-66): voxel (num_bins,height,width) is zeroed,
 * then every event adds pol*(1-dt) to bin floor(t') and pol*dt to the next, t' = (bins-1)(t-first)/dT;
 * polarity 0 counts as -1.  fp32 atomics: summation order differs from np.add.at (tolerance). */
int refid_events_to_voxel(const double* ts, const int* xs, const int* ys, const float* ps, long long n_events,
                          int num_bins, int width, int height, double first_stamp, double last_stamp,
                          float* voxel, void* stream);
/* tensor2img quantisation (utils/img_util.py:90-117: clamp [0,1], x255, round) fused with the squared
 * error of calculate_psnr (metrics/psnr_ssim.py:48-63): sq[f] = sum (q(a)-q(b))^2 per frame, float64;
 * parts: refid_sqerr_u8_parts(...) doubles (refid_ssim3d_u8: refid_ssim3d_u8_parts(...)). */
int refid_sqerr_u8_parts(int n_frames, long long frame_elems);
int refid_sqerr_u8(const float* a, const float* b, int n_frames, long long frame_elems, double* sq, double* parts,
                   void* stream);
/* calculate_ssim -> _ssim_3d (metrics/psnr_ssim.py:135-182,225-303): separable 11^3 Gaussian (sigma 1.5,
 * replicate padding) over (H, W, C=3) of the uint8-quantised frames, fp32; sum_out[f] = sum of the ssim
 * map of frame f (divide by 3*h*w for the mean).  a, b: (n_frames, 3, h, w) in [0,1]. */
int refid_ssim3d_u8_parts(int n_frames, int h, int w);
int refid_ssim3d_u8(const float* a, const float* b, int n_frames, int h, int w, double* sum_out, double* parts,
                    void* stream);
/* The validation tail of one item in one pass (twoImage_event_recurrent_model.py:412-432 get_current_visuals +
 * tensor2img per frame, utils/img_util.py:59-121; :460-491 calculate_psnr / calculate_ssim per frame,
 * metrics/psnr_ssim.py:9-63,135-182,225-303).  pred, gt: (n_frames, 3, h, w) fp32 NCHW.  pred_u8 / gt_u8:
 * (n_frames, h, w, 3) uint8, tensor2img's quantisation (clamp [0,1], x255, round half to even); flags &
 * REFID_VAL_TAIL_BGR writes the channels as tensor2img(rgb2bgr=True) returns them, otherwise RGB (what a PNG holds).
 * sq_out[f] = sum (q(pred)-q(gt))^2 of frame f as an exact integer (calculate_psnr's MSE numerator);
 * ssim_out[f] = the sum refid_ssim3d_u8 gives for frame f, bit for bit.  gt, gt_u8, sq_out and ssim_out may each be
 * NULL (gt NULL: conversion only); parts: refid_val_tail_parts(...) 8-byte words, needed with sq_out or ssim_out. */
#define REFID_VAL_TAIL_BGR 1
long long refid_val_tail_parts(int n_frames, int h, int w);
int refid_val_tail(const float* pred, const float* gt, int n_frames, int h, int w, int flags, unsigned char* pred_u8,
                   unsigned char* gt_u8, unsigned long long* sq_out, double* ssim_out, void* parts, void* stream);
/* grids_inverse (twoImage_event_recurrent_model.py:252-268): acc[:, i0:i0+th, j0:j0+tw] += tile,
 * cnt += 1; then acc /= cnt. */
int refid_tile_add(const float* tile, float* acc, float* cnt, int c, int th, int tw, int h, int w, int i0, int j0,
                   void* stream);
int refid_tile_normalize(float* acc, const float* cnt, int c, int h, int w, void* stream);

/* ------------------------------------------------------------------------------------
 * Training-batch assembly from raw frames and events (csrc/sample.hip): the device counterpart of the recurrent
 * datasets' __getitem__ (data/image_npy_dataset.py:188-232, data/image_sharp_npy_dataset.py:180-225) -- event
 * voxelisation restricted to the crop, paired crop, flip / flip / transpose, BGR->RGB and /255, and the lq / voxel / gt
 * layouts -- batched over the samples of a batch through a table of refid_sample_desc in device memory.
 * Bit-reproducible: the event sums are 64-bit fixed point (32 fractional bits) integer atomics, every float is one
 * correctly rounded operation.  Events outside the frame, outside the crop, or with a negative normalised time are
 * DROPPED (the reference's flat np.add.at index wraps or spills them into other pixels; that is not reproduced).
 * ---------------------------------------------------------------------------------- */
typedef struct refid_sample_desc {
    const float* events;                        /* (n_events,4) float32 rows [t,x,y,p], 16-byte aligned (device)  */
    long long n_events;                         /* may be 0                                                       */
    float first_stamp, last_stamp;              /* normalisation: ts = (bins-1)*(t-first)/(last-first), in fp32   */
    int height, width;                          /* full frame                                                     */
    const unsigned char* frames;                /* 2 + n_gt frames (blur0, blur1, gt...), u8 HWC BGR (device)     */
    long long frame_stride;                     /* bytes from one frame to the next (>= the uploaded window)      */
    int row_pitch;                              /* bytes from one row to the next                                 */
    int y0, x0;                                 /* frame coordinates of the uploaded window's first pixel         */
    int top, left;                              /* crop origin in frame coordinates                               */
    int hflip, vflip, rot90;                    /* transforms.py:110-129, applied in this order after the crop    */
} refid_sample_desc;

#define REFID_LAYOUT_BLUR 0    /* bins = 2m+n+1; lq (B, 6+2(m-1), h, w) = blur0 | bins 1..m-1 | blur1 | bins m+2+n..  */
#define REFID_LAYOUT_SHARP 1   /* bins = n+1;    lq (B, 2, 3, h, w)                                                  */
#define REFID_ASSEMBLE_ZERO 1
#define REFID_ASSEMBLE_SCATTER 2
#define REFID_ASSEMBLE_FINISH 4
#define REFID_ASSEMBLE_FRAMES 8
#define REFID_ASSEMBLE_ALL 15
typedef struct refid_assemble_desc {
    const refid_sample_desc* samples_host;      /* the table in host memory (validated on every call)             */
    const refid_sample_desc* samples_dev;       /* the same table in device memory (read by the kernels)          */
    int batch;
    int m, n, layout;
    int crop_h, crop_w;                         /* crop BEFORE the transpose; rot90 needs crop_h == crop_w        */
    long long* scratch;                         /* int64 [batch][bins][crop_h*crop_w]                             */
    float* lq;
    float* voxel;                               /* (batch, bins-1, 2, h, w): sliding bin pairs                    */
    float* gt;                                  /* (batch, bins-1, 3, h, w)                                       */
} refid_assemble_desc;

/* Number of voxel bins of a layout, or -1 (with the error text set) when (m, n, layout) is not supported. */
int refid_assemble_bins(int m, int n, int layout);
/* Runs the chosen stages (REFID_ASSEMBLE_*) in the order zero, scatter, finish, frames on `stream`: one launch each. */
int refid_assemble_batch(const refid_assemble_desc* d, int stages, void* stream);

/* ------------------------------------------------------------------------------------
 * voxel_norm (data/event_util.py:141-160) on the device, and the single-image event deblurring dataset's __getitem__
 * (data/Single_image_npy_dataset.py:136-201), the one place where the reference KEEPS voxel_norm's result (:187, after
 * crop and augmentation).  Per sample, with v the fp32 voxel element:
 *   S0 = #{v != 0}, S1 = sum v, S2 = sum v^2, mean64 = S1/S0, var64 = S2/S0 - mean64^2 (float64),
 *   mean_f = (float)mean64, std_f = (float)sqrt(var64),
 *   out = v != 0 ? (v - mean_f) / std_f : 0     -- one fp32 subtraction and one IEEE fp32 division, no contraction: the
 *                                                   reference's order, mask * (voxel - mean) / stddev.
 * Bit-reproducible, no floating-point atomics: a statistics launch writes one partial {S0, S1, S2} (three 8-byte words)
 * per (sample, chunk of 4096 elements) into `parts`, which the caller owns (refid_voxel_norm_parts words); the
 * normalising launch adds a sample's partials in index order.  S0 is an integer count.  S2 is float64 in a fixed tree
 * order (every v*v is exact in float64; within a chunk: 16 elements per thread at stride 256 in sequence, the 64 lanes of
 * a wave by the xor tree 1,2,..,32, the 4 waves in order).  S1 is float64 in that same order on the stand-alone route and
 * an exact int64 sum of v*2^32 on the fused route, where v = (float)a * 2^-32 of the int64 scratch is a multiple of
 * 2^-32.  The order depends on an element's index inside its sample only: the result does not depend on the run, the
 * batch size, the sample's position in the batch, or the other samples.  Inputs must be finite.
 * Degenerate samples:
 *   S0 == 0: the output is all zeros (the reference leaves the voxel untouched: the same thing).
 *   var64 <= 0 or std_f == 0 (one non-zero element, or all non-zero elements equal): the output is all zeros.  The
 *   reference divides 0 by 0 there and returns an all-NaN voxel; that is NOT reproduced, a deliberate departure like
 *   the dropped events above.
 * ---------------------------------------------------------------------------------- */
/* 8-byte words of `parts` for `batch` samples of `per_sample` elements */
long long refid_voxel_norm_parts(int batch, long long per_sample);
/* Stand-alone form on an fp32 (batch, per_sample) tensor, e.g. a voxel that arrives already assembled; out == in is
 * allowed.  Two launches on `stream`. */
int refid_voxel_norm(const float* in, float* out, int batch, long long per_sample, void* parts, void* stream);

#define REFID_ASSEMBLE_STATS 16
typedef struct refid_single_desc {
    const refid_sample_desc* samples_host;      /* as refid_assemble_desc; frames: 2 per sample, blur then sharp   */
    const refid_sample_desc* samples_dev;
    int batch;
    int bins;                                   /* >= 1 and != 3 (img2tensor would swap bins 0 and 2)             */
    int crop_h, crop_w;                         /* crop BEFORE the transpose; rot90 needs crop_h == crop_w        */
    int norm;                                   /* 0: voxel = the plain bins; 1: voxel_norm per sample            */
    long long* scratch;                         /* int64 [batch][bins][crop_h*crop_w]                             */
    void* parts;                                /* refid_voxel_norm_parts(batch, bins*crop_h*crop_w) words; norm  */
    float* lq;                                  /* (batch, 3, h, w): frame 0, BGR -> RGB, /255                    */
    float* voxel;                               /* (batch, bins, h, w): plain bins, not sliding pairs             */
    float* gt;                                  /* (batch, 3, h, w): frame 1                                      */
} refid_single_desc;
/* `bins`, or -1 (with the error text set) when the single layout does not support it. */
int refid_single_bins(int bins);
/* Runs the chosen stages (REFID_ASSEMBLE_* and REFID_ASSEMBLE_STATS) in the order zero, scatter, stats, finish, frames
 * on `stream`: one launch each for the whole batch.  Scatter and frames are the kernels of refid_assemble_batch; stats
 * is skipped when norm == 0.  With norm == 1 the fused result equals refid_voxel_norm applied to the norm == 0 voxel of
 * the same call, bit for bit (float64 adds multiples of 2^-32 exactly while the partial sums stay below 2^21).  Fewer
 * than 2^30 events per sample with norm (S1 stays inside int64). */
int refid_assemble_single(const refid_single_desc* d, int stages, void* stream);

/* ------------------------------------------------------------------------------------
 * Test-time assembly of network inputs for frame pairs of ONE resident sequence (csrc/sequence.hip): the key frames and
 * the whole event stream are uploaded once, and every pair (two key-frame indices + a row window of the stream) becomes
 * one sample of `lq` / `voxel` in the layouts of refid_assemble_batch.  No crop, no flips, no ground truth.  The event
 * arithmetic is that of refid_assemble_batch, bit for bit (fp32 normalisation in three roundings, 64-bit fixed-point
 * integer atomics, one rounding to fp32; events outside the frame or with a negative normalised time are dropped;
 * polarity <= 0 counts as -1).  Frames of any size: the outputs are (out_h, out_w) >= (height, width) planes, filled in
 * the same launches -- image channels replicate the last row / column (np.pad mode="edge"), voxel channels are zero
 * there.  Pair windows may overlap, be adjacent, be empty, or all cover the same rows.  The host table and every
 * argument are validated on each call: -1 with refid_last_error() naming the offending field, nothing launched.
 * The library allocates nothing.
 * ---------------------------------------------------------------------------------- */
typedef struct refid_seq_pair {
    int left, right;                            /* key-frame indices into `frames`                                */
    long long row0, row1;                       /* event rows [row0, row1) of the stream; may be empty            */
    float first_stamp, last_stamp;              /* ts = (bins-1)*(t-first)/(last-first) in fp32, as refid_sample_desc */
} refid_seq_pair;
typedef struct refid_seq_desc {
    const float* events;                        /* device, (n_events,4) float32 rows [t,x,y,p], 16-byte aligned    */
    long long n_events;                         /* may be 0                                                       */
    const unsigned char* frames;                /* device, n_frames u8 HWC key frames                             */
    int n_frames;
    long long frame_stride;                     /* bytes from one frame to the next                               */
    int row_pitch;                              /* bytes from one row to the next                                 */
    int height, width;
    int bgr;                                    /* != 0: BGR as decoded by cv2 (swapped to RGB); 0: RGB           */
    const refid_seq_pair* pairs_host;           /* the pair table in host memory (validated on every call)        */
    const refid_seq_pair* pairs_dev;            /* the same table in device memory (read by the kernels)          */
    int n_pairs;
    int m, n, layout;                           /* REFID_LAYOUT_BLUR / REFID_LAYOUT_SHARP                         */
    int out_h, out_w;                           /* >= height, width: the padded size the network takes            */
    long long* scratch;                         /* int64 [n_pairs][bins][height*width]                            */
    float* lq;                                  /* sharp: (P, 2, 3, out_h, out_w); blur: (P, 6+2(m-1), out_h, out_w) */
    float* voxel;                               /* (P, bins-1, 2, out_h, out_w): sliding bin pairs                */
} refid_seq_desc;
/* Runs the chosen stages (REFID_ASSEMBLE_*) in the order zero, scatter, finish, frames on `stream`: one launch each. */
int refid_seq_assemble(const refid_seq_desc* d, int stages, void* stream);

/* ------------------------------------------------------------------------------------
 * Test-time assembly for the single-image deblurring network from ONE resident sequence: every item (a blurry frame + a
 * row window of the stream, its exposure) becomes one sample of `lq` / `voxel` in the layout of refid_assemble_single,
 * without ground truth, crop or flips, at any frame size.  Items are refid_seq_pair rows: `left` is the blurry frame,
 * `right` is not read, [row0, row1) is the event window, first_stamp / last_stamp as above.
 * The voxel of an item is what refid_assemble_single gives for the same frame and events at a whole-frame crop without
 * flips, bit for bit: the same scatter arithmetic, and voxel_norm's statistics taken over the UNPADDED (bins, height,
 * width) scratch of the item, so that an element's place in the fixed summation order depends on its index in the
 * unpadded sample only; the padding (zero in voxel channels, the replicated last row / column in image channels) is
 * written by the same launches and never enters the statistics.  The departures of refid_assemble_single carry over:
 * events outside the frame or with a negative normalised time are dropped, and an item whose non-zero elements have no
 * spread (no event, one element, all equal) comes out all zeros where the reference's voxel_norm returns NaN.
 * Windows may overlap, be empty, or repeat.  Every field and the host table are validated on each call: -1 with
 * refid_last_error() naming the offending field, nothing launched.  The library allocates nothing and does not
 * synchronise.  No floating-point atomics.
 * ---------------------------------------------------------------------------------- */
typedef struct refid_seq_single_desc {
    const float* events;                        /* device, (n_events,4) float32 rows [t,x,y,p], 16-byte aligned    */
    long long n_events;                         /* may be 0                                                       */
    const unsigned char* frames;                /* device, n_frames u8 HWC blurry frames                          */
    int n_frames;
    long long frame_stride;                     /* bytes from one frame to the next                               */
    int row_pitch;                              /* bytes from one row to the next                                 */
    int height, width;
    int bgr;                                    /* != 0: BGR as decoded by cv2 (swapped to RGB); 0: RGB           */
    const refid_seq_pair* items_host;           /* the item table in host memory (validated on every call)        */
    const refid_seq_pair* items_dev;            /* the same table in device memory (read by the kernels)          */
    int n_items;
    int bins;                                   /* as refid_single_bins: >= 1 and != 3                            */
    int norm;                                   /* 0: voxel = the plain bins; 1: voxel_norm per item              */
    int out_h, out_w;                           /* >= height, width: the padded size the network takes            */
    long long* scratch;                         /* int64 [n_items][bins][height*width]                            */
    void* parts;                                /* refid_voxel_norm_parts(n_items, bins*height*width) words; norm */
    float* lq;                                  /* (P, 3, out_h, out_w)                                           */
    float* voxel;                               /* (P, bins, out_h, out_w): plain bins, not sliding pairs         */
} refid_seq_single_desc;
/* Runs the chosen stages (REFID_ASSEMBLE_* and REFID_ASSEMBLE_STATS) in the order zero, scatter, stats, finish, frames
 * on `stream`: one launch each for all items.  stats is skipped when norm == 0.  Fewer than 2^30 events per item with
 * norm (S1 stays inside int64). */
int refid_seq_assemble_single(const refid_seq_single_desc* d, int stages, void* stream);

/* ------------------------------------------------------------------------------------
 * NIQE (basicsr/metrics/niqe.py calculate_niqe, convert_to='y'): the per-pixel half on the device (csrc/niqe.hip).  From
 * n_frames uint8 HWC frames (h, w, 3) -- RGB, or BGR with REFID_NIQE_BGR -- it produces, for both scales, the five moment
 * sums of the five maps of every block; the host turns them into AGGD features and the score (refid_amd/niqe.py).
 * The frame is cropped by crop_border on every side and then to hc x wc = floor(./96)*96 from the top-left; fewer than
 * 96 rows or columns: error.  Arithmetic, every step one correctly rounded operation, no contraction:
 *   v_c = fl32(u8/255);  y64 = ((b*24.966 + g*128.553) + r*65.481) + 16.0 in float64;  Y = fl32(fl32(y64/255.0) * 255)
 *   scale 2: Y2 = fl32(m(fl32(Y/255)) * 255), m the float32 2x2 mean, horizontal pair first, each a*0.5 + b*0.5
 *            (cv2.resize INTER_LINEAR at an exact factor 2; a stand-in that was never compared with a real cv2)
 *   mu64 / sq64 = sum over the 49 taps of window49 (float64, row-major, from a zero accumulator, acc = acc + w*x) of Y
 *            and of fl32(Y*Y), coordinates clamped at the edges of the cropped image;  mu = fl32(mu64), sq = fl32(sq64)
 *   n = (Y - mu) / (sqrt(|sq - mu*mu|) + 1) in float32
 *   maps of a block (96x96 at scale 1, 48x48 at scale 2): n, and fl32(n * roll(n, s)) for s = (0,1), (1,0), (1,1), (1,-1),
 *            the roll wrapping inside the block as np.roll does
 * sums: float64 [n_frames][2 scales][blocks][5 maps][5] with blocks = (hc/96)*(wc/96) in width-major order (block column
 * bw, block row bh -> bw*(hc/96) + bh, as the reference walks them) and the five entries
 *   count(x < 0), count(x > 0), sum_{x<0} x^2, sum_{x>0} x^2, sum |x|
 * the counts as exact float64 integers, the squares exact in float64, every sum a fixed-order tree without atomics: the
 * bits do not depend on the run, on n_frames or on the frame's place in the call.  Inside an area of constant colour mu
 * equals Y exactly and the map is exactly zero, as in the reference: zeros count on neither side.
 * parts: refid_niqe_moments_parts(...) 8-byte words of scratch; 0 with the present tiling (one workgroup per block), and
 * then parts may be NULL.  y_out (n_frames, hc, wc), mscn1_out (n_frames, hc, wc), mscn2_out (n_frames, hc/2, wc/2):
 * float32 planes Y and n per scale for tests, each may be NULL.  Two launches on `stream`; nothing is allocated.
 * ---------------------------------------------------------------------------------- */
#define REFID_NIQE_BGR 1
long long refid_niqe_moments_parts(int n_frames, int h, int w);
int refid_niqe_moments(const unsigned char* frames_u8, int n_frames, int h, int w, int flags, int crop_border,
                       const double* window49, double* sums, void* parts, float* y_out, float* mscn1_out,
                       float* mscn2_out, void* stream);

/* ------------------------------------------------------------------------------------
 * PNG reconstruction of inflated key frames (csrc/png.hip): the input is the inflate output of n_frames PNGs of one
 * (height, width, channels), unchanged and back to back -- per frame `height` rows of 1 + width*channels bytes, the first
 * byte of a row its filter type (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth); the output is uint8 (n_frames, height, width, 3)
 * in the file's channel order, a grey file (channels 1) replicated to three channels.  The arithmetic is the PNG
 * specification's: per byte a = the byte bpp to the left, b = the byte above, c = the byte above-left, each 0 outside the
 * image; Sub adds a, Up b, Average (a + b) >> 1 in more than 8 bits, Paeth its predictor with the tie order a, b, c; every
 * sum modulo 256.  Integers only, no atomics: the bytes do not depend on the launch or on `bands`.
 * bands: NULL (n_bands 0): one wave per frame.  Otherwise int32 (n_bands, 3) rows [frame, row0, row1): one wave per band,
 * which decodes rows row0 .. row1-1 taking the row above row0 as zero -- so a band must start at row 0 or at a row of
 * filter type 0 or 1, which do not read the row above (the caller reads the filter bytes; refid_amd.png.find_bands), and
 * the bands must cover every row once.  A band outside the frame set is skipped.  A filter byte above 4 adds nothing (as
 * type 0); callers reject such files on the host.  No row alignment is assumed (the pitch is odd for RGB).
 * width*channels <= REFID_PNG_MAX_ROW_BYTES (the LDS line that carries a block's last row to the next block): wider files
 * are decoded on the host.  One launch on `stream`; nothing is allocated, nothing synchronises.
 * ---------------------------------------------------------------------------------- */
#define REFID_PNG_MAX_ROW_BYTES 32760
typedef struct refid_png_unfilter_desc {
    const uint8_t* rows;                        /* device: n_frames * height * (1 + width*channels) bytes          */
    uint8_t* frames;                            /* device: (n_frames, height, width, 3)                            */
    const int32_t* bands;                       /* device or NULL: (n_bands, 3) = frame, row0, row1                */
    int32_t n_bands, n_frames, height, width, channels;   /* n_bands 0 with bands NULL; channels: 1 or 3          */
} refid_png_unfilter_desc;
int refid_png_unfilter(const refid_png_unfilter_desc* d, void* stream);

/* ------------------------------------------------------------------------------------
 * PNG forward filtering of resident frames (csrc/png_filter.hip): the encoder's half of the section above.  frames: uint8
 * (n_frames, height, width, 3), contiguous; rows: n_frames * height rows of 1 + 3*width bytes back to back, the filter
 * type first, then the filtered bytes -- the layout refid_png_unfilter reads, and what deflate takes as it stands.
 * Per byte a = the byte 3 to the left, b = the byte above, c = the byte above-left, each 0 outside the frame (row 0 of a
 * frame never reads the frame before); type 0 x, 1 x - a, 2 x - b, 3 x - ((a + b) >> 1), 4 x - Paeth(a, b, c) with the tie
 * order a, b, c; every residual modulo 256.  mode 0..4 puts that type on every row; REFID_PNG_FILTER_ADAPTIVE chooses per
 * row the type with the least sum of |residual read as int8| (libpng's heuristic), the lowest type on a tie.  costs: NULL,
 * or uint32 (n_frames, height, 5): the five sums of every row, in every mode.  Integers only, no atomics: the bytes do not
 * depend on n_frames, on a frame's position in the call or on the alignment of `rows` (none is assumed; costs: 4 bytes).
 * Nothing outside [rows, rows + n_frames*height*(1 + 3*width)) is written.  width <= REFID_PNG_FILTER_MAX_WIDTH, where a
 * row's sum still fits uint32: the kernel itself has no row limit.  One launch on `stream`; nothing is allocated, nothing
 * synchronises.  A bad argument returns 1 with a message (refid_last_error) and launches nothing.
 * ---------------------------------------------------------------------------------- */
#define REFID_PNG_FILTER_ADAPTIVE 5
#define REFID_PNG_FILTER_MAX_WIDTH 11184810
typedef struct refid_png_filter_desc {
    const uint8_t* frames;                      /* device: (n_frames, height, width, 3)                            */
    uint8_t* rows;                              /* device: n_frames * height * (1 + 3*width) bytes                 */
    uint32_t* costs;                            /* device or NULL: (n_frames, height, 5)                           */
    int32_t n_frames, height, width, mode;      /* mode: 0..4 or REFID_PNG_FILTER_ADAPTIVE                          */
} refid_png_filter_desc;
int refid_png_filter(const refid_png_filter_desc* d, void* stream);

/* ------------------------------------------------------------------------------------
 * Huffman-only deflate of filtered rows (csrc/png_deflate.hip): the last stage of the PNG writer.  src: n_streams runs of
 * stream_bytes bytes back to back (per frame the height * (1 + 3*width) bytes refid_png_filter writes); stream s becomes
 * ONE zlib stream at out + s*out_pitch, its length in lens[s]:
 *   78 01 | one byte-aligned segment per block of block_bytes input bytes (the last may be shorter) | 01 00 00 FF FF (a final
 *   empty stored block) | Adler-32 of the stream's input, big-endian.
 * A DYNAMIC segment (RFC 1951 3.2.7): BFINAL 0, BTYPE 10; HLIT 0 (257 literal/length codes), HDIST 0 (one distance code),
 * HCLEN 15; the 19 code-length-code lengths in the RFC's order, 0 for the symbols 16 17 18 and 4 for 0..15 (a complete code
 * without run lengths: the 4-bit code of a length is the length); 257 lengths and one distance length 0 as those codes; the
 * block's bytes as canonical Huffman codes; the end-of-block code; an empty stored block 000, padding to a byte, 00 00 FF FF.
 * A STORED segment: 00, LEN, ~LEN, the bytes; used exactly when the dynamic one would take >= len + 5 bytes.
 * The code of a block: frequencies of its bytes and 1 for end-of-block; the occurring symbols sorted by (frequency, symbol);
 * two-queue merge, the leaf queue winning a tie; depths from the root down, each one more than its parent's clamped depth,
 * a depth above 15 clamped and counted (merged nodes too); zlib's gen_bitlen repair on the counts per length; the counts
 * dealt out longest first in the sorted order; canonical code values.  tests/deflate_ref.py restates all of it in numpy.
 * Integers only; the only atomics are integer adds / ors in LDS, whose result does not depend on the order: bytes
 * [0, lens[s]) of a stream do not depend on n_streams, on the stream's position in the call, on the alignment of src or
 * out, or on the run.  Bytes [lens[s], out_pitch) are left as they were.  Nothing outside [out, out + n_streams*out_pitch),
 * lens[0 .. n_streams) and the first refid_png_deflate_work_bytes(...) bytes of work is written.
 * Three launches on `stream` that meet only at the kernel boundaries -- per block: histogram, Adler sums, code, segment
 * length; per stream: segment offsets, 78 01, terminator, Adler-32, lens; per block: the bits -- nothing is allocated,
 * nothing synchronises.  out_pitch >= refid_png_deflate_bound(stream_bytes, block_bytes) = 2 + stream_bytes + 5*blocks + 9,
 * which must fit int32; block_bytes 1 .. 65535 (REFID_PNG_DEFLATE_BLOCK: the measured default); lens and work aligned to 4
 * bytes.  A bad argument returns 1 with a message (refid_last_error) and launches nothing; the two size functions return 0
 * for sizes the entry point would turn down.
 * ---------------------------------------------------------------------------------- */
#define REFID_PNG_DEFLATE_BLOCK 32768
#define REFID_PNG_DEFLATE_MAX_BLOCK 65535
#define REFID_PNG_DEFLATE_RECORD 1088           /* scratch bytes per block: segment length / kind, Adler sums, offset, 257 codes */
typedef struct refid_png_deflate_desc {
    const uint8_t* src;                         /* device: n_streams * stream_bytes bytes                          */
    uint8_t* out;                               /* device: n_streams * out_pitch bytes                             */
    uint32_t* lens;                             /* device: [n_streams], the streams' lengths                       */
    uint32_t* work;                             /* device: refid_png_deflate_work_bytes(...) bytes of scratch      */
    int32_t n_streams, stream_bytes, block_bytes, out_pitch;
} refid_png_deflate_desc;
size_t refid_png_deflate_bound(int32_t stream_bytes, int32_t block_bytes);
size_t refid_png_deflate_work_bytes(int32_t n_streams, int32_t stream_bytes, int32_t block_bytes);
int refid_png_deflate(const refid_png_deflate_desc* d, void* stream);

/* ------------------------------------------------------------------------------------
 * Full-reference scores of uint8 frames that are already on the device (csrc/score.hip): what calculate_psnr and
 * calculate_ssim of basicsr/metrics/psnr_ssim.py do with crop_border and test_y_channel, per frame.
 * a_u8, b_u8: (n_frames, h, w, 3) uint8 HWC -- RGB, or BGR with REFID_SCORE_BGR -- the layout refid_val_tail writes and
 * refid_png_unfilter produces.  Both are cropped by crop_border on every side first: hc = h - 2cb, wc = w - 2cb; every
 * clamp below is to the cropped frame.  Each of the four outputs may be NULL; its work is then skipped.
 *   sq_rgb[f]  sum (a - b)^2 over the cropped frame and its 3 channels, an exact integer (calculate_psnr's numerator)
 *   sq_y[f]    sum in float64 of e = fl32(d * d), d = fl32(Ya - Yb), Y the float32 BT.601 plane of the NIQE section above
 *              (csrc/y_plane.h, one body for both): the float32 (img1 - img2)**2 of calculate_psnr(test_y_channel=True)
 *   ssim3d[f]  the sum refid_ssim3d_u8 gives for the cropped frames as float32 u8/255 planes R, G, B, bit for bit
 *              (csrc/ssim3d_tile.h, one body for the three kernels)
 *   ssim_y[f]  the sum of _ssim_cly's map in float64: the window is outer(g, g) of the 11-tap sigma-1.5 Gaussian in float64
 *              (closed form, normalised by its sum; computed on the host); the five fields Y1, Y2, Y1^2, Y2^2, Y1*Y2 (products
 *              exact in float64) are each the 121-tap sum acc = acc + w * x in row-major tap order from a zero accumulator,
 *              coordinates clamped (BORDER_REPLICATE); then ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2))
 *              with C1 = (0.01*255)^2, C2 = (0.03*255)^2 in the reference's operation order.  Divide by hc*wc for the mean.
 * Every step of sq_y and ssim_y is one correctly rounded operation without contraction.  Each sum is a fixed tree per
 * 16x16 tile (xor-shuffle inside a wave, then the waves in order), the tiles' partials [frame][tile row][tile column] are
 * finished in a fixed order: no atomics, and the bits do not depend on the run, on n_frames or on the frame's place in the call.
 * parts: refid_score_u8_parts(...) 8-byte words of scratch (0 for arguments the entry point turns down).  ya_out
 * (n_frames, hc, wc) float32 = Y of a, ssim_y_map_out (n_frames, hc, wc) float64 = the map: test taps, each may be NULL
 * (the map needs ssim_y).  The frames are read as aligned 4-byte words that hold at least one of their bytes, so up to 3
 * bytes either side of a buffer are read (never used); such a word lies in the page of that byte.
 * NULL frames or parts, unknown flags, crop_border < 0, hc < 1 or wc < 1, more than 2^31 - 1 tiles or frame bytes: returns 1
 * with a message (refid_last_error) and launches nothing.  One kernel for the colour outputs, one for the Y outputs and
 * one row sum per output, each only when asked for: at most six launches on `stream`; nothing is allocated.
 * ---------------------------------------------------------------------------------- */
#define REFID_SCORE_BGR 1
long long refid_score_u8_parts(int n_frames, int h, int w, int crop_border);
int refid_score_u8(const unsigned char* a_u8, const unsigned char* b_u8, int n_frames, int h, int w, int flags,
                   int crop_border, unsigned long long* sq_rgb, double* sq_y, double* ssim3d, double* ssim_y,
                   void* parts, float* ya_out, double* ssim_y_map_out, void* stream);

/* ------------------------------------------------------------------------------------
 * Baseline JPEG frames for Motion-JPEG video (csrc/jpeg.hip).  frames: (n_frames, height, width, 3) uint8 RGB, contiguous,
 * what refid_val_tail writes; frame k becomes ONE baseline sequential JFIF file at out + k*out_pitch, lens[k] bytes long:
 *   SOI | APP0 "JFIF" 1.01, density 1:1 without unit, no thumbnail | DQT, one segment with table 0 (luminance) and table 1
 *   (chrominance), 8 bit, in zig-zag order | SOF0: 8 bit, height, width, components 1 2 3, Y sampling 2x2 (REFID_JPEG_420) or
 *   1x1 (REFID_JPEG_444) on table 0, Cb and Cr 1x1 on table 1 | DHT x4 in the order DC0 AC0 DC1 AC1: the typical tables
 *   K.3 .. K.6 of ITU-T T.81 Annex K, unchanged | DRI | SOS: interleaved, Y on DC0/AC0, Cb and Cr on DC1/AC1, Ss 0, Se 63,
 *   Ah/Al 0 | the entropy-coded segments, RSTm in front of every segment but the first (m = 0 1 .. 7 0 ..) | EOI.
 * These REFID_JPEG_HEADER_BYTES = 625 bytes in front of the first segment do not depend on the frame's content.
 * Colour: JFIF full-range BT.601 in 16-bit fixed point, per pixel
 *   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *   Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16        (8421375 = (128 << 16) + 32767)
 *   Cr = ( 32768 R - 27439 G -  5329 B + 8421375) >> 16
 * A frame that does not fill its last MCU column or row (MCU: 16x16 pixels for 420, 8x8 for 444) is extended by replicating
 * its last column and row: pixel (y, x) of the extension is pixel (min(y, height-1), min(x, width-1)); no read leaves the
 * frame.  420 chroma: the rounded mean (a + b + c + d + 2) >> 2 of the Cb (Cr) of each 2x2 pixels of the extended frame.
 * DCT: s = sample - 128; with T[u][k] = round(2^14 a(u) cos((2k+1) u pi / 16)), a(0) = sqrt(1/8), a(u) = 1/2, rounded half
 * away from zero:  r[y][u] = (sum_k s[y][k] T[u][k] + 128) >> 8 (arithmetic shift), then F[v][u] = sum_k r[k][u] T[v][k], which
 * is 2^20 times the orthonormal coefficient; F[0][0] is instead the exact (sum of the 64 s) << 17, so that a flat block
 * quantises as its mean does, ties included (its AC terms are exactly 0: every row u > 0 of T sums to 0).  Quantisation: the Annex K tables K.1 / K.2 scaled as libjpeg does, s = 5000/q
 * (integer division) for quality q < 50, else 200 - 2q; entry Q = clamp((base*s + 50)/100, 1, 255); the quantised coefficient
 * is sign(F) * (((|F| + (Q << 19)) >> 20) / Q): F / (2^20 Q) rounded half away from zero (|F| + (Q << 19) < 2^31).
 * Entropy coding (T.81 F.1.2): DC difference to the previous block of the same component, predictor 0 at every segment
 * start, as category and bits; AC in zig-zag order as run/size, ZRL for runs over 15, EOB unless coefficient 63 is
 * non-zero; every FF byte followed by 00; every segment padded to a byte with 1-bits.  A segment is restart_mcus MCUs
 * (1 .. 65535; 0: the MCUs of one MCU row; the frame's last segment may be shorter).  tests/jpeg_ref.py restates all of it.
 * Integers only; the only atomics are integer adds / ors in LDS, whose result does not depend on the order: bytes
 * [0, lens[k]) of a frame do not depend on n_frames, on the frame's place in the call, on the alignment of frames or out,
 * or on the run.
 * Three launches on `stream` that meet only at the kernel boundaries -- per segment: coefficients, codes, the unstuffed
 * bits parked in `work`, the stuffed length; per frame: segment offsets, the header, EOI, lens; per segment: RSTm and the
 * stuffed bytes into place -- nothing is allocated, nothing synchronises.
 * refid_jpeg_bound(height, width, subsampling, restart_mcus) is a length every frame of that geometry fits, whatever its
 * content and quality: a block costs at most REFID_JPEG_BLOCK_BITS = 1660 bits (DC: an 11-bit code of table K.4 and 11 bits;
 * each of 63 AC coefficients a 16-bit code and 10 bits, no EOB), a segment of b blocks ceil(1660 b / 8) bytes before
 * stuffing, at most every byte is FF and doubles, and every segment but the first has its 2-byte RSTm in front:
 *   bound = 625 + sum over segments of 2 * ceil(1660 * blocks / 8) + 2 * (segments - 1) + 2.
 * out_pitch may be smaller, down to 627 (header and EOI): a frame whose file does not fit gets lens[k] = -(bytes needed),
 * its slot may hold anything and nothing outside the slot is written.  Bytes [lens[k], out_pitch) of a slot that fitted are
 * left as they were.  Nothing outside [out, out + n_frames*out_pitch), lens[0 .. n_frames) and the first
 * refid_jpeg_work_bytes(...) bytes of work is written: per segment a 16-byte record and room for its unstuffed bytes,
 *   work_bytes = n_frames * segments * (16 + round_up(ceil(1660 * blocks of the largest segment / 8), 4)).
 * height, width 1 .. 65535; quality 1 .. 100; lens and work aligned to 4 bytes; the bound and n_frames * segments must fit
 * int32.  A bad argument returns 1 with a message (refid_last_error) and launches nothing; the size functions return 0 for
 * what the entry point would turn down.
 * ---------------------------------------------------------------------------------- */
#define REFID_JPEG_444 0
#define REFID_JPEG_420 1
#define REFID_JPEG_HEADER_BYTES 625
#define REFID_JPEG_BLOCK_BITS 1660
typedef struct refid_jpeg_desc {
    const uint8_t* frames;                      /* device: n_frames * height * width * 3 bytes, RGB                */
    uint8_t* out;                               /* device: n_frames * out_pitch bytes                              */
    int32_t* lens;                              /* device: [n_frames], the files' lengths, or -(bytes needed)      */
    uint32_t* work;                             /* device: refid_jpeg_work_bytes(...) bytes of scratch             */
    int32_t n_frames, height, width, quality, subsampling, restart_mcus, out_pitch;
} refid_jpeg_desc;
int refid_jpeg_encode(const refid_jpeg_desc* d, void* stream);
size_t refid_jpeg_header_bytes(void);
size_t refid_jpeg_bound(int32_t height, int32_t width, int32_t subsampling, int32_t restart_mcus);
size_t refid_jpeg_work_bytes(int32_t n_frames, int32_t height, int32_t width, int32_t subsampling, int32_t restart_mcus);

/* ----------------------------------------------------------------------------------
 * Baseline JPEG decode (csrc/jpeg_entropy.h on the host, csrc/jpeg_decode.hip on the device): JPEG key frames and the
 * frames of a Motion-JPEG AVI -> (n_frames, height, width, 3) uint8 RGB.  The serial entropy stage runs on the host
 * (refid_jpeg_probe, refid_jpeg_entropy_decode: no GPU call, no allocation that outlives the call, safe from several threads
 * at once); dequantisation, IDCT, chroma upsampling and colour conversion run on the device (refid_jpeg_decode).  The
 * pixels are what libjpeg(-turbo) gives with its defaults (islow IDCT, fancy upsampling, table-based YCbCr -> RGB), which
 * is what PIL returns: integers only, compared byte for byte.  tests/jpeg_decode_ref.py restates all of it.
 *
 * Accepted files: SOF0, 8 bit, one interleaved scan (Ss 0, Se 63, Ah = Al = 0); 1 component (grey, any sampling factors:
 * REFID_JPEG_DEC_GREY) or 3 components with chroma 1x1 and luma 1x1 (REFID_JPEG_DEC_444), 2x1 (.._422) or 2x2 (.._420); any
 * DQT (8-bit tables) and DHT, in any number of segments, a later one replacing an earlier one; DRI of any value, RSTn
 * checked modulo 8; APPn, COM and other segments without meaning here are skipped; 0xFF fill bytes in front of a marker.
 * The Annex K Huffman tables K.3 .. K.6 stand in slots 0 (luminance) and 1 (chrominance) until a DHT replaces them, so a
 * file without DHT decodes, as Motion-JPEG cameras write them.  Refused, each with a message that begins "jpeg_decode:":
 * progressive, arithmetic, lossless and hierarchical frames, SOF1, a precision other than 8, 2 or 4 or more components,
 * other samplings, a scan that does not hold all components in frame order, 16-bit quantisation tables, RGB-coded files
 * (Adobe transform 0, or component ids 'R' 'G' 'B'), a table that is referenced but not defined, a Huffman code that is not
 * in its table, a DC category above 11, an AC category above 10, a DC value that leaves int16, a zero run past coefficient
 * 63, entropy data that ends (or meets a marker) before the last MCU -- nothing is padded with zeros --, bytes left over in
 * front of a restart marker, a wrong RST number, a height or width of 0, and any segment that passes the end of the file.
 * Neither function reads outside [file, file + len).
 *
 * refid_jpeg_probe fills `info`.  blocks[c] = 8x8 blocks of component c's plane padded to whole MCUs: with MCU rows R and
 * columns C (MCU = 8 h_max x 8 v_max pixels; grey: 8x8), component c holds (R v_c) x (C h_c) blocks.
 * refid_jpeg_entropy_decode turns a file down unless its header gives exactly *expect, then writes
 *   coefs  int16 [total_blocks][64]: the components back to back (Y, Cb, Cr), a component's blocks in raster order of its
 *          padded plane, a block's quantised coefficients in natural (row-major, de-zigzagged) order, DC prediction undone;
 *   quant  uint16 [components][64]: each component's quantisation table in natural order.
 * After a refusal the contents of coefs and quant are unspecified (but nothing outside them was written).
 *
 * refid_jpeg_decode: coefs (n_frames, total_blocks, 64) and quant (n_frames, components, 64) on the device, as above, one
 * set per frame (tables may differ from frame to frame) -> frames.  Two launches on `stream`, no allocation, no atomics, no
 * synchronisation; `work` is refid_jpeg_decode_work_bytes(n_frames, height, width, sampling) bytes of scratch (the
 * component planes between the launches; 0 from that function = a geometry the entry point turns down).
 *   1. x = coef * q.  IDCT: libjpeg's jpeg_idct_islow, CONST_BITS 13, PASS1_BITS 2, multipliers 2446 3196 4433 6270 7373
 *      9633 12299 15137 16069 16819 20995 25172; the column pass descales by 11, the row pass by 18, DESCALE(x, n) =
 *      (x + (1 << (n-1))) >> n (arithmetic shift); + 128, clamped to 0 .. 255.  All of it in 32-bit two's complement with
 *      wrap-around (unsigned on the device).  For coefficients an encoder can produce this equals libjpeg.
 *   2. A component plane is cropped to ceil(H v / v_max) x ceil(W h / h_max); where a neighbour is missing the edge sample
 *      stands in.  h2v1 (4:2:2), s = the chroma row: out[2i] = (3 s[i] + s[i-1] + 1) >> 2, out[2i+1] = (3 s[i] + s[i+1] + 2)
 *      >> 2, out[0] = s[0], out[2 last + 1] = s[last].  h2v2 (4:2:0): t = 3 near_row + far_row (far: the row above for the
 *      upper output row, below for the lower); out[2i] = (3 t[i] + t[i-1] + 8) >> 4, out[2i+1] = (3 t[i] + t[i+1] + 7) >> 4,
 *      out[0] = (4 t[0] + 8) >> 4, out[2 last + 1] = (4 t[last] + 7) >> 4.  A chroma plane of at most 2 columns is
 *      replicated instead (as libjpeg does).
 *   3. F(x) = int(x 65536 + 0.5), cb -= 128, cr -= 128: R = Y + ((F(1.402) cr + 32768) >> 16), B = Y + ((F(1.772) cb + 32768)
 *      >> 16), G = Y + ((-F(0.34414) cb + 32768 - F(0.71414) cr) >> 16), each clamped; grey: R = G = B = Y.
 * Only the n_frames * height * width * 3 bytes of `frames` are written (any alignment; rows whose first byte is 4-aligned
 * are stored as whole dwords, other rows byte by byte); a frame's bytes do not depend on n_frames, on its position or on
 * the alignment.  height, width 1 .. 65535; n_frames 1 .. 65535; coefs and work aligned to 16 bytes, quant to 2.  A bad
 * descriptor returns 1 with a message naming the field and launches nothing.
 * ---------------------------------------------------------------------------------- */
#define REFID_JPEG_DEC_GREY 0
#define REFID_JPEG_DEC_444 1
#define REFID_JPEG_DEC_422 2
#define REFID_JPEG_DEC_420 3
typedef struct refid_jpeg_info {
    int32_t height, width, components, sampling;
    int32_t blocks[3];                          /* per component (0 for the components a grey file lacks)          */
    int32_t total_blocks, restart_interval;     /* restart_interval in MCUs, 0 = none                              */
} refid_jpeg_info;
int refid_jpeg_probe(const uint8_t* file, size_t len, refid_jpeg_info* info);
int refid_jpeg_entropy_decode(const uint8_t* file, size_t len, const refid_jpeg_info* expect, int16_t* coefs, uint16_t* quant);
typedef struct refid_jpeg_decode_desc {
    const int16_t* coefs;                       /* device: n_frames * total_blocks * 64                            */
    const uint16_t* quant;                      /* device: n_frames * components * 64                              */
    uint8_t* frames;                            /* device: n_frames * height * width * 3 bytes, RGB                */
    uint8_t* work;                              /* device: refid_jpeg_decode_work_bytes(...) bytes of scratch      */
    int32_t n_frames, height, width, sampling;
} refid_jpeg_decode_desc;
int refid_jpeg_decode(const refid_jpeg_decode_desc* d, void* stream);
size_t refid_jpeg_decode_work_bytes(int32_t n_frames, int32_t height, int32_t width, int32_t sampling);
/* blocks of one frame: fills blocks[3], returns their sum (0 for a geometry that is turned down) */
int32_t refid_jpeg_decode_blocks(int32_t height, int32_t width, int32_t sampling, int32_t* blocks);

/* ----------------------------------------------------------------------------------
 * Simulated events (csrc/event_sim.hip): high-frame-rate uint8 frames -> the float32 (E, 4) rows [t, x, y, p] every event
 * route takes, by the ESIM contrast-threshold model: a reference level per pixel in log intensity, an event at each
 * threshold crossing, its time interpolated linearly between the two frames.  Integers only, apart from the three float64
 * operations of the time stamp; tests/event_sim_ref.py restates all of it and the device is compared bit for bit.
 *
 * Inputs: frames uint8 (n_frames, height, width, 3), RGB or (bgr) BGR, n_frames >= 2; stamps float64 [n_frames], strictly
 * increasing; lut int32 [256]; thresholds c_pos, c_neg int32 in units of 2^-16, each one scalar or a (height, width) map;
 * state int32 (height, width), read and written.
 *   Luma   Y8 = (19595 R + 38470 G + 7471 B + 32768) >> 16 (the coefficients of csrc/jpeg.hip).
 *   Level  a = lut[Y8].  The default table (refid_amd.event_sim.default_lut) is rint(65536 ln(v / 255 + eps)) in float64 on the
 *          host, eps = 1e-3, v = 0 .. 255; its span lut[255] - lut[0] is 452773.  The table is an argument: no transcendental
 *          is evaluated on the device, and a caller may pass another monotone mapping.
 *   State  ref = the level of the pixel's last event.  RESET sets ref = lut[Y8(frame 0)].  At every frame boundary
 *          a - c_pos < ref < a + c_neg holds and is expected of a `state` that is passed in; rows from a state that breaks it
 *          are unspecified (but bounded and inside their slots, see the cap).
 *   Interval k, frame k to frame k + 1, per pixel, a = lut[Y8_k], b = lut[Y8_{k+1}], j = 0:
 *          b > a: while ref + c_pos <= b: ref += c_pos, emit p = +1 with num = ref - a, den = b - a, ++j;
 *          b < a: while ref - c_neg >= b: ref -= c_neg, emit p = -1 with num = a - ref, den = a - b, ++j;
 *          b == a: nothing.   tick = (num 2^20) / den by 64-bit integer floor division, in (0, 2^20].
 *   Time   t = fl32(t_k + (t_{k+1} - t_k) * (double(tick) 2^-20)): three float64 operations, each rounded once, no contraction.
 *   Row    [t, x, y, p] float32, p = 1.0 or -1.0.
 *   Order  ascending in (k, tick, y width + x, j); t is then non-decreasing in float32.  An event with tick = 2^20 carries
 *          t_{k+1}: under a half-open window [t_k, t_{k+1}) it belongs to the next window.
 *   Cap    at most REFID_EVENT_SIM_CAP (255) events per pixel and interval.  The entry turns down thresholds that could exceed
 *          it, (lut_max - lut_min) / c_min + 1 > 255 (refid_event_sim_min_threshold gives the least threshold a table
 *          allows: 1776 for the default table), where lut_min, lut_max and, for maps, c_min are the caller's statement about
 *          device data.  Whatever the data, the device loop ends at 255 events and sets REFID_EVENT_SIM_FLAG_OVERFLOW in the
 *          flag word; an EMIT lane stores only into its own slots and sets REFID_EVENT_SIM_FLAG_SLOTS when they do not fit
 *          (the frames changed between the passes, or `ends` is not the prefix sum of `counts`).
 *
 * refid_event_sim launches the one kernel `stage` names on `stream`; it allocates nothing and does not synchronise:
 *   RESET   reads frames (frame 0), lut; writes state.
 *   COUNT   reads frames, lut, thresholds, state; writes counts[pix] = the pixel's rows over the chunk and ADDS the rows of
 *           interval k to totals[k] (k < n_frames - 1) and ORs flags into totals[n_frames - 1]: zero `totals` first.
 *   EMIT    reads the same and `ends` (the inclusive prefix sum of counts, int64), n_rows = ends[last]; writes the pixel's
 *           rows to rows[ends[pix - 1] .. ends[pix]) in (k, j) order, one 16-byte store each, and the row's key
 *           k << 54 | tick << 33 | pix << 8 | j to `keys`; writes state; ORs flags into totals[n_frames - 1].
 *   GATHER  sorted[i] = rows[perm[i]], i < n_rows (perm: the permutation that sorts `keys`; the keys are unique, so it does
 *           not depend on the sorting algorithm).
 * Between COUNT and EMIT the caller reads the totals and the flag (one synchronisation).  Turned down with return 1 and a
 * message that begins "event_sim:" and names the field, before any launch: a null or misaligned pointer (rows and sorted 16
 * bytes; stamps_dev, totals, ends, keys, perm 8; the int32 arrays 4; frames any), n_frames < 2 or above
 * REFID_EVENT_SIM_MAX_FRAMES (the key's 9 bits of k), height width above REFID_EVENT_SIM_MAX_PIXELS (its 25 bits of pix),
 * a scalar threshold or c_min below 1, the cap condition, stamps that are not finite and strictly increasing, n_rows outside
 * 1 .. 2^31 - 1 (use a smaller chunk).
 * ---------------------------------------------------------------------------------- */
#define REFID_EVENT_SIM_RESET 1
#define REFID_EVENT_SIM_COUNT 2
#define REFID_EVENT_SIM_EMIT 4
#define REFID_EVENT_SIM_GATHER 8
#define REFID_EVENT_SIM_CAP 255
#define REFID_EVENT_SIM_MAX_FRAMES 512
#define REFID_EVENT_SIM_MAX_PIXELS 33554432
#define REFID_EVENT_SIM_FLAG_OVERFLOW 1
#define REFID_EVENT_SIM_FLAG_SLOTS 2
typedef struct refid_event_sim_desc {
    const uint8_t* frames;                      /* device: n_frames * height * width * 3 bytes                      */
    const double* stamps_host;                  /* host:   n_frames stamps (checked here)                           */
    const double* stamps_dev;                   /* device: the same stamps (read by EMIT)                           */
    const int32_t* lut;                         /* device: 256 levels                                               */
    const int32_t* c_pos_map;                   /* device: (height, width) thresholds, or null: the scalar c_pos    */
    const int32_t* c_neg_map;                   /* device: (height, width) thresholds, or null: the scalar c_neg    */
    int32_t* state;                             /* device: (height, width) reference levels                         */
    int32_t* counts;                            /* device: (height, width) rows per pixel (COUNT writes)            */
    int64_t* totals;                            /* device: n_frames words: rows per interval, then the flag word    */
    const int64_t* ends;                        /* device: (height, width) inclusive prefix sum of counts (EMIT)    */
    float* rows;                                /* device: n_rows * 4, in pixel order (EMIT writes, GATHER reads)   */
    int64_t* keys;                              /* device: n_rows sort keys (EMIT writes)                           */
    const int64_t* perm;                        /* device: n_rows indices into rows (GATHER)                        */
    float* sorted;                              /* device: n_rows * 4, the result (GATHER writes)                   */
    int64_t n_rows;
    int32_t n_frames, height, width, bgr;
    int32_t c_pos, c_neg;                       /* scalar thresholds, units of 2^-16 (used where the map is null)   */
    int32_t c_min;                              /* the maps' smallest value (read only when a map is given)         */
    int32_t lut_min, lut_max;                   /* the table's smallest and largest level                           */
    int32_t stage;                              /* one of REFID_EVENT_SIM_RESET, _COUNT, _EMIT, _GATHER             */
} refid_event_sim_desc;
int refid_event_sim(const refid_event_sim_desc* d, void* stream);
/* the least threshold the cap allows for a table with these extremes (0: lut_max < lut_min, or none fits int32) */
int32_t refid_event_sim_min_threshold(int32_t lut_min, int32_t lut_max);

/* ----------------------------------------------------------------------------------
 * Blur synthesis (csrc/blur_synth.hip): blurry key frames as averages of consecutive frames of a high-frame-rate clip, what
 * GoPro's blur/ (plain) and blur_gamma/ (response) directories hold.  Integers only; tests/blur_ref.py restates it and the
 * device is compared bit for bit.
 *
 * Inputs: frames uint8 (n_frames, height, width, 3), contiguous, any alignment; windows int32 (n_windows, 2), rows
 * [first, count] with 1 <= count <= REFID_BLUR_MAX_COUNT and first + count <= n_frames, which may overlap or repeat, on
 * the host (checked here) and on the device (read by the kernel); to_linear uint32 [256], L, on both sides, or null on both.
 * Output: out uint8 (n_windows, height, width, 3), any alignment; nothing outside it is written.  Per byte b of a frame
 * (the channels are independent, so RGB and BGR frames are treated alike):
 *   plain      out = (sum_j f[first+j][b] + count/2) / count                       integer division: ties round up
 *   response   v = (sum_j L[f[first+j][b]] + count/2) / count, out = the number of c in 1 .. 255 with thr[c] <= v,
 *              thr[c] = (L[c-1] + L[c] + 1) >> 1: the code whose level is nearest to the average in linear light.
 * L must be strictly increasing with L[255] <= 2^24 (a sum of 64 entries then stays below 2^31);
 * refid_amd.blur_synth.gamma_table(g) is rint(2^24 (c / 255)^g) in float64 on the host.  Since thr[c] <= L[c] < thr[c+1],
 * a window of identical frames returns that frame exactly, in both modes and for every count.
 *
 * One launch for all windows on `stream`; allocates nothing, does not synchronise.  The grid is capped (4096 workgroups
 * that walk the tiles with a stride; max_groups > 0 lowers or raises the cap, 0 keeps it).  Turned down with return 1 and a
 * message that begins "blur_synth:" and names the field, before any launch: a null pointer, a table pointer that is not
 * aligned to 4 bytes, one copy of to_linear without the other, n_windows, height, width or n_frames below 1, a negative
 * max_groups, a count outside 1 .. 64, a window outside the frames, a table that is not strictly increasing (the first
 * such index is named) or whose last entry exceeds 2^24, more than 2^40 pixels per frame or 2^31 - 1 tiles (4096 bytes of
 * one window each) per call.
 * ---------------------------------------------------------------------------------- */
#define REFID_BLUR_MAX_COUNT 64
typedef struct refid_blur_synth_desc {
    const uint8_t* frames;                      /* device: n_frames * height * width * 3 bytes                      */
    const int32_t* windows_host;                /* host:   n_windows rows [first, count] (checked here)              */
    const int32_t* windows;                     /* device: the same rows (read by the kernel)                       */
    const uint32_t* to_linear_host;             /* host:   256 levels (checked here), or null: plain mode           */
    const uint32_t* to_linear;                  /* device: the same levels, or null                                 */
    uint8_t* out;                               /* device: n_windows * height * width * 3 bytes                     */
    int32_t n_frames, height, width, n_windows;
    int32_t max_groups;                         /* 0: the default cap of the grid; else the cap, in workgroups      */
} refid_blur_synth_desc;
int refid_blur_synth(const refid_blur_synth_desc* d, void* stream);

/* ----------------------------------------------------------------------------------
 * Double integral (csrc/edi.hip): latent sharp frames from key frames and events without a network, the event-based double
 * integral of Pan et al. (CVPR 2019) and the model-based inverse of "Simulated events" + "Blur synthesis".  A pixel's log
 * level moves by +c_pos or -c_neg per event, so the latent frame at an instant is the key frame times exp(level) divided by
 * the mean of exp(level) over the key's exposure.  tests/edi_ref.py restates it and the device is compared bit for bit.
 *
 * Inputs.  frames uint8 (n_frames, height, width, 3), contiguous, any alignment; the three channels are treated alike.
 *   The stream, packed once per sequence (refid_amd.edi.EdiStream): the rows [t, x, y, p] of a time-sorted float32 stream
 *   with x and y truncated toward zero, rows outside the frame dropped, sorted stably by pixel y width + x:
 *   ev_t float32 [n_events] stamps, ev_p int8 [n_events] signs (p > 0: +1, anything else: -1), seg int32 [height width + 1],
 *   pixel q owns ev[seg[q] .. seg[q + 1]).  n_events may be 0 (ev_t and ev_p are then not read).
 *   Items, each on the host (checked here) and on the device (read by the kernel): items int32 (n_items, 2) rows
 *   [left, right], key-frame indices, right < 0: no right key (deblurring); bounds float32 (n_items, 4) rows
 *   [s0, e0, s1, e1], the exposures of the two keys, s0 <= e0 <= s1 <= e1 (without a right key s1 and e1 are not read);
 *   instants float32 (n_items, n_instants), ascending, inside [s0, e1] ([s0, e0] without a right key);
 *   samples float32 (n_items, 2 m) in REFID_EDI_SAMPLES mode, null on both sides in REFID_EDI_CONTINUOUS mode: m ascending
 *   instants inside [s0, e0], then m inside [s1, e1] (refid_amd.edi.sample_instants: fl32(s + ((e - s) j) / (m - 1)) in
 *   float64, m = 1: s).  tables float64 [REFID_EDI_TABLE] on the device (refid_amd.edi.gain_tables): exp(i), i = -32 .. 32 |
 *   exp(h / 256), h = 0 .. 255 | exp(l / 65536), l = 0 .. 255, built on the host: nothing transcendental runs on the device.
 *   Level  e(tau) = the sum of (p > 0 ? +c_pos : -c_neg) over the pixel's events with s0 < t <= tau, compared in float32:
 *          an exact integer in units of 2^-16 (thresholds 1 .. REFID_EDI_MAX_THRESHOLD).  An event at s0 is not the
 *          item's, one at tau counts towards tau (the simulator stamps a crossing reached at a frame with that frame).
 *   Gain   g(e): ec = e held inside +-REFID_EDI_CLAMP 2^16, ec = 65536 i + 256 h + l, g = (T0[i] T1[h]) T2[l] in float64.
 *          A pixel of an item for which some gain was held counts once in the flag words.
 *   S      of a key with exposure [s, e] and level e(s): 1 when s == e (a sharp key); SAMPLES: (sum_j g(e(sigma_j) - e(s))) / m
 *          summed in j order from 0; CONTINUOUS: (sum_k g_k (t_{k+1} - t_k)) / (e - s) over the piecewise-constant level on
 *          [s, e], its knots s, the events with s < t <= e, and e, float64 from the float32 stamps, in time order.
 *   Latent L_key(tau)[c] = ((B_key[c] + eps255) g(e(tau) - e(s_key))) / S_key, eps255 = 255 eps (the simulator's eps: 1e-3).
 *   Blend  w = 0 for tau <= e0, 1 for tau >= s1, else (tau - e0) / (s1 - e0);
 *          out = clamp(rint(((1 - w) L_left + w L_right) - eps255), 0, 255), rint to even; without a right key L_left alone.
 *   Every float64 operation is rounded once (no contraction), in the order written.
 * Output: out uint8 (n_items, n_instants, height, width, 3), any alignment; clamped int32 [n_items ceil(height width /
 * REFID_EDI_THREADS)]: every workgroup writes the count of its held pixels into its own word (no atomics); sum them.
 *
 * One launch for all items on `stream`; allocates nothing, does not synchronise.  Turned down with return 1 and a message
 * that begins "edi:" and names the field, before any launch: a null or misaligned pointer (tables 8 bytes, the int32 and
 * float arrays 4), one copy of samples without the other or samples in CONTINUOUS mode, n_items outside 1 ..
 * REFID_EDI_MAX_ITEMS, n_instants outside 1 .. REFID_EDI_MAX_INSTANTS, m outside 1 .. REFID_BLUR_MAX_COUNT, height width
 * outside 1 .. REFID_EDI_MAX_PIXELS, n_events outside 0 .. 2^31 - 1, an unknown exposure mode, a threshold outside 1 ..
 * REFID_EDI_MAX_THRESHOLD, eps255 not finite or negative, a key index outside the frames, bounds, instants or samples that
 * are not finite, not ordered or outside their range.  Nothing is retried and nothing falls back to the host.
 * ---------------------------------------------------------------------------------- */
#define REFID_EDI_SAMPLES 0
#define REFID_EDI_CONTINUOUS 1
#define REFID_EDI_THREADS 256
#define REFID_EDI_CLAMP 32
#define REFID_EDI_TABLE 577
#define REFID_EDI_MAX_INSTANTS 256
#define REFID_EDI_MAX_ITEMS 65535
#define REFID_EDI_MAX_PIXELS 33554432
#define REFID_EDI_MAX_THRESHOLD 1048576
typedef struct refid_edi_desc {
    const uint8_t* frames;                      /* device: n_frames * height * width * 3 bytes                      */
    const float* ev_t;                          /* device: n_events stamps, by pixel, then by time                  */
    const int8_t* ev_p;                         /* device: n_events signs, +1 or -1                                 */
    const int32_t* seg;                         /* device: height * width + 1 segment starts                        */
    const int32_t* items_host;                  /* host:   n_items rows [left, right] (checked here)                */
    const int32_t* items;                       /* device: the same rows                                            */
    const float* bounds_host;                   /* host:   n_items rows [s0, e0, s1, e1] (checked here)             */
    const float* bounds;                        /* device: the same rows                                            */
    const float* samples_host;                  /* host:   n_items rows of 2 m sample instants, or null             */
    const float* samples;                       /* device: the same rows, or null                                   */
    const float* instants_host;                 /* host:   n_items rows of n_instants output instants               */
    const float* instants;                      /* device: the same rows                                            */
    const double* tables;                       /* device: REFID_EDI_TABLE gains                                    */
    uint8_t* out;                               /* device: n_items * n_instants * height * width * 3 bytes          */
    int32_t* clamped;                           /* device: n_items * ceil(height width / REFID_EDI_THREADS) counts  */
    double eps255;                              /* 255 eps                                                          */
    int64_t n_events;
    int32_t n_frames, height, width, n_items, n_instants;
    int32_t m, exposure;                        /* samples per key (SAMPLES mode), REFID_EDI_SAMPLES / _CONTINUOUS  */
    int32_t c_pos, c_neg;                       /* thresholds, units of 2^-16                                       */
} refid_edi_desc;
int refid_edi(const refid_edi_desc* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* REFID_HIP_H */
