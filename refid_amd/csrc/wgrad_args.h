// Launch scaffolding shared by the weight-gradient partial-product kernels (conv_wgrad.hip, wgrad_bf16.hip, wgrad_wino.hip,
// wgrad_wino24.hip, wgrad_pws.hip): the kernel-side argument block, its fill from a refid_wgrad_desc, the split plan, the
// 32-bit offset guard and the queue of deferred reductions.  Every one of the kernels fills the same private slabs
// [split][tap][CoP][CiP] (+ bias slabs [split][CoP]).
#pragma once

#include "common.h"
#include <cstring>
#include <vector>

struct WgArgs {
    // up to REFID_WGRAD_MAX_GROUPS time steps of the same convolution (same geometry): their tiles form one K range, the
    // slabs are read-modify-written once per group instead of once per step (refid_wgrad_desc.groups)
    const float* g[REFID_WGRAD_MAX_GROUPS]; const float* inA[REFID_WGRAD_MAX_GROUPS]; const float* inB[REFID_WGRAD_MAX_GROUPS];
    int groups;
    int ldG, Co;
    int ldA, ldB, Ca, Ctot;
    float* slabs; float* bslabs;
    int N, H, W, Ho, Wo, pad;
    int tilesX, tilesY, ntiles, nsplit;
    int CoP, CiP;
    int accum = 0;             // add into the slabs instead of overwriting them
};
struct WgKArgs : WgArgs {
    // wgrad_pws.hip only, patch form (refid_wgrad_desc.algo 8): input pixel p sits at (p / patchW) * patchRow + (p % patchW) * ld
    // floats instead of p * ld (both sources: the even / odd rows of ONE tensor); 0 = dense
    int patchW = 0, patchRow = 0;
};
// (wgrad_wino24.hip derives its W24Args from WgArgs in the same way.)  The kernels read these blocks at fixed offsets: a derived
// block's members begin in the four bytes behind `accum` (WgArgs has a default member initialiser, so its tail padding is not
// reserved), where they sat when each family had a flat struct of its own.

// Split plan of a launch: (ncoT x nciT) channel tiles of cot x cit, K tiles of th x tw gradient pixels (th = 0: runs of tw
// pixels of the whole batch, the streaming 1x1 form) divided into nsplit ranges -- as many as give `wgs` workgroups over
// `mult` grids per channel tile, a multiple of 8 where `round8` (grid x is fastest: the workgroups of one K range then stay
// on one XCD), never more than there are tiles.  refid_wgrad_workspace_bytes and the launches call this one function, so
// the workspace query and the launch agree.
struct WgSplit { int ncoT, nciT, tilesX, tilesY, ntiles, nsplit, CoP, CiP; };

static inline WgSplit refid_wgrad_split(const refid_wgrad_desc* d, int cot, int cit, int th, int tw, int wgs, bool round8,
                                        int mult = 1) {
    WgSplit g;
    g.ncoT = cdiv(d->c_o, cot);
    // stable across steps: a phased call sizes by i_total (the first recurrent step has no second source yet)
    const int ci_src = d->c_a + d->c_b, ci_geo = (d->phase != 0) ? d->i_total - d->i_base : ci_src;
    g.nciT = cdiv(ci_geo > ci_src ? ci_geo : ci_src, cit);
    g.tilesX = th ? cdiv(d->wo, tw) : 0;
    g.tilesY = th ? cdiv(d->ho, th) : 0;
    // (the streaming form keeps one split, a slab of zeros, for an empty batch)
    const long long px = ((long long)d->n * d->h * d->w + tw - 1) / tw;
    g.ntiles = th ? g.tilesX * g.tilesY * d->n : (int)(px > 1 ? px : 1);
    int want = cdiv(wgs, g.ncoT * g.nciT * mult);
    if (round8 && want >= 8) want = want / 8 * 8;
    if (want < 1) want = 1;
    if (want > g.ntiles) want = g.ntiles;
    g.nsplit = want;
    g.CoP = g.ncoT * cot;
    g.CiP = g.nciT * cit;
    return g;
}

// every byte offset into the gradient and the sources fits the kernels' signed 32-bit buffer offsets
static inline bool refid_wgrad_offsets_fit(const refid_wgrad_desc* d) {
    const long long lim = 0x7fffffffLL, gpix = (long long)d->n * d->ho * d->wo, xpix = (long long)d->n * d->h * d->w;
    return gpix * d->ld_g * 4 < lim && xpix * d->ld_a * 4 < lim && (d->c_b == 0 || xpix * d->ld_b * 4 < lim);
}

// Fills the shared block from a descriptor and its split plan (slabFloats = floats of one split's slab; the bias slabs lie
// behind the nsplit slabs).  align16: the LDS-DMA families move 16-byte pieces straight from the tensors.  0, or 1 with
// refid_set_error.
static inline int refid_wgrad_fill(WgArgs& a, const refid_wgrad_desc* d, const WgSplit& g, long long slabFloats, bool align16,
                                   const char* family) {
    const int ngrp = d->groups > 1 ? d->groups : 1;
    REFID_CHECK(ngrp <= REFID_WGRAD_MAX_GROUPS, "wgrad: at most %d grouped time steps", REFID_WGRAD_MAX_GROUPS);
    for (int k = 0; k < REFID_WGRAD_MAX_GROUPS; ++k) {
        const bool on = k > 0 && k < ngrp;                 // (the unused entries repeat the first step: always valid pointers)
        a.g[k] = on ? d->g_more[k - 1] : d->g;
        a.inA[k] = on ? d->in_a_more[k - 1] : d->in_a;
        a.inB[k] = on ? d->in_b_more[k - 1] : d->in_b;
        REFID_CHECK(a.g[k] && a.inA[k] && (d->c_b == 0 || a.inB[k]), "wgrad: null tensor pointer in group %d", k);
        REFID_CHECK(!align16 || ((uintptr_t)a.g[k] | (uintptr_t)a.inA[k] | (uintptr_t)(d->c_b ? a.inB[k] : nullptr)) % 16 == 0,
                    "wgrad (%s): tensors must be 16-byte aligned (group %d)", family, k);
    }
    a.groups = ngrp;
    a.ldG = d->ld_g; a.Co = d->c_o;
    a.ldA = d->ld_a; a.ldB = d->ld_b;
    a.Ca = d->c_a; a.Ctot = d->c_a + d->c_b;
    a.slabs = d->slabs;
    a.bslabs = d->db ? d->slabs + (size_t)g.nsplit * slabFloats : nullptr;
    a.N = d->n; a.H = d->h; a.W = d->w; a.Ho = d->ho; a.Wo = d->wo; a.pad = d->pad;
    a.tilesX = g.tilesX; a.tilesY = g.tilesY; a.ntiles = g.ntiles; a.nsplit = g.nsplit;
    a.CoP = g.CoP; a.CiP = g.CiP;
    a.accum = (d->phase == 2);
    return 0;
}

// Deferred second stage of the slab reductions (refid_wgrad_desc.phase = 4 + refid_wgrad_finish_flush): a phase-4 call runs its
// streaming fold at once and QUEUES its element-wise stage; the flush issues every queued stage of a family as ONE launch
// (the job blocks travel as kernel arguments, at most REFID_FINISH_BATCH per launch: no device table, graph-capturable).
// ~130 dependent 10-300 us launches of 1-30 workgroups per step become three or four.
constexpr int REFID_FINISH_BATCH = 40;

// One family's queue.  Job has dw and iBase; Batch is { Job job[REFID_FINISH_BATCH]; int blk0[REFID_FINISH_BATCH + 1]; int n; },
// the argument of the family's batch kernel, in which a workgroup finds its job by its block range.
template <class Job, class Batch>
struct WgFinishQueue {
    struct Queued { Job r; int nblocks; };
    std::vector<Queued> jobs;

    // Two queued jobs must not add into the same gradient block (they would run concurrently): flush_all() first.
    template <class Flush>
    int push(const Job& r, int nblocks, Flush&& flush_all) {
        for (const Queued& q : jobs)
            if (q.r.dw == r.dw && q.r.iBase == r.iBase) {
                if (int rc = flush_all()) return rc;
                break;
            }
        jobs.push_back({r, nblocks});
        return 0;
    }
    // launch(batch, workgroups) -> false when the launch failed (the queue is dropped)
    template <class Launch>
    int flush(Launch&& launch) {
        for (size_t at = 0; at < jobs.size();) {
            Batch b;
            memset(&b, 0, sizeof(b));
            int n = 0, blk = 0;
            for (; n < REFID_FINISH_BATCH && at < jobs.size(); ++n, ++at) {
                b.job[n] = jobs[at].r;
                b.blk0[n] = blk;
                blk += jobs[at].nblocks;
            }
            b.blk0[n] = blk; b.n = n;
            if (!launch(b, blk)) { jobs.clear(); return 1; }
        }
        jobs.clear();
        return 0;
    }
};

// wgrad_bf16.hip: 3x3 / stride-1 partial products with bf16 MFMA operands; geometry = the fp32 W3 plan
// (64 x 64 channel tile, 2 x 32 pixel tiles), grid (nsplit, nciT, ncoT)
int refid_wgrad_bf16_launch(const WgKArgs& a, int nciT, int ncoT, hipStream_t st);

// wgrad_wino.hip (algo 1) and wgrad_wino24.hip (algo 5: Winograd over 2x4 tiles, F(3,2) x F(3,4); algo 7: conv_down)
size_t refid_wgrad_wino_workspace_bytes(const refid_wgrad_desc* d);
int refid_wgrad_wino_launch(const refid_wgrad_desc* d, hipStream_t st);
size_t refid_wgrad_wino24_workspace_bytes(const refid_wgrad_desc* d);
int refid_wgrad_wino24_launch(const refid_wgrad_desc* d, hipStream_t st, bool defer);

// wgrad_wino24.hip: streaming first stage of a split-K slab reduction (S partial slabs out of nsplit; 0 = nothing to fold);
// defer (a phase-4 call): queued for refid_slab_fold_flush, which runs before either family's second stage
int refid_slab_fold_count(long long slabFloats, int nsplit);
int refid_launch_slab_fold(const float* slabs, float* part, long long slabFloats, int nsplit, int S, hipStream_t st, bool defer);
int refid_slab_fold_flush(hipStream_t st);
int refid_wino24_finish_flush(hipStream_t st);          // wgrad_wino24.hip: its queue of second stages

// wgrad_pws.hip: streaming 1x1 weight gradient (LDS-DMA ring, fp32 MFMA); geometry of its slabs [split][CoP][CiP]
bool refid_wgrad_pws_ok(const refid_wgrad_desc* d);
int refid_wgrad_pws_pixels_per_buffer(const refid_wgrad_desc* d);
WgSplit refid_wgrad_pws_geo(const refid_wgrad_desc* d);
int refid_wgrad_pws_launch(const refid_wgrad_desc* d, const WgKArgs& a, int nciT, int ncoT, hipStream_t st);
