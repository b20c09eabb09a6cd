// The tile walk of the wgrad_wino24 family (wgrad_wino24.hip): which K tiles a split owns and the wave-uniform cursor over them.
// The two 3x3 kernels (algo 5, four and eight waves) use it; conv_down's kernel (algo 7) still carries its own copy of the same
// walk, which is the second geometry of the parameters below.  A split walks a CONTIGUOUS range p0 .. p1 of the groups x N x tilesY x
// tilesX tiles (x fastest), and the cursor keeps, next to the tile's coordinates, the byte offsets of its first halo and
// gradient pixel: one tile width further per step (two scalar adds), recomputed only at the end of a tile row.  The tensors of
// the current time step (group) are reloaded from the argument block only when the walk crosses into the next one -- a load
// per request would put a full scalar-memory latency in front of every tile.
//
// Plain C++ on purpose: tools/probes/w24_walk_host_check.cpp includes this file as host code and walks every split range under
// ASan + UBSan.  `A` is the kernels' argument block (W24Args) or the probe's stand-in: anything with g[], inA[], inB[], groups,
// ntiles, nsplit, tilesX, tilesY, N, Ho, Wo and ldG.
#pragma once

// Timing experiment 7 of wgrad_wino24.hip (tools/probes/w24_ablate.py): the cursor never moves, so every request fetches the
// split's FIRST tile again (same instructions, same LDS writes, cache hits instead of HBM).
#ifndef REFID_W24_ABLATE
#define REFID_W24_ABLATE 0
#endif

#if defined(__HIPCC__)
#define W24_WALK_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define W24_WALK_FN inline
#endif

constexpr int W24_GW = 16;                     // gradient pixels per K tile row (four Winograd tile columns of four)

// GHT: gradient rows per K tile (4; conv_down 6).  XPS: input pixels per tile pixel (1; conv_down walks a parity phase of its
// input: 2).  (oy, ox): how far the halo starts above / left of the tile's first pixel, in tile pixels (pad; conv_down: the
// phase's parities).
template <int GHT, int XPS>
struct W24Walk {
    int p0, p1;                                // this split's tiles
    int qg, qn, qy, qx;                        // the next tile to request: group, sample, tile row, tile column
    int xTile, gTile;                          // byte offsets of its first halo / gradient pixel
    const float *gPtr, *xPtr;                  // the group's gradient and input
    int Hin, Win, xld;
    bool xFromA;

    W24_WALK_FN int x_origin(int n, int ty, int tx, int oy, int ox) const {
        return ((n * Hin + XPS * ty * GHT - oy) * Win + XPS * tx * W24_GW - ox) * xld * 4;
    }
    template <class A>
    W24_WALK_FN void load_group(const A& a) {
        gPtr = a.g[qg];
        xPtr = xFromA ? a.inA[qg] : a.inB[qg];
    }
    // the input comes from source A or B at pitch ld floats and is hin x win pixels per sample
    template <class A>
    W24_WALK_FN void init(const A& a, int split, bool fromA, int ld, int hin, int win, int oy, int ox) {
        xFromA = fromA; xld = ld; Hin = hin; Win = win;
        const int ntAll = a.ntiles * a.groups;
        const int chunk = (ntAll + a.nsplit - 1) / a.nsplit;
        p0 = split * chunk < ntAll ? split * chunk : ntAll;
        p1 = p0 + chunk < ntAll ? p0 + chunk : ntAll;
        int t = p0 < ntAll ? p0 : 0;
        qg = t / a.ntiles; t -= qg * a.ntiles;
        qx = t % a.tilesX; t /= a.tilesX;
        qy = t % a.tilesY; qn = t / a.tilesY;
        load_group(a);
        xTile = x_origin(qn, qy, qx, oy, ox);
        gTile = ((qn * a.Ho + qy * GHT) * a.Wo + qx * W24_GW) * a.ldG * 4;
    }
    // (behind the last tile of the last group the cursor wraps to that group's first tile: always valid pointers)
    template <class A>
    W24_WALK_FN void advance(const A& a, int oy, int ox) {
        if (REFID_W24_ABLATE == 7) return;
        qx += 1;
        if (qx != a.tilesX) {
            xTile += W24_GW * XPS * xld * 4;
            gTile += W24_GW * a.ldG * 4;
            return;
        }
        qx = 0;
        qy += 1;
        if (qy == a.tilesY) {
            qy = 0;
            qn += 1;
            if (qn == a.N) {
                qn = 0;
                qg = qg + 1 < a.groups - 1 ? qg + 1 : a.groups - 1;
                load_group(a);
            }
        }
        xTile = x_origin(qn, qy, 0, oy, ox);
        gTile = (qn * a.Ho + qy * GHT) * a.Wo * a.ldG * 4;
    }
};
