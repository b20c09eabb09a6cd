// Host-only walk of the wgrad_wino24 family's tile cursor (refid_amd/csrc/wgrad_w24_walk.h), meant to be built with host
// sanitizers:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I refid_amd/csrc \
//         -x hip tools/probes/w24_walk_host_check.cpp -o /tmp/w24_walk_host_check
//   /tmp/w24_walk_host_check
//
// (The header is plain C++: `c++ -std=c++17 -fsanitize=address,undefined -I refid_amd/csrc` builds the same program.)
//
// For both geometries of the family -- the 3x3 / pad-1 kernels (4-row K tiles of the image itself) and conv_down's four parity
// phases (6-row K tiles, two input pixels per tile pixel) -- every split range of every plan is walked by advance(), as the
// kernels do after each request: outputs of 12x40, 7x21 and 6x10 pixels (partial tiles on both axes), N in {1, 2}, 1 and 3
// grouped time steps, both sources, nsplit from 1 to more than there are tiles (empty ranges).  At every tile the cursor, both
// byte offsets and both tensors must equal what the tile's index gives directly, and all ranges together must visit every
// tile of every group exactly once.  Needs no GPU.
#include "wgrad_w24_walk.h"
#include <cstdio>
#include <vector>

struct Args {                                  // the members of W24Args the walk reads
    const float* g[8]; const float* inA[8]; const float* inB[8];
    int groups, ldG, N, Ho, Wo, tilesX, tilesY, ntiles, nsplit;
};

#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "line %d: %s failed (%s, %dx%d N %d groups %d nsplit %d split %d tile %d)\n", \
                                           __LINE__, #c, what, Ho, Wo, N, groups, a.nsplit, split, t); return 1; } } while (0)

// GHT x 16 K tiles of an Ho x Wo gradient; the input is Hin x Win at XPS pixels per tile pixel, halo origin (oy, ox)
template <int GHT, int XPS>
static int walk_all(const char* what, int Ho, int Wo, int Hin, int Win, int oy, int ox, long long& tiles_walked) {
    static float tensors[3 * 8];               // distinct addresses; never dereferenced
    for (int N = 1; N <= 2; ++N)
        for (int groups = 1; groups <= 3; groups += 2)
            for (int fromA = 0; fromA < 2; ++fromA) {
                Args a{};
                for (int k = 0; k < 8; ++k) { a.g[k] = tensors + k; a.inA[k] = tensors + 8 + k; a.inB[k] = tensors + 16 + k; }
                a.groups = groups; a.ldG = 40; a.N = N; a.Ho = Ho; a.Wo = Wo;
                a.tilesX = (Wo + W24_GW - 1) / W24_GW; a.tilesY = (Ho + GHT - 1) / GHT;
                a.ntiles = a.tilesX * a.tilesY * N;
                const int ntAll = a.ntiles * groups, xld = fromA ? 72 : 136;
                for (a.nsplit = 1; a.nsplit <= ntAll + 3; ++a.nsplit) {
                    std::vector<int> seen(ntAll, 0);
                    int prev_end = 0, split = 0, t = 0;
                    for (; split < a.nsplit; ++split) {
                        W24Walk<GHT, XPS> w;
                        w.init(a, split, fromA != 0, xld, Hin, Win, oy, ox);
                        EXPECT(w.p0 == prev_end && w.p0 <= w.p1 && w.p1 <= ntAll);
                        prev_end = w.p1;
                        for (t = w.p0; t < w.p1; ++t) {
                            const int g = t / a.ntiles, r = t % a.ntiles;
                            const int n = r / (a.tilesX * a.tilesY), ty = r / a.tilesX % a.tilesY, tx = r % a.tilesX;
                            EXPECT(w.qg == g && w.qn == n && w.qy == ty && w.qx == tx);
                            // first halo pixel: tile pixel (ty GHT - oy, tx 16 - ox) -> input pixel XPS x that, + the phase
                            const int iy = XPS * (ty * GHT - oy) + (XPS - 1) * oy, ix = XPS * (tx * W24_GW - ox) + (XPS - 1) * ox;
                            EXPECT(w.xTile == ((n * Hin + iy) * Win + ix) * xld * 4);
                            EXPECT(w.gTile == ((n * Ho + ty * GHT) * Wo + tx * W24_GW) * a.ldG * 4);
                            EXPECT(w.gPtr == a.g[g] && w.xPtr == (fromA ? a.inA[g] : a.inB[g]));
                            ++seen[t];
                            ++tiles_walked;
                            w.advance(a, oy, ox);      // (also behind the range's last tile, as the kernels do)
                            EXPECT(w.qg >= 0 && w.qg < groups && w.qn >= 0 && w.qn < N);
                        }
                    }
                    EXPECT(prev_end == ntAll);
                    for (t = 0; t < ntAll; ++t) EXPECT(seen[t] == 1);
                }
            }
    return 0;
}

int main() {
    const int sizes[3][2] = {{12, 40}, {7, 21}, {6, 10}};
    long long tiles = 0;
    for (const auto& s : sizes) {
        const int Ho = s[0], Wo = s[1];
        if (walk_all<4, 1>("3x3 pad 1", Ho, Wo, Ho, Wo, 1, 1, tiles)) return 1;
        for (int phase = 0; phase < 4; ++phase)
            if (walk_all<6, 2>("conv_down phase", Ho, Wo, 2 * Ho, 2 * Wo, phase >> 1, phase & 1, tiles)) return 1;
    }
    printf("w24_walk_host_check: %lld tiles walked, ok\n", tiles);
    return 0;
}
