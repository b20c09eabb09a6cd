// Host-only walk of conv_wino6's plan (wino6_plan through refid_wino6_route), meant to be built with host sanitizers:
//
//   FLAGS="--offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I refid_amd/csrc"
//   for f in conv_wino conv_wino6; do hipcc $FLAGS -c refid_amd/csrc/$f.hip -o /tmp/$f.o; done
//   hipcc $FLAGS -x hip tools/probes/wino6_route_host_check.cpp -x none /tmp/conv_wino.o /tmp/conv_wino6.o -o /tmp/wino6_route_host_check
//   /tmp/wino6_route_host_check
//
// Over a sweep of geometries, split policies and wino_tile values: the in-group split (two K groups in one workgroup) is chosen
// exactly where the plan has two K ranges and wino_tile is not 5; wino_tile 5 gives wino_tile 0's tile and K ranges (the routing
// before the in-group form); no policy = no split; and the workspace size never depends on the in-group form (the byte counts
// tests/test_host_logic.py pins).  The train step's layers are named at the end.  Needs no GPU: nothing is launched.
#include "common.h"
#include "conv_args.h"

static char g_err[512];
void refid_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "line %d: %s failed (N=%d H=%d W=%d Ctot=%d Cout=%d policy=%d tile=%d)\n", \
                                           __LINE__, #c, a.N, a.Ho, a.Wo, a.Ctot, a.Cout, pol, hint); return 1; } } while (0)

static ConvKArgs geo(int n, int h, int w, int ctot, int cout) {
    ConvKArgs a{};
    a.N = n; a.H = a.Ho = h; a.W = a.Wo = w; a.Ca = a.Ctot = ctot; a.ldA = ctot; a.Cout = cout; a.CoutPad = (cout + 63) / 64 * 64;
    a.pad = 1;
    return a;
}

int main() {
    long long rows = 0, ingroup = 0, gridsplit = 0;
    int pol = 0, hint = 0;
    for (int n : {1, 2, 3, 8})
        for (int h : {4, 8, 9, 32, 64, 256})
            for (int w : {8, 32, 33, 64, 256})
                for (int ctot : {4, 16, 36, 64, 124, 128, 132, 144, 176, 252, 256, 512})
                    for (int cout : {1, 3, 20, 32, 33, 40, 64, 96, 128, 256}) {
                        ConvKArgs a = geo(n, h, w, ctot, cout);
                        for (pol = 0; pol < 3; ++pol) {
                            int r[6];
                            for (hint = 0; hint < 6; ++hint) {
                                r[hint] = refid_wino6_route(a, pol, hint);
                                const int ks = r[hint] & 255, nt = (r[hint] >> 8) & 255, kg = r[hint] >> 16;
                                ++rows;
                                EXPECT(ks >= 1 && ks <= 8 && (nt == 1 || nt == 2) && (kg == 1 || kg == 2));
                                EXPECT(pol != 0 || ks == 1);
                                EXPECT((kg == 2) == (ks == 2 && hint != 5));
                                EXPECT(nt == 1 || cout > 32);
                                EXPECT(hint != 1 || nt == (cout > 32 ? 2 : 1));
                                EXPECT(hint != 4 || nt == 1);
                                EXPECT(ks == 1 || (ctot + 15) / 16 >= 8);
                                ingroup += kg == 2;
                                gridsplit += ks > 1 && kg == 1;
                            }
                            hint = 5;
                            EXPECT((r[5] & 0xffff) == (r[0] & 0xffff));          // the parent's routing: 0's tile and K ranges
                            // the workspace covers the grid split of any wino_tile value, in-group form or not
                            size_t need = 0;
                            for (int t : {0, 1, 4}) {
                                const int ks = refid_wino6_route(a, pol, t) & 255;
                                const size_t b = refid_splitk_bytes(ks, (long long)n * h * w, cout);
                                need = b > need ? b : need;
                            }
                            EXPECT(refid_wino6_workspace_bytes(a, pol) == need);
                            EXPECT(refid_splitk_bytes(r[5] & 255, (long long)n * h * w, cout) <= need);
                        }
                    }
    // the train step's bottleneck convs at B = 8 (256 -> 256 at 32 x 32): two K ranges, in one workgroup
    {
        ConvKArgs a = geo(8, 32, 32, 256, 256);
        pol = 2; hint = 0;
        EXPECT(refid_wino6_route(a, 2, 0) == (2 | 2 << 8 | 2 << 16));
        EXPECT(refid_wino6_route(a, 2, 5) == (2 | 2 << 8 | 1 << 16));
        a = geo(8, 256, 256, 64, 32);                                              // decoder 2's trunk: never split
        EXPECT(refid_wino6_route(a, 2, 0) == (1 | 1 << 8 | 1 << 16));
        a = geo(1, 64, 64, 256, 256);                                              // B = 1, level 2: four K ranges, grid split
        EXPECT(refid_wino6_route(a, 2, 0) == (4 | 2 << 8 | 1 << 16));
        EXPECT(ingroup > 1000 && gridsplit > 1000);
    }
    printf("wino6_route_host_check: %lld plans, %lld in-group, %lld grid split, ok\n", rows, ingroup, gridsplit);
    return 0;
}
