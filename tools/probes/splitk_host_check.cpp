// Host-only walk of the conv tiles' split-K arithmetic, meant to be built with host sanitizers:
//
//   FLAGS="--offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I refid_amd/csrc"
//   for f in conv_igemm conv_wino conv_wino6; do hipcc $FLAGS -c refid_amd/csrc/$f.hip -o /tmp/$f.o; done
//   hipcc $FLAGS -x hip tools/probes/splitk_host_check.cpp -x none /tmp/conv_igemm.o /tmp/conv_wino.o /tmp/conv_wino6.o -o /tmp/splitk_host_check
//   python -c "import sys; sys.path.insert(0, 'tests'); import test_host_logic as t; [print(*r) for r in t.CONV_WORKSPACE_TABLE]" > /tmp/conv_ws.txt
//   /tmp/splitk_host_check /tmp/conv_ws.txt
//
// Every row of tests/test_host_logic.py::CONV_WORKSPACE_TABLE goes through the tile's plan and workspace size
// (refid_conv_workspace_bytes) and, where it splits, through refid_launch_splitk with a stub in place of the partial launch:
// a workspace one byte short and a misaligned one must be refused before anything is launched, the right one must reach the
// stub with the partial pass's arguments.  Needs no GPU: without a device the finishing launch reports a launch error (2).
#include "common.h"
#include "conv_args.h"
#include <cstring>
#include <vector>

static char g_err[512];
void refid_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" int refid_device_cu_count(void) { return 256; }
// the tiles conv_igemm.hip dispatches to besides the three under test
bool refid_split3x3_eligible(const ConvKArgs&) { return false; }
int refid_launch_split3x3(const ConvKArgs&, int, int, int, int, hipStream_t) { return 1; }
int refid_launch_pointwise(const ConvKArgs&, hipStream_t, const PwExtra*, int) { return 1; }

#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "line %d row %d: %s failed (%s)\n", __LINE__, row, #c, g_err); return 1; } } while (0)

int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) { fprintf(stderr, "usage: splitk_host_check TABLE (rows of CONV_WORKSPACE_TABLE)\n"); return 2; }
    int k, s, mode, algo, n, h, w, ca, cb, cout, split, row = 0, nsplit = 0;
    long long want;
    while (fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %lld", &k, &s, &mode, &algo, &n, &h, &w, &ca, &cb, &cout, &split, &want) == 12) {
        ++row;
        refid_conv_desc d;
        memset(&d, 0, sizeof(d));
        d.n = n; d.h = h; d.w = w;
        d.ho = mode == 0 ? h / s : h; d.wo = mode == 0 ? w / s : w;
        d.c_a = ca; d.c_b = cb; d.cout = cout; d.cout_pad = (cout + 63) / 64 * 64;
        d.kh = d.kw = k; d.stride = s; d.pad = k > 1; d.mode = mode; d.algo = algo; d.split_k = split;
        const size_t got = refid_conv_workspace_bytes(&d);
        EXPECT(got == (size_t)want);
        if (got == 0) continue;
        // the same workspace through the launch sequence (ks and the pixel count recovered from the byte count)
        ++nsplit;
        const long long npix = (long long)n * d.ho * d.wo * (mode == 2 ? 4 : 1);
        const int ldW = (cout + 3) / 4 * 4;
        const int ks = (int)(got / (npix * ldW * 4));
        EXPECT(ks >= 2 && ks <= 8 && refid_splitk_bytes(ks, npix, cout) == got);
        ConvKArgs a{};
        a.ksplit = 1; a.N = n; a.Ho = d.ho; a.Wo = d.wo; a.Cout = cout;
        std::vector<float> ws(got / 4 + 8);
        float* al = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(ws.data()) + 15) & ~uintptr_t(15));
        int calls = 0;
        ConvKArgs seen{};
        auto partial = [&](const ConvKArgs& p) { ++calls; seen = p; return 7; };     // (7: stop before the finishing launch)
        EXPECT(refid_launch_splitk("check", a, ks, npix, al, got - 1, partial, nullptr) == 1 && calls == 0 && strstr(g_err, "too small"));
        EXPECT(refid_launch_splitk("check", a, ks, npix, al + 1, got, partial, nullptr) == 1 && calls == 0);
        EXPECT(refid_launch_splitk("check", a, ks, npix, al, got, partial, nullptr) == 7 && calls == 1);
        EXPECT(seen.ksplit == ks && seen.wsStride == npix * ldW && seen.out == al && seen.ldO == ldW && seen.out2 == nullptr);
        for (size_t i = 0; i < got / 4; i += 1 + got / 64) al[i] = 1.f;                // the whole size is the caller's to write
    }
    fclose(f);
    int row0 = row; row = 0;
    EXPECT(row0 >= 20 && nsplit >= 10);
    // the clamp itself, over its whole argument range: 1 .. 8, never more than the chunks allow
    for (int nwg = 1; nwg <= 600; ++nwg)
        for (int nch = 0; nch <= 70; ++nch)
            for (int pol = 0; pol < 3; ++pol) {
                const int lim = pol == 2 ? 128 : 256, minc = pol == 0 ? 16 : 8, div = pol == 0 ? 8 : 4;
                const int ks = refid_splitk_count(nwg, nch, lim, minc, div);
                EXPECT(ks >= 1 && ks <= 8 && (ks == 1 || (nwg <= lim && nch >= minc && ks <= nch / div && ks <= 512 / nwg)));
            }
    printf("splitk_host_check: %d rows, %d split, ok\n", row0, nsplit);
    return 0;
}
