// Host-only walk of the weight-packing record builder, meant to be built with host sanitizers:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I refid_amd/csrc \
//         -x hip tools/probes/pack_host_check.cpp -o /tmp/pack_host_check && /tmp/pack_host_check
//
// pack.hip is compiled INTO this program (its records live in an unnamed namespace, and the probe reads their `total`), with
// refid_set_error stubbed; nothing is launched, so it needs no GPU.  Roles x kinds x plane counts x the geometries of
// tests/test_hip_pack_layouts.py plus degenerate ones (o or i = 0, bn = 0, kc = 0, negative sizes, kinds and roles out of range) go
// through the size functions, refid_pack_entry_fill and refid_pack_table_check: nothing may trap, every accepted record's
// `total` must give the bytes its size function reports, and a table of the accepted records must pass the check until a
// record is blanked or moved.  Prints "clean" or the findings.
#include "../../refid_amd/csrc/pack.hip"
#include <vector>

static char g_err[512];
void refid_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static int findings = 0;
#define EXPECT(c, ...) do { if (!(c)) { ++findings; fprintf(stderr, "line %d: %s failed: ", __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, " (%s)\n", g_err); } } while (0)

// the exported size function that belongs to a record kind
static size_t api_size(int kind, int planes, int role, int o, int i, int kh, int kw, int kc, int bn) {
    switch (kind) {
        case 0: return refid_packed_weight_floats(role, o, i, kh, kw, kc, bn) * (planes ? 2 : 4);
        case 1: case 2: return refid_packed_weight_split_bytes(role, o, i, kh, kw, bn, planes);
        case 3: return refid_packed_weight_wino6_bytes(role, o, i, bn);
        case 5: return planes == 1 ? refid_packed_weight_wino1h_bytes(role, o, i, bn) : refid_packed_weight_wino3h_bytes(role, o, i, bn);
        case 6: return refid_packed_weight_split_f16_bytes(role, o, i, kh, kw, bn);
        default: return (size_t)o * 4;
    }
}

int main() {
    const int geos[][2] = {{20, 12}, {24, 20}, {40, 24}, {12, 24}, {20, 24}, {37, 5}, {1, 1}, {0, 12}, {20, 0}, {-3, 12}, {20, -1}, {4096, 4096}};
    const int ks[] = {0, 1, 2, 3, 4, 5, -1};
    const int kcs[] = {8, 16, 0, -8}, bns[] = {32, 64, 0, -32};
    float w = 0.f, s = 0.f;
    alignas(16) char dst[16];
    std::vector<PackEntry> table;
    long long blk = 0, tried = 0;
    for (int kind = -1; kind <= 7; ++kind)
        for (int role = -1; role <= 8; ++role)
            for (auto& g : geos)
                for (int k : ks)
                    for (int kc : kcs)
                        for (int bn : bns)
                            for (int planes = -1; planes <= 4; ++planes)
                                for (int scaled = 0; scaled < 2; ++scaled) {
                                    const int o = g[0], i = g[1];
                                    PackEntry en;
                                    memset(&en, 0x5a, sizeof(en));
                                    ++tried;
                                    const int nb = refid_pack_entry_fill(&en, kind, &w, scaled || kind == 4 ? &s : nullptr, dst, role, o, i, k, k, kc,
                                                                         bn, planes, (int)blk);
                                    if (kind == 0 && planes == 0 && nb < 0)     // what the builder refuses has no size either
                                        EXPECT(scaled || refid_packed_weight_floats(role, o, i, k, k, kc, bn) == 0, "kind 0 role %d %dx%d k %d", role, o, i, k);
                                    if (nb < 0) { EXPECT(g_err[0] != 0, "a refusal without a message"); continue; }
                                    EXPECT(nb >= 1 && nb <= 1024 && nb == en.nblk && en.blk0 == blk && en.kind == kind && en.total > 0,
                                           "kind %d role %d: nblk %d / %d, total %lld", kind, role, nb, en.nblk, en.total);
                                    EXPECT(o > 0 && (kind == 4 || (i > 0 && bn > 0 && k > 0)), "kind %d accepted o %d i %d bn %d k %d", kind, o, i, bn, k);
                                    EXPECT(nb == (en.total + 255) / 256 || nb == 1024, "kind %d: %d workgroups for %lld", kind, nb, en.total);
                                    // bytes from the record's total, restated: elements x element size + header
                                    const long long t = en.total;
                                    const size_t want = kind == 0 ? t * (planes ? 2 : 4) : kind == 3 ? t * 96 : kind == 5 ? 64 + t * 32 * en.planes
                                                      : kind == 6 ? 64 + t * 2 : kind == 4 ? t * 4 : t * 2;
                                    const size_t got = api_size(kind, planes, role, o, i, k, k, kc, bn);
                                    EXPECT(got == want && got == pack_entry_size(en), "kind %d role %d %dx%d k %d planes %d: size %zu, record %zu", kind, role, o, i, k,
                                           planes, got, want);
                                    if (table.size() < 4096) { table.push_back(en); blk += nb; }
                                }
    EXPECT(table.size() > 100, "only %zu records were accepted", table.size());
    EXPECT(refid_pack_table_check(table.data(), (int)table.size()) == blk, "the table of accepted records");
    EXPECT(refid_pack_table_check(table.data(), 0) == -1 && refid_pack_table_check(nullptr, 3) == -1, "an empty table");
    std::vector<PackEntry> t2 = table;
    memset(&t2[t2.size() / 2], 0, sizeof(PackEntry));
    EXPECT(refid_pack_table_check(t2.data(), (int)t2.size()) == -1, "an unfilled record");
    t2 = table;
    t2[7].blk0 += 1;
    EXPECT(refid_pack_table_check(t2.data(), (int)t2.size()) == -1, "a gap in blk0");
    EXPECT(refid_pack_entry_fill(nullptr, 0, &w, nullptr, dst, 0, 20, 12, 3, 3, 8, 32, 0, 0) == -1, "a null record");
    EXPECT(refid_pack_entry_fill(&t2[0], 5, &w, nullptr, dst + 4, 5, 40, 24, 3, 3, 16, 64, 2, 0) == -1, "a misaligned fp16 packing");
    EXPECT(refid_pack_entry_fill(&t2[0], 0, &w, nullptr, dst, 0, 20, 12, 3, 3, 8, 32, 0, -1) == -1, "a negative first block");
    printf("%lld records tried, %zu accepted into the table: %s\n", tried, table.size(), findings ? "FINDINGS (above)" : "clean");
    return findings ? 1 : 0;
}
