// Host-only run of the argument checker the two entry points of csrc/sequence.hip share (refid_amd/csrc/seq_plan.h), meant to
// be built with host sanitizers:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I refid_amd/csrc \
//         -x hip tools/probes/seq_check_host_check.cpp -o /tmp/seq_check_host_check
//   /tmp/seq_check_host_check
//
// (The header is plain C++: `c++ -std=c++17 -fsanitize=address,undefined -I refid_amd/csrc` builds the same program.)
//
// For both flavours -- pairs (`right` is checked) and items (`right` is not read; with norm fewer than 2^30 events per item)
// -- and tables of 1 and 3 rows, seq_check gets a valid call and calls with exactly one field wrong.  The valid tables hold
// empty windows (in the middle of the stream, at its end, and of a stream without events), a window with row1 == n_events
// and frame indices at both ends (0 and n_frames - 1); they must pass with the longest window in max_rows.  A wrong call
// must return -1 with the message that names the field, the row and the flavour's words.  The host table lives in a heap
// block of exactly `count` rows, so a read behind it stops the program under ASan; a count outside 1..65535 must be
// rejected before the table is read at all.  Needs no GPU.
#include "seq_plan.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

static char g_error[512];
void refid_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}

static int g_checks = 0;

struct Flavour {
    const char *who, *item, *count_name;
    bool check_right, limit_events;
};

constexpr long long N_EVENTS = 1000;
constexpr int N_FRAMES = 5, H = 37, W = 50;
alignas(16) static float g_events[8];                     // an aligned address; the checker never reads events or frames
static unsigned char g_frames[1];
static long long g_scratch[1];
static float g_out[2];
static refid_seq_pair g_dev[1];                           // stands for the device table: never read either

static SeqArgs valid_args(const Flavour& f, const refid_seq_pair* tab, int count) {
    SeqArgs a{};
    a.events = g_events; a.n_events = N_EVENTS;
    a.frames = g_frames; a.n_frames = N_FRAMES; a.frame_stride = 3ll * H * W; a.row_pitch = 3 * W;
    a.height = H; a.width = W; a.bgr = 1;
    a.tab_host = tab; a.tab_dev = g_dev; a.count = count;
    a.out_h = 40; a.out_w = 56;
    a.scratch = g_scratch; a.lq = g_out; a.voxel = g_out + 1;
    a.who = f.who; a.item = f.item; a.count_name = f.count_name;
    a.check_right = f.check_right; a.limit_events = f.limit_events;
    return a;
}

// rows of a valid table: the last one ends at n_events and uses the last frame; the others are empty windows
static std::vector<refid_seq_pair> valid_table(int count) {
    std::vector<refid_seq_pair> t(count);
    const refid_seq_pair rows[3] = {{N_FRAMES - 1, 0, 400, N_EVENTS, 1.f, 2.f},          // row1 == n_events, both frame ends
                                    {0, N_FRAMES - 1, 300, 300, 0.f, 0.f},               // empty, inside the stream
                                    {2, 2, N_EVENTS, N_EVENTS, 0.f, 0.f}};               // empty, at the end of the stream
    for (int p = 0; p < count; ++p) t[count - 1 - p] = rows[p];
    t.shrink_to_fit();
    return t;
}

static int expect(const char* what, const SeqArgs& a, const char* message, long long want_rows) {
    long long max_rows = -7;
    g_error[0] = 0;
    const int rc = seq_check(a, &max_rows);
    ++g_checks;
    if (message == nullptr) {
        if (rc == 0 && max_rows == want_rows && g_error[0] == 0) return 0;
        fprintf(stderr, "%s %s (count %d): expected acceptance with max_rows %lld, got rc %d, max_rows %lld, '%s'\n", a.who, what,
                a.count, want_rows, rc, max_rows, g_error);
        return 1;
    }
    if (rc == -1 && strcmp(g_error, message) == 0) return 0;
    fprintf(stderr, "%s %s (count %d): expected -1 with '%s', got rc %d, '%s'\n", a.who, what, a.count, message, rc, g_error);
    return 1;
}

static int run(const Flavour& f, int count) {
    char msg[512];
    const int last = count - 1;
    std::vector<refid_seq_pair> tab = valid_table(count);
    const SeqArgs good = valid_args(f, tab.data(), count);
    int bad = expect("valid", good, nullptr, N_EVENTS - 400);

    // a stream without events: null events, every window empty
    {
        std::vector<refid_seq_pair> t = valid_table(count);
        for (auto& s : t) s.row0 = s.row1 = 0;
        SeqArgs a = valid_args(f, t.data(), count);
        a.events = nullptr; a.n_events = 0;
        bad += expect("no events", a, nullptr, 0);
    }

    // one descriptor field wrong
    auto field = [&](const char* what, const std::function<void(SeqArgs&)>& change, const char* message) {
        SeqArgs a = good;
        change(a);
        bad += expect(what, a, message, 0);
    };
    snprintf(msg, sizeof msg, "%s: null outputs (lq %p, voxel %p)", f.who, (void*)nullptr, (void*)(g_out + 1));
    field("lq", [](SeqArgs& a) { a.lq = nullptr; }, msg);
    snprintf(msg, sizeof msg, "%s: null outputs (lq %p, voxel %p)", f.who, (void*)g_out, (void*)nullptr);
    field("voxel", [](SeqArgs& a) { a.voxel = nullptr; }, msg);
    snprintf(msg, sizeof msg, "%s: null scratch", f.who);
    field("scratch", [](SeqArgs& a) { a.scratch = nullptr; }, msg);
    snprintf(msg, sizeof msg, "%s: %s %d needs 1..65535 %ss and both %s tables", f.who, f.count_name, count, f.item, f.item);
    field("tab_host", [](SeqArgs& a) { a.tab_host = nullptr; }, msg);
    field("tab_dev", [](SeqArgs& a) { a.tab_dev = nullptr; }, msg);
    for (int n : {0, -1, 65536}) {                            // (65536 rows are not there: rejected before the table is read)
        snprintf(msg, sizeof msg, "%s: %s %d needs 1..65535 %ss and both %s tables", f.who, f.count_name, n, f.item, f.item);
        field("count", [n](SeqArgs& a) { a.count = n; }, msg);
    }
    snprintf(msg, sizeof msg, "%s: events must be %lld 16-byte aligned float32 rows", f.who, N_EVENTS);
    field("events + 4", [](SeqArgs& a) { a.events = g_events + 1; }, msg);
    field("events null", [](SeqArgs& a) { a.events = nullptr; }, msg);
    snprintf(msg, sizeof msg, "%s: events must be -1 16-byte aligned float32 rows", f.who);
    field("n_events", [](SeqArgs& a) { a.n_events = -1; }, msg);
    snprintf(msg, sizeof msg, "%s: no frames (n_frames %d, %dx%d)", f.who, 0, H, W);
    field("n_frames", [](SeqArgs& a) { a.n_frames = 0; }, msg);
    snprintf(msg, sizeof msg, "%s: no frames (n_frames %d, %dx%d)", f.who, N_FRAMES, H, W);
    field("frames", [](SeqArgs& a) { a.frames = nullptr; }, msg);
    snprintf(msg, sizeof msg, "%s: no frames (n_frames %d, %dx%d)", f.who, N_FRAMES, 0, W);
    field("height", [](SeqArgs& a) { a.height = 0; }, msg);
    snprintf(msg, sizeof msg, "%s: row_pitch %d / frame_stride %lld too small for %dx%d frames", f.who, 3 * W - 1, 3ll * H * W, H, W);
    field("row_pitch", [](SeqArgs& a) { a.row_pitch = 3 * W - 1; }, msg);
    snprintf(msg, sizeof msg, "%s: row_pitch %d / frame_stride %lld too small for %dx%d frames", f.who, 3 * W, 3ll * H * W - 1, H, W);
    field("frame_stride", [](SeqArgs& a) { a.frame_stride = 3ll * H * W - 1; }, msg);
    snprintf(msg, sizeof msg, "%s: out_h 36 < height 37", f.who);
    field("out_h", [](SeqArgs& a) { a.out_h = 36; }, msg);
    snprintf(msg, sizeof msg, "%s: out_w 48 < width 50", f.who);
    field("out_w", [](SeqArgs& a) { a.out_w = 48; }, msg);
    snprintf(msg, sizeof msg, "%s: out_h x out_w 32768x32769 too large", f.who);
    field("out_h x out_w", [](SeqArgs& a) { a.out_h = 32768; a.out_w = 32769; }, msg);
    bad += expect("out_h x out_w = 2^30", [&] { SeqArgs a = good; a.out_h = a.out_w = 32768; return a; }(), nullptr, N_EVENTS - 400);

    // one field of one table row wrong: the first and the last row (behind which the heap block ends)
    for (int p : {0, last}) {
        auto row = [&](const char* what, const std::function<void(refid_seq_pair&)>& change, const char* message,
                       long long want_rows = 0) {
            std::vector<refid_seq_pair> t = valid_table(count);
            change(t[p]);
            bad += expect(what, valid_args(f, t.data(), count), message, want_rows);
        };
        const long long keep = N_EVENTS - 400;                 // the longest window when row p's own window is untouched
        for (int v : {-1, N_FRAMES}) {
            snprintf(msg, sizeof msg, "%s: %s %d: left %d outside the %d frames", f.who, f.item, p, v, N_FRAMES);
            row("left", [v](refid_seq_pair& s) { s.left = v; }, msg);
            snprintf(msg, sizeof msg, "%s: %s %d: right %d outside the %d frames", f.who, f.item, p, v, N_FRAMES);
            row("right", [v](refid_seq_pair& s) { s.right = v; }, f.check_right ? msg : nullptr, keep);
        }
        row("left 0", [](refid_seq_pair& s) { s.left = 0; }, nullptr, keep);
        row("left n_frames - 1", [](refid_seq_pair& s) { s.left = N_FRAMES - 1; }, nullptr, keep);
        snprintf(msg, sizeof msg, "%s: %s %d: row0 %lld > row1 %lld (or negative)", f.who, f.item, p, -1ll, 5ll);
        row("row0 -1", [](refid_seq_pair& s) { s.row0 = -1; s.row1 = 5; }, msg);
        snprintf(msg, sizeof msg, "%s: %s %d: row0 %lld > row1 %lld (or negative)", f.who, f.item, p, 11ll, 10ll);
        row("row0 > row1", [](refid_seq_pair& s) { s.row0 = 11; s.row1 = 10; }, msg);
        snprintf(msg, sizeof msg, "%s: %s %d: row1 %lld > n_events %lld", f.who, f.item, p, N_EVENTS + 1, N_EVENTS);
        row("row1", [](refid_seq_pair& s) { s.row0 = 0; s.row1 = N_EVENTS + 1; }, msg);
        row("whole stream", [](refid_seq_pair& s) { s.row0 = 0; s.row1 = N_EVENTS; }, nullptr, N_EVENTS);
    }

    // 2^30 events in one window: too many for voxel_norm's int64 sum, fine without it
    {
        std::vector<refid_seq_pair> t = valid_table(count);
        t[last].row0 = 3; t[last].row1 = 3 + (1ll << 30);
        SeqArgs a = valid_args(f, t.data(), count);
        a.n_events = 4 + (1ll << 30);
        snprintf(msg, sizeof msg, "%s: %s %d: voxel_norm supports fewer than 2^30 events per %s (%lld)", f.who, f.item, last, f.item,
                 1ll << 30);
        bad += expect("2^30 events", a, f.limit_events ? msg : nullptr, 1ll << 30);
        t[last].row1 -= 1;
        bad += expect("2^30 - 1 events", a, nullptr, (1ll << 30) - 1);
    }
    return bad;
}

int main() {
    const Flavour flavours[3] = {{"seq_assemble", "pair", "n_pairs", true, false},
                                 {"seq_assemble_single", "item", "n_items", false, true},
                                 {"seq_assemble_single", "item", "n_items", false, false}};     // norm == 0
    int bad = 0;
    for (const Flavour& f : flavours)
        for (int count : {1, 3}) bad += run(f, count);
    if (bad) {
        fprintf(stderr, "seq_check_host_check: %d of %d checks failed\n", bad, g_checks);
        return 1;
    }
    printf("seq_check_host_check: %d checks, ok\n", g_checks);
    return 0;
}
