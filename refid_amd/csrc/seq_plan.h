// The host plan the two entry points of sequence.hip share: what refid_seq_desc and refid_seq_single_desc have in common
// (SeqArgs), and the checks of those fields and of the host table (seq_check).  An entry point fills a SeqArgs (in the
// order of its members), calls seq_check, adds the checks of its own fields and hands it to sequence.hip's seq_launch.
//
// Plain C++ on purpose: tools/probes/seq_check_host_check.cpp includes this file as host code, gives refid_set_error a
// body that keeps the text, and runs seq_check over valid and one-field-wrong tables under ASan + UBSan.
#pragma once
#include <stdint.h>

#include "../../include/refid_hip.h"

void refid_set_error(const char* fmt, ...);

struct SeqArgs {
    const float* events; long long n_events;
    const unsigned char* frames; int n_frames; long long frame_stride; int row_pitch, height, width, bgr;
    const refid_seq_pair *tab_host, *tab_dev; int count;       // pairs_* / items_*, n_pairs / n_items
    int out_h, out_w;
    long long* scratch; float *lq, *voxel;
    const char *who, *item, *count_name;       // the messages' words: "seq_assemble", "pair", "n_pairs"
    bool check_right;                          // the layout reads `right`
    bool limit_events;                         // voxel_norm: fewer than 2^30 events per item
};

#define SEQ_CHECK(cond, ...) do { if (!(cond)) { refid_set_error(__VA_ARGS__); return -1; } } while (0)

// 0, and the longest window of the table in *max_rows; or -1 with the error text set.  Reads tab_host[0 .. count) only,
// and only after count passed its own check.
inline int seq_check(const SeqArgs& a, long long* max_rows) {
    const char* w = a.who;
    SEQ_CHECK(a.lq && a.voxel, "%s: null outputs (lq %p, voxel %p)", w, (void*)a.lq, (void*)a.voxel);
    SEQ_CHECK(a.scratch, "%s: null scratch", w);
    SEQ_CHECK(a.tab_host && a.tab_dev && a.count > 0 && a.count <= 65535, "%s: %s %d needs 1..65535 %ss and both %s tables", w,
              a.count_name, a.count, a.item, a.item);
    SEQ_CHECK(a.n_events >= 0 && (a.n_events == 0 || a.events) && ((uintptr_t)a.events & 15) == 0,
              "%s: events must be %lld 16-byte aligned float32 rows", w, a.n_events);
    SEQ_CHECK(a.frames && a.n_frames > 0 && a.height > 0 && a.width > 0, "%s: no frames (n_frames %d, %dx%d)", w, a.n_frames,
              a.height, a.width);
    SEQ_CHECK(a.row_pitch >= 3ll * a.width && a.frame_stride >= (long long)(a.height - 1) * a.row_pitch + 3ll * a.width,
              "%s: row_pitch %d / frame_stride %lld too small for %dx%d frames", w, a.row_pitch, a.frame_stride, a.height, a.width);
    SEQ_CHECK(a.out_h >= a.height, "%s: out_h %d < height %d", w, a.out_h, a.height);
    SEQ_CHECK(a.out_w >= a.width, "%s: out_w %d < width %d", w, a.out_w, a.width);
    SEQ_CHECK((long long)a.out_h * a.out_w <= (1ll << 30), "%s: out_h x out_w %dx%d too large", w, a.out_h, a.out_w);
    *max_rows = 0;
    for (int p = 0; p < a.count; ++p) {
        const refid_seq_pair& s = a.tab_host[p];
        SEQ_CHECK(s.left >= 0 && s.left < a.n_frames, "%s: %s %d: left %d outside the %d frames", w, a.item, p, s.left, a.n_frames);
        SEQ_CHECK(!a.check_right || (s.right >= 0 && s.right < a.n_frames), "%s: %s %d: right %d outside the %d frames", w,
                  a.item, p, s.right, a.n_frames);
        SEQ_CHECK(s.row0 >= 0 && s.row0 <= s.row1, "%s: %s %d: row0 %lld > row1 %lld (or negative)", w, a.item, p, s.row0, s.row1);
        SEQ_CHECK(s.row1 <= a.n_events, "%s: %s %d: row1 %lld > n_events %lld", w, a.item, p, s.row1, a.n_events);
        // every event adds exactly 2^32 of magnitude to the scratch, so below 2^30 events the int64 sum S1 cannot overflow
        SEQ_CHECK(!a.limit_events || s.row1 - s.row0 < (1ll << 30),
                  "%s: %s %d: voxel_norm supports fewer than 2^30 events per %s (%lld)", w, a.item, p, a.item, s.row1 - s.row0);
        if (s.row1 - s.row0 > *max_rows) *max_rows = s.row1 - s.row0;
    }
    return 0;
}
