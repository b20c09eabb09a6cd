"""The numpy restatement of "Double integral" in include/refid_hip.h (csrc/edi.hip): the event-based double integral, the
model-based inverse of event_sim + blur_synth.  Not a test file: test_edi_ref_host.py pins it against closed forms and the
simulator's closed loop, test_hip_edi.py pins the device to it bit for bit.

Levels are Python / int64 integers in units of 2^-16; every float64 operation is written out one per line so that numpy
rounds it once, as the kernel does with contraction off.  Where the kernel walks a pixel's events in time order, this
file takes prefix sums and ``searchsorted`` on the same float32 stamps."""
import numpy as np

MAX_COUNT = 64                      # M, == blur_ref.MAX_COUNT
MAX_INSTANTS = 256                  # output instants per item
MAX_PIXELS = 1 << 25
MAX_THRESHOLD = 1 << 20             # thresholds, units of 2^-16
CLAMP = 32                          # the gain is exp(level) for |level| <= CLAMP, held there beyond it
FIXED_ONE = 1 << 16
TABLE = 2 * CLAMP + 1 + 256 + 256
SAMPLES, CONTINUOUS = 0, 1


def to_fixed(c):
    return int(np.rint(float(c) * FIXED_ONE))


def gain_tables():
    """float64 [577]: exp(i), i = -32 .. 32 | exp(h / 256), h = 0 .. 255 | exp(l / 65536), l = 0 .. 255."""
    t0 = np.exp(np.arange(-CLAMP, CLAMP + 1, dtype=np.float64))
    t1 = np.exp(np.arange(256, dtype=np.float64) / 256.0)
    t2 = np.exp(np.arange(256, dtype=np.float64) / 65536.0)
    return np.concatenate([t0, t1, t2])


def gain(level, tables):
    """(g float64, clamped bool) of integer levels: e = 65536 i + 256 h + l after the clamp, g = (T0[i] T1[h]) T2[l]."""
    e = np.asarray(level, dtype=np.int64)
    ec = np.clip(e, -CLAMP * FIXED_ONE, CLAMP * FIXED_ONE)
    i, h, l = ec >> 16, (ec >> 8) & 255, ec & 255
    first = tables[i + CLAMP] * tables[2 * CLAMP + 1 + h]
    return first * tables[2 * CLAMP + 1 + 256 + l], ec != e


def load(events, height, width):
    """The stream by pixel: ({pix: (stamps float32, signs int64 of +1 / -1)} in time order, dropped rows).  x and y are
    truncated toward zero; a row outside the frame (or with a NaN coordinate) is dropped; p > 0 is positive, anything else
    negative."""
    ev = np.asarray(events, dtype=np.float32).reshape(-1, 4)
    assert not np.any(ev[1:, 0] < ev[:-1, 0]), "the stream is not sorted by time"
    x, y = np.trunc(ev[:, 1]), np.trunc(ev[:, 2])
    inside = (x >= 0) & (x < width) & (y >= 0) & (y < height)
    pix = (y[inside].astype(np.int64) * width + x[inside].astype(np.int64))
    t, sign = ev[inside, 0], np.where(ev[inside, 3] > 0, 1, -1).astype(np.int64)
    order = np.argsort(pix, kind="stable")
    pix, t, sign = pix[order], t[order], sign[order]
    cuts = np.flatnonzero(np.diff(pix)) + 1
    out = {}
    for a, b in zip(np.concatenate([[0], cuts]).tolist(), np.concatenate([cuts, [len(pix)]]).tolist()):
        if b > a:
            out[int(pix[a])] = (t[a:b], sign[a:b])
    return out, int(len(ev) - inside.sum())


def sample_instants(s, e, m):
    """float32 [m]: fl32(s + ((e - s) j) / (m - 1)) in float64, held inside [s, e]; m = 1: s."""
    s, e = np.float32(s), np.float32(e)
    if m == 1:
        return np.array([s], dtype=np.float32)
    j = np.arange(m, dtype=np.float64)
    span = np.float64(e) - np.float64(s)
    part = span * j
    part = part / np.float64(m - 1)
    return np.clip((np.float64(s) + part).astype(np.float32), s, e)


def output_instants(layout, bounds, m=1, n=None):
    """float32 (T,) for bounds (s0, e0, s1, e1): sharp: s0 + (s1 - s0)(f + 1)/(n + 1), f < n; blur: s0 + (e1 - s0) f /
    (2m + n - 1), f < 2m + n; single: (s0 + e0) / 2.  float64 from the float32 bounds, one operation per line, then fl32,
    held inside the bounds."""
    s0, e0, s1, e1 = (np.float64(np.float32(v)) for v in bounds)
    if layout == "single":
        return np.array([(s0 + e0) / 2.0], dtype=np.float64).astype(np.float32)
    if layout == "sharp":
        f = np.arange(1, n + 1, dtype=np.float64)
        part = (s1 - s0) * f
        part = part / np.float64(n + 1)
        return np.clip((s0 + part).astype(np.float32), np.float32(s0), np.float32(s1))
    f = np.arange(2 * m + n, dtype=np.float64)
    part = (e1 - s0) * f
    part = part / np.float64(2 * m + n - 1)
    return np.clip((s0 + part).astype(np.float32), np.float32(s0), np.float32(e1))


def _running(terms):
    acc = 0.0
    for v in terms.tolist():            # in order, each sum rounded once
        acc = acc + v
    return acc


def _normaliser(t, cum, base_at, s, e, m, exposure, tables):
    """(S, clamped) of the key with exposure [s, e] for a pixel with stamps t and prefix levels cum; the key's own level is
    cum[base_at]."""
    if s == e:
        return 1.0, False
    if exposure == SAMPLES:
        at = np.searchsorted(t, sample_instants(s, e, m), side="right")
        at = np.maximum(at, base_at)                                   # (sample 0 is s itself)
        g, cl = gain(cum[at] - cum[base_at], tables)
        return _running(g) / np.float64(m), bool(cl.any())
    a, b = base_at, max(int(np.searchsorted(t, e, side="right")), base_at)
    knots = np.concatenate([[np.float64(s)], t[a:b].astype(np.float64), [np.float64(e)]])
    g, cl = gain(cum[a:b + 1] - cum[base_at], tables)
    acc = _running(g * (knots[1:] - knots[:-1]))
    return acc / (np.float64(e) - np.float64(s)), bool(cl.any())


def edi(frames, stream, items, bounds, instants, m, exposure, c_pos, c_neg, eps=1e-3):
    """frames uint8 (N, H, W, 3); stream from ``load``; items int (P, 2) rows [left, right], right < 0: none; bounds float32
    (P, 4) rows [s0, e0, s1, e1]; instants float32 (P, T) ascending inside [s0, e1] ([s0, e0] without a right key);
    c_pos, c_neg in units of 2^-16 -> (uint8 (P, T, H, W, 3), clamped (item, pixel) pairs)."""
    frames = np.asarray(frames)
    by_pixel = stream[0] if isinstance(stream, tuple) else stream
    h, w = frames.shape[1:3]
    items = np.asarray(items, dtype=np.int64).reshape(-1, 2)
    bounds = np.asarray(bounds, dtype=np.float32).reshape(-1, 4)
    instants = np.asarray(instants, dtype=np.float32).reshape(len(items), -1)
    assert 1 <= m <= MAX_COUNT and 1 <= instants.shape[1] <= MAX_INSTANTS and exposure in (SAMPLES, CONTINUOUS)
    assert 1 <= c_pos <= MAX_THRESHOLD and 1 <= c_neg <= MAX_THRESHOLD
    tables = gain_tables()
    eps255 = np.float64(255.0 * float(eps))
    n_t = instants.shape[1]
    out = np.empty((len(items), n_t, h, w, 3), dtype=np.uint8)
    clamped = 0
    for k, (left, right) in enumerate(items.tolist()):
        s0, e0, s1, e1 = bounds[k]
        tau = instants[k]
        pair = right >= 0
        assert s0 <= e0 and (not pair or e0 <= s1 <= e1) and np.all(tau[1:] >= tau[:-1])
        assert tau[0] >= s0 and tau[-1] <= (e1 if pair else e0)
        if pair:
            span = np.float64(s1) - np.float64(e0)
            wgt = np.where(tau <= e0, 0.0, np.where(tau >= s1, 1.0, (tau.astype(np.float64) - np.float64(e0)) / (span if span > 0 else 1.0)))
        b_left = frames[left].astype(np.float64) + eps255                             # (H, W, 3)
        b_right = frames[right].astype(np.float64) + eps255 if pair else None
        g_l = np.ones((n_t, h, w), dtype=np.float64)
        g_r = np.ones((n_t, h, w), dtype=np.float64)
        s_l = np.ones((h, w), dtype=np.float64)
        s_r = np.ones((h, w), dtype=np.float64)
        for pix, (t, sign) in by_pixel.items():
            y, x = divmod(pix, w)
            cum = np.concatenate([[0], np.cumsum(np.where(sign > 0, c_pos, -c_neg))]).astype(np.int64)
            lo = int(np.searchsorted(t, s0, side="right"))                            # events at s0 or before: not the item's
            at = np.maximum(np.searchsorted(t, tau, side="right"), lo)
            g, cl = gain(cum[at] - cum[lo], tables)
            g_l[:, y, x] = g
            s_l[y, x], c1 = _normaliser(t, cum, lo, s0, e0, m, exposure, tables)
            hit = bool(cl.any()) or c1
            if pair:
                mid = max(int(np.searchsorted(t, s1, side="right")), lo)
                g, cl = gain(cum[at] - cum[mid], tables)
                g_r[:, y, x] = g
                s_r[y, x], c2 = _normaliser(t, cum, mid, s1, e1, m, exposure, tables)
                hit = hit or bool(cl.any()) or c2
            clamped += int(hit)
        for f in range(n_t):
            lat = b_left * g_l[f][:, :, None]
            lat = lat / s_l[:, :, None]
            if pair:
                other = b_right * g_r[f][:, :, None]
                other = other / s_r[:, :, None]
                lat = (1.0 - wgt[f]) * lat
                other = wgt[f] * other
                lat = lat + other
            lat = lat - eps255
            out[k, f] = np.clip(np.rint(lat), 0.0, 255.0).astype(np.uint8)
    return out, clamped
