"""The numpy restatement of "Simulated events" in include/refid_hip.h (csrc/event_sim.hip): the ESIM contrast-threshold
model in integers.  Not a test file: test_event_sim_ref_host.py pins it against a scalar model written with
``fractions.Fraction``, test_hip_event_sim.py pins the device to it bit for bit.

Everything is int64 numpy apart from the three float64 operations of the time stamp, which numpy rounds once each, as the
kernel does with contraction off."""
import numpy as np

CAP = 255
TICK_ONE = 1 << 20
DEFAULT_SPAN = 452773


def default_lut(eps=1e-3):
    """rint(65536 ln(v / 255 + eps)) in float64, v = 0 .. 255."""
    v = np.arange(256, dtype=np.float64)
    return np.rint(65536.0 * np.log(v / 255.0 + eps)).astype(np.int32)


def min_threshold(lut):
    """The least threshold (units of 2^-16) for which (lut.max - lut.min) // c + 1 <= CAP."""
    lut = np.asarray(lut, dtype=np.int64)
    return int((lut.max() - lut.min()) // CAP + 1)


def luma(frames, bgr=False):
    f = np.asarray(frames).astype(np.int64)
    r, g, b = (f[..., 2], f[..., 1], f[..., 0]) if bgr else (f[..., 0], f[..., 1], f[..., 2])
    return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16


def reset(frame0, lut, bgr=False):
    """state = lut[Y8(frame0)], int32 (H, W)."""
    return np.asarray(lut, dtype=np.int32)[luma(frame0, bgr)].astype(np.int32)


def stamp(t0, t1, tick):
    """fl32(t0 + (t1 - t0) * (double(tick) 2^-20)), each float64 operation rounded once."""
    t0, t1 = np.float64(t0), np.float64(t1)
    dt = t1 - t0
    frac = np.asarray(tick).astype(np.float64) * np.float64(2.0 ** -20)        # exact
    part = dt * frac
    return (t0 + part).astype(np.float32)


def simulate(frames, stamps, state, lut, c_pos, c_neg, bgr=False):
    """frames uint8 (N, H, W, 3), stamps float64 (N,), state int32 (H, W), lut int32 [256], c_pos / c_neg an int or an int
    (H, W) array -> (rows float32 (E, 4), offsets int64 (N,), the new state int32 (H, W), overflow).  ``state`` is not
    modified.  ``overflow``: some pixel had more than CAP crossings in an interval; its walk stopped at CAP there."""
    frames = np.asarray(frames)
    n, h, w = frames.shape[:3]
    stamps = np.asarray(stamps, dtype=np.float64)
    assert n >= 2 and stamps.shape == (n,) and np.all(stamps[1:] > stamps[:-1])
    lut = np.asarray(lut, dtype=np.int64)
    cp = np.broadcast_to(np.asarray(c_pos, dtype=np.int64), (h, w)).reshape(-1)
    cn = np.broadcast_to(np.asarray(c_neg, dtype=np.int64), (h, w)).reshape(-1)
    ref = np.asarray(state, dtype=np.int64).reshape(-1).copy()
    levels = lut[luma(frames, bgr)].reshape(n, h * w)
    pix = np.arange(h * w, dtype=np.int64)
    out, offsets, overflow = [], [0], False
    for k in range(n - 1):
        a, b = levels[k], levels[k + 1]
        up, down = b > a, b < a
        den = np.abs(b - a)
        ticks, pixs, js, ps = [], [], [], []
        for j in range(CAP + 1):
            go = (up & (ref + cp <= b)) | (down & (ref - cn >= b))
            if not go.any():
                break
            if j == CAP:
                overflow = True
                break
            ref = np.where(go, np.where(up, ref + cp, ref - cn), ref)
            num = np.where(up, ref - a, a - ref)[go]
            ticks.append((num * TICK_ONE) // den[go])
            pixs.append(pix[go])
            js.append(np.full(int(go.sum()), j, dtype=np.int64))
            ps.append(np.where(up[go], 1.0, -1.0))
        count = 0
        if ticks:
            tick, px, jj, pp = (np.concatenate(v) for v in (ticks, pixs, js, ps))
            order = np.lexsort((jj, px, tick))
            tick, px, pp = tick[order], px[order], pp[order]
            rows = np.empty((len(tick), 4), dtype=np.float32)
            rows[:, 0] = stamp(stamps[k], stamps[k + 1], tick)
            rows[:, 1] = px % w
            rows[:, 2] = px // w
            rows[:, 3] = pp
            out.append(rows)
            count = len(tick)
        offsets.append(offsets[-1] + count)
    rows = np.concatenate(out) if out else np.zeros((0, 4), dtype=np.float32)
    return rows, np.asarray(offsets, dtype=np.int64), ref.reshape(h, w).astype(np.int32), overflow


def simulate_chunked(frames, stamps, lut, c_pos, c_neg, chunks, bgr=False):
    """reset on frame 0, then ``simulate`` over chunks of the given frame counts that share their boundary frames."""
    state = reset(frames[0], lut, bgr)
    rows, offsets, at = [], [np.zeros(1, dtype=np.int64)], 0
    for count in chunks:
        r, o, state, over = simulate(frames[at:at + count], stamps[at:at + count], state, lut, c_pos, c_neg, bgr)
        assert not over
        rows.append(r)
        offsets.append(o[1:] + offsets[-1][-1])
        at += count - 1
    assert at == len(frames) - 1
    return np.concatenate(rows), np.concatenate(offsets), state
