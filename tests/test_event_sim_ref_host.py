"""CPU-only: pins tests/event_sim_ref.py, the numpy restatement of "Simulated events" (include/refid_hip.h), against a
differently written scalar model -- one pixel at a time, crossing times as exact ``fractions.Fraction`` -- and checks
the properties the contract states; also the host helpers of refid_amd.event_sim (table, threshold maps, cap, .npz
files), none of which needs a GPU."""
from fractions import Fraction

import numpy as np
import pytest

import event_sim_ref as R


def _scalar_model(frames, stamps, state, lut, c_pos, c_neg, bgr=False):
    """One pixel at a time.  The level moves linearly from a to b over the interval; the crossing of level L happens at
    the exact fraction (L - a) / (b - a) of it, the tick is the floor of that fraction times 2^20."""
    n, h, w = frames.shape[:3]
    events, state = [], [[int(v) for v in row] for row in state]
    for y in range(h):
        for x in range(w):
            cp = int(c_pos[y][x]) if np.ndim(c_pos) else int(c_pos)
            cn = int(c_neg[y][x]) if np.ndim(c_neg) else int(c_neg)
            ref = state[y][x]
            for k in range(n - 1):
                level = []
                for f in (frames[k, y, x], frames[k + 1, y, x]):
                    r, g, b = (int(f[2]), int(f[1]), int(f[0])) if bgr else (int(f[0]), int(f[1]), int(f[2]))
                    level.append(int(lut[(19595 * r + 38470 * g + 7471 * b + 32768) // 65536]))
                a, b = level
                j = 0
                while a != b and j < R.CAP:
                    nxt = ref + cp if b > a else ref - cn
                    if (b > a and nxt > b) or (b < a and nxt < b):
                        break
                    ref = nxt
                    when = Fraction(ref - a, b - a)                    # exact crossing time within the interval
                    assert 0 < when <= 1
                    tick = (when * 2 ** 20).__floor__()
                    t = np.float32(np.float64(stamps[k]) + (np.float64(stamps[k + 1]) - np.float64(stamps[k])) * np.float64(tick / 2 ** 20))
                    events.append((k, tick, y * w + x, j, t, x, y, 1.0 if b > a else -1.0))
                    j += 1
            state[y][x] = ref
    events.sort(key=lambda e: e[:4])
    rows = np.array([e[4:] for e in events], dtype=np.float32).reshape(-1, 4)
    offsets = np.searchsorted(np.array([e[0] for e in events], dtype=np.int64), np.arange(n), "left")
    return rows, offsets.astype(np.int64), np.array(state, dtype=np.int32)


def _noise(seed, n, h, w):
    return np.random.default_rng(seed).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)


def _invariant(frames, state, lut, cp, cn):
    a = np.asarray(lut, dtype=np.int64)[R.luma(frames)]
    ref = state.astype(np.int64)
    return bool(np.all((a - cp < ref) & (ref < a + cn)))


def test_the_default_table():
    lut = R.default_lut()
    assert lut.dtype == np.int32 and lut.shape == (256,) and np.all(np.diff(lut) > 0)
    assert int(lut[255]) - int(lut[0]) == R.DEFAULT_SPAN == 452773
    assert R.min_threshold(lut) == 1776
    assert R.luma(np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255]], dtype=np.uint8)).tolist() == [0, 255, 76, 150, 29]
    assert R.luma(np.array([10, 20, 30], dtype=np.uint8), bgr=True) == R.luma(np.array([30, 20, 10], dtype=np.uint8))


@pytest.mark.parametrize("seed,n,h,w,cp,cn,bgr", [(0, 3, 3, 5, 13107, 13107, False), (1, 4, 4, 4, 6000, 9000, True), (2, 2, 2, 7, 1776, 1776, False),
                                                  (3, 5, 3, 3, "map", "map", False)])
def test_the_restatement_equals_the_scalar_model_with_exact_crossing_times(seed, n, h, w, cp, cn, bgr):
    frames = _noise(seed, n, h, w)
    rng = np.random.default_rng(100 + seed)
    if cp == "map":
        cp, cn = rng.integers(1776, 30000, size=(h, w)), rng.integers(1776, 30000, size=(h, w))
    stamps = np.cumsum(rng.uniform(1e-3, 5e-3, size=n))
    lut = R.default_lut()
    state = R.reset(frames[0], lut, bgr)
    rows, offsets, new_state, over = R.simulate(frames, stamps, state, lut, cp, cn, bgr)
    want_rows, want_offsets, want_state = _scalar_model(frames, stamps, state, lut, cp, cn, bgr)
    assert not over and len(rows) > 0
    assert rows.tobytes() == want_rows.tobytes() and offsets.tolist() == want_offsets.tolist()
    assert new_state.tobytes() == want_state.tobytes()


def test_the_state_invariant_holds_at_every_boundary_and_ref_tracks_the_level():
    lut = R.default_lut()
    frames = _noise(5, 7, 6, 9)
    cp, cn = 5000, 7000
    stamps = np.arange(7, dtype=np.float64) / 240.0
    state = R.reset(frames[0], lut)
    assert _invariant(frames[0], state, lut, cp, cn)
    for k in range(6):
        rows, offsets, state, over = R.simulate(frames[k:k + 2], stamps[k:k + 2], state, lut, cp, cn)
        assert not over and offsets.tolist() == [0, len(rows)]
        assert _invariant(frames[k + 1], state, lut, cp, cn)
        assert int(np.abs(state.astype(np.int64) - lut[R.luma(frames[k + 1])]).max()) < max(cp, cn)     # within one threshold


def test_static_frames_give_no_events():
    frames = np.repeat(_noise(6, 1, 5, 5), 4, axis=0)
    lut = R.default_lut()
    state = R.reset(frames[0], lut)
    rows, offsets, new_state, over = R.simulate(frames, np.arange(4.0), state, lut, 1776, 1776)
    assert rows.shape == (0, 4) and rows.dtype == np.float32 and offsets.tolist() == [0, 0, 0, 0] and not over
    assert new_state.tobytes() == state.tobytes()


def test_a_flash_at_the_minimum_threshold_stays_at_the_cap():
    lut = R.default_lut()
    frames = np.zeros((5, 2, 2, 3), dtype=np.uint8)
    frames[1::2, 0, 1] = 255                                           # 0 -> 255 -> 0 -> 255 -> 0 at one pixel
    state = R.reset(frames[0], lut)
    rows, offsets, _, over = R.simulate(frames, np.arange(5.0), state, lut, 1776, 1776)
    per = np.diff(offsets)
    assert not over and np.all((per >= 254) & (per <= 255)), per
    assert np.all(rows[:, 1] == 1) and np.all(rows[:, 2] == 0)
    assert np.all(rows[:offsets[1], 3] == 1) and np.all(rows[offsets[1]:offsets[2], 3] == -1)
    # 1775 is refused because a pixel may start up to c - 1 below its level: from the level itself it still gives 255
    _, offsets, _, over = R.simulate(frames[:2], np.arange(2.0), state, lut, 1775, 1775)
    assert not over and offsets.tolist() == [0, 255]
    _, offsets, _, over = R.simulate(frames[:2], np.arange(2.0), state - 1774, lut, 1775, 1775)
    assert over and offsets.tolist() == [0, 255]                       # ... and from there the walk stops at the cap and says so
    _, offsets, _, over = R.simulate(frames[:2], np.arange(2.0), state, lut, 1700, 1700)
    assert over and offsets.tolist() == [0, 255]


@pytest.mark.parametrize("t0,dt", [(0.0, 1 / 240), (1e9, 1 / 240), (1e9, 100.0), (16777216.0, 1.0), (3.0, 1e-6)])
def test_t_is_non_decreasing_in_float32(t0, dt):
    lut = R.default_lut()
    frames = _noise(7, 4, 8, 8)
    stamps = t0 + dt * np.arange(4, dtype=np.float64)
    rows, offsets, _, _ = R.simulate(frames, stamps, R.reset(frames[0], lut), lut, 3000, 3000)
    assert len(rows) > 100 and rows.dtype == np.float32 and not np.any(np.diff(rows[:, 0]) < 0)
    for k in range(3):
        part = rows[offsets[k]:offsets[k + 1], 0]
        assert np.all(part >= np.float32(stamps[k])) and np.all(part <= np.float32(stamps[k + 1]))
    # all ticks of one interval, in order
    every = R.stamp(stamps[1], stamps[2], np.arange(1, R.TICK_ONE + 1))
    assert not np.any(np.diff(every) < 0) and every[-1] == np.float32(stamps[2])


def test_offsets_agree_with_the_rows_of_each_interval():
    lut = R.default_lut()
    frames = _noise(8, 5, 4, 6)
    stamps = np.array([0.0, 0.5, 0.75, 2.0, 2.25])
    rows, offsets, _, _ = R.simulate(frames, stamps, R.reset(frames[0], lut), lut, 4000, 4000)
    assert offsets.dtype == np.int64 and offsets[0] == 0 and offsets[-1] == len(rows)
    for k in range(4):
        one, o, _, _ = R.simulate(frames[k:k + 2], stamps[k:k + 2], R.simulate_chunked(frames[:k + 1], stamps[:k + 1], lut, 4000, 4000, [k + 1])[2]
                                  if k else R.reset(frames[0], lut), lut, 4000, 4000)
        assert rows[offsets[k]:offsets[k + 1]].tobytes() == one.tobytes()


def test_chunked_simulation_equals_one_shot():
    lut = R.default_lut()
    frames = _noise(9, 9, 5, 7)
    stamps = np.cumsum(np.random.default_rng(9).uniform(0.001, 0.01, size=9))
    whole = R.simulate_chunked(frames, stamps, lut, 2500, 3500, [9])
    for chunks in ([3, 3, 5], [2] * 8, [5, 5]):
        parts = R.simulate_chunked(frames, stamps, lut, 2500, 3500, chunks)
        assert parts[0].tobytes() == whole[0].tobytes() and parts[1].tolist() == whole[1].tolist()
        assert parts[2].tobytes() == whole[2].tobytes()


def test_the_package_helpers_agree_with_the_restatement(tmp_path):
    from refid_amd import _lib, event_sim, sequence
    from refid_amd._lib import RefidHipError
    assert event_sim.default_lut().tobytes() == R.default_lut().tobytes()
    assert event_sim.default_lut(1e-2).tobytes() == R.default_lut(1e-2).tobytes()
    assert _lib.EVENT_SIM_CAP == R.CAP and event_sim.min_threshold(R.default_lut()) == 1776 == R.min_threshold(R.default_lut())
    # the cap condition
    event_sim.check_cap(R.default_lut(), 1776)
    with pytest.raises(RefidHipError, match="smallest threshold 1775 .* 256 events .* at least 1776"):
        event_sim.check_cap(R.default_lut(), 1775)
    with pytest.raises(RefidHipError, match="at least 1"):
        event_sim.check_cap(R.default_lut(), 0)
    with pytest.raises(RefidHipError, match="at least 1776"):
        event_sim.EventSimulator(4, 4, c_pos=0.2, c_neg=1775 / 65536, device="cpu")   # refused before the device is looked at
    with pytest.raises(RefidHipError, match="a GPU device is required"):
        event_sim.EventSimulator(4, 4, device="cpu")
    # threshold maps
    assert event_sim.threshold_maps(4, 6, 0.2, 0.3) == (13107, 19661)
    a = event_sim.threshold_maps(4, 6, 0.2, 0.3, sigma=0.05, seed=3)
    b = event_sim.threshold_maps(4, 6, 0.2, 0.3, sigma=0.05, seed=3)
    c = event_sim.threshold_maps(4, 6, 0.2, 0.3, sigma=0.05, seed=4)
    assert a[0].dtype == np.int32 and a[0].shape == (4, 6) and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[0].tobytes() != c[0].tobytes() and a[0].tobytes() != a[1].tobytes()
    wide = event_sim.threshold_maps(16, 16, 0.05, 0.05, sigma=1.0, seed=0)
    assert min(wide[0].min(), wide[1].min()) == event_sim.to_fixed(event_sim.DEFAULT_FLOOR) >= 1776
    with pytest.raises(RefidHipError, match="sigma"):
        event_sim.threshold_maps(4, 4, 0.2, 0.2, sigma=-1.0)
    with pytest.raises(RefidHipError, match="c_neg"):
        event_sim.threshold_maps(4, 4, 0.2, 0.0)
    # the .npz round trip
    lut = R.default_lut()
    frames = _noise(10, 4, 6, 8)
    frames[2] = frames[1]                                             # an interval without events: an empty file
    rows, offsets, _, _ = R.simulate(frames, 1e9 + np.arange(4.0), R.reset(frames[0], lut), lut, 3000, 3000)
    paths = event_sim.save_event_npz(str(tmp_path / "events"), rows, offsets)
    assert [p[-10:] for p in paths] == ["000000.npz", "000001.npz", "000002.npz"] and offsets[1] == offsets[2]
    z = np.load(paths[0])
    assert (z["x"].dtype, z["y"].dtype, z["timestamp"].dtype, z["polarity"].dtype) == (np.uint16, np.uint16, np.float32, np.int8)
    back = sequence.load_event_npz(sorted(paths))
    assert back.dtype == np.float32 and back.tobytes() == rows.tobytes()
    with pytest.raises(RefidHipError, match="offsets"):
        event_sim.save_event_npz(str(tmp_path / "bad"), rows, offsets[:-1])
