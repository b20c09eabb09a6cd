"""CPU-only: tests/edi_ref.py, the restatement of "Double integral" in include/refid_hip.h, against closed forms, its tie and
sign conventions, the gain tables against ``numpy.exp``, and the simulator's closed loop: events from event_sim_ref and
blurry key frames from blur_ref, inverted, must beat the blurry key frame on every frame -- and lose to it on every frame
once the polarities are flipped."""
import json
import math
import os

import numpy as np
import pytest

import blur_ref
import edi_ref as R
import event_sim_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = R.to_fixed(0.2)
EPS255 = 255.0 * 1e-3


def _frames(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)


def _rows(rows):
    return np.array(sorted(rows), dtype=np.float32).reshape(-1, 4)


def _run(frames, rows, items, bounds, instants, m=1, exposure=R.SAMPLES, c_pos=C, c_neg=C):
    h, w = frames.shape[1:3]
    return R.edi(frames, R.load(_rows(rows), h, w), items, bounds, instants, m, exposure, c_pos, c_neg)


def test_no_events_blend_and_identity():
    frames = _frames(2, 3, 5, 1)
    frames[1] = (frames[0].astype(int) // 4 * 4 + 8 * (np.arange(15).reshape(3, 5, 1) % 5) - 16).clip(0, 252).astype(np.uint8)
    frames[0] = frames[0] // 4 * 4                              # differences are multiples of 4: quarter blends are integers
    tau = R.output_instants("sharp", (1.0, 1.0, 2.0, 2.0), n=3)
    assert tau.tolist() == [1.25, 1.5, 1.75]
    out, held = _run(frames, [], [[0, 1]], [[1.0, 1.0, 2.0, 2.0]], [tau])
    a, b = frames[0].astype(np.float64), frames[1].astype(np.float64)
    for f, w in enumerate((0.25, 0.5, 0.75)):
        assert np.array_equal(out[0, f], np.rint((1 - w) * a + w * b).astype(np.uint8))
    assert held == 0
    for exposure in (R.SAMPLES, R.CONTINUOUS):                  # a single key: the key frame exactly, blurry or not
        out, _ = _run(frames, [], [[1, -1]], [[1.0, 3.0, 0.0, 0.0]], [[2.0]], m=5, exposure=exposure)
        assert np.array_equal(out[0, 0], frames[1])


def test_one_event_in_mid_exposure_against_the_closed_form():
    """One positive event at t = 1.25 of the exposure [1, 2] at pixel (x 2, y 1), M = 5 samples at 1, 1.25, .. 2: the sample at
    1.25 counts it, so S = (1 + 4 g) / 5; for a continuous shutter S = 0.25 + 0.75 g.  Latent before the event (B + e) / S - e,
    after it (B + e) g / S - e."""
    frames = _frames(1, 2, 4, 2)
    g = math.exp(C / 65536.0)
    for exposure, norm in ((R.SAMPLES, (1 + 4 * g) / 5), (R.CONTINUOUS, 0.25 + 0.75 * g)):
        out, held = _run(frames, [(1.25, 2, 1, 1)], [[0, -1]], [[1.0, 2.0, 0, 0]], [[1.0, 1.125, 1.25, 2.0]], m=5, exposure=exposure)
        b = frames[0].astype(np.float64) + EPS255
        assert held == 0
        for f, gain in enumerate((1.0, 1.0, g, g)):
            want = b.copy()
            want[1, 2] = b[1, 2] * gain / norm
            assert np.array_equal(out[0, f], np.clip(np.rint(want - EPS255), 0, 255).astype(np.uint8)), (exposure, f)
        assert out[0, 0, 1, 2, 0] != out[0, 3, 1, 2, 0] or frames[0, 1, 2, 0] < 4


def test_ties_and_events_outside_the_item():
    frames = np.full((2, 1, 2, 3), 100, dtype=np.uint8)
    g = math.exp(C / 65536.0)
    lat = lambda gain: int(np.clip(np.rint((100 + EPS255) * gain - EPS255), 0, 255))      # noqa: E731
    bounds, tau = [[1.0, 1.0, 2.0, 2.0]], [[1.0, 1.5, 2.0]]
    # an event exactly at s0 is not the item's; one before it neither
    out, _ = _run(frames, [(1.0, 0, 0, 1), (0.5, 0, 0, 1)], [[0, 1]], bounds, tau)
    assert out[0, :, 0, 0, 0].tolist() == [100, 100, 100]
    # an event exactly at tau counts towards tau
    out, _ = _run(frames, [(1.5, 0, 0, 1)], [[0, -1]], [[1.0, 1.0, 0, 0]], [[1.0]])
    assert out[0, 0, 0, 0, 0] == 100
    out, _ = _run(frames, [(1.5, 0, 0, 1)], [[0, -1]], [[1.0, 2.0, 0, 0]], [[1.25, 1.5]], exposure=R.CONTINUOUS)
    s = 0.5 + 0.5 * g
    assert out[0, :, 0, 0, 0].tolist() == [lat(1 / s), lat(g / s)]
    # an event exactly at e1 = s1 counts: the right key, stamped there, already holds it, so it is undone towards the left
    out, _ = _run(frames, [(2.0, 0, 0, 1)], [[0, 1]], bounds, [[1.5, 2.0]])
    assert out[0, :, 0, 0, 0].tolist() == [int(np.rint(0.5 * (100 + EPS255) + 0.5 * (100 + EPS255) / g - EPS255)), lat(1.0)]
    assert out[0, 0, 0, 0, 0] < 100
    assert out[0, 0, 0, 1, 0] == 100                            # (the other pixel has no events)
    # an event after e1 is ignored, in either mode
    for exposure in (R.SAMPLES, R.CONTINUOUS):
        out, _ = _run(frames, [(2.5, 0, 0, 1)], [[0, 1]], [[1.0, 1.25, 1.75, 2.0]], [[1.0, 1.5, 2.0]], m=3, exposure=exposure)
        assert out[0, :, 0, 0, 0].tolist() == [100, 100, 100]


def test_zero_polarity_is_negative_and_the_thresholds_differ():
    frames = np.full((1, 1, 3, 3), 100, dtype=np.uint8)
    cp, cn = R.to_fixed(0.3), R.to_fixed(0.1)
    out, _ = _run(frames, [(1.5, 0, 0, 1), (1.5, 1, 0, 0), (1.5, 2, 0, -1)], [[0, -1]], [[1.0, 2.0, 0, 0]], [[2.0]], c_pos=cp, c_neg=cn)
    up = int(np.rint((100 + EPS255) * math.exp(cp / 65536.0) - EPS255))
    down = int(np.rint((100 + EPS255) * math.exp(-cn / 65536.0) - EPS255))
    assert out[0, 0, 0, :, 0].tolist() == [up, down, down] and up - 100 > 3 * (100 - down) - 4
    # a pixel that oscillates comes back exactly when the thresholds agree, and drifts by the difference when they do not
    swing = [(1.0 + 0.001 * k, 0, 0, 1 if k % 2 == 0 else -1) for k in range(1, 2001)]
    out, _ = _run(frames, swing, [[0, -1]], [[1.0, 4.0, 0, 0]], [[4.0]])
    assert out[0, 0, 0, 0, 0] == 100
    out, _ = _run(frames, swing, [[0, -1]], [[1.0, 4.0, 0, 0]], [[4.0]], c_pos=cn + 1, c_neg=cn)
    assert out[0, 0, 0, 0, 0] == int(np.rint((100 + EPS255) * math.exp(1000 / 65536.0) - EPS255)) == 102


def test_rows_outside_the_frame_are_dropped_and_coordinates_truncate():
    rows = _rows([(1.0, -0.5, 0.9, 1), (1.1, 3.99, 1.2, 1), (1.2, 4.0, 0, 1), (1.3, 0, 2, 1), (1.4, -1.0, 0, 1), (1.5, float("nan"), 0, 1)])
    by_pixel, dropped = R.load(rows, 2, 4)
    assert dropped == 4 and sorted(by_pixel) == [0, 7]
    assert by_pixel[0][0].tolist() == [1.0] and by_pixel[7][0].tolist() == [np.float32(1.1)]


def test_the_clamp_and_its_flag():
    frames = np.full((1, 1, 2, 3), 10, dtype=np.uint8)
    hot = [(1.0 + 1e-4 * k, 0, 0, 1) for k in range(1, 5001)]          # 5000 events of 0.2: level 1000, held at 32
    cold = [(1.0 + 1e-4 * k, 1, 0, -1) for k in range(1, 5001)]
    out, held = _run(frames, hot + cold, [[0, -1]], [[1.0, 3.0, 0, 0]], [[1.2, 3.0]])
    assert held == 2 and out[0, :, 0, 0, 0].tolist() == [255, 255] and out[0, :, 0, 1, 0].tolist() == [0, 0]
    g, cl = R.gain(np.array([R.CLAMP << 16, (R.CLAMP << 16) + 1, -(R.CLAMP << 16), -(R.CLAMP << 16) - 1, 0]), R.gain_tables())
    assert cl.tolist() == [False, True, False, True, False]
    assert g[0] == g[1] == np.exp(32.0) and g[2] == g[3] == np.exp(-32.0) and g[4] == 1.0
    out, held = _run(frames, hot[:100], [[0, -1]], [[1.0, 3.0, 0, 0]], [[3.0]])      # level 20: large, but not held
    assert held == 0


def test_the_tables_against_numpy_exp():
    """Every level the gain takes, all 4 194 305 integers inside +-32 * 2^16, against ``numpy.exp`` of the same level.  Measured:
    the largest distance is exactly 3.0 ulp (of the numpy value), the mean 0.56 ulp; the bound asserted is that measured
    maximum.  (An a-priori bound would be 5: three entries within 1 ulp each, two roundings of half an ulp, numpy's own ulp.)"""
    tables = R.gain_tables()
    assert tables.shape == (R.TABLE,) and tables[R.CLAMP] == 1.0 and tables[2 * R.CLAMP + 1] == 1.0 and tables[2 * R.CLAMP + 257] == 1.0
    levels = np.arange(-(R.CLAMP << 16), (R.CLAMP << 16) + 1, dtype=np.int64)
    g, cl = R.gain(levels, tables)
    want = np.exp(levels.astype(np.float64) / 65536.0)
    ulps = np.abs(g - want) / np.spacing(want)
    print(f"gain tables against numpy.exp over {len(levels)} levels: max {ulps.max()} ulp, mean {ulps.mean():.3f} ulp")
    assert not cl.any() and ulps.max() <= 3.0, ulps.max()
    assert ulps.mean() <= 0.6, ulps.mean()
    assert g[R.CLAMP << 16] == 1.0
    assert np.all(np.diff(R.gain(np.arange(-300000, 300000, 7), tables)[0]) > 0)      # monotone across the table seams


def test_sample_and_output_instants():
    assert R.sample_instants(1.0, 2.0, 5).tolist() == [1.0, 1.25, 1.5, 1.75, 2.0]
    assert R.sample_instants(3.0, 7.0, 1).tolist() == [3.0] and R.sample_instants(3.0, 3.0, 4).tolist() == [3.0] * 4
    s = R.sample_instants(0.1, 0.3, 64)
    assert s.dtype == np.float32 and s[0] == np.float32(0.1) and s[-1] == np.float32(0.3) and np.all(np.diff(s) > 0)
    assert R.output_instants("single", (1.0, 2.0, 0, 0)).tolist() == [1.5]
    assert R.output_instants("blur", (0.0, 2.0, 4.0, 6.0), m=3, n=1).tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    from refid_amd import edi
    for args in (("sharp", (0.1, 0.1, 0.7, 0.7), 1, 7), ("blur", (0.1, 0.2, 0.3, 0.45), 11, 1), ("single", (0.1, 0.2, 0, 0), 1, None)):
        assert np.array_equal(R.output_instants(*args), edi.output_instants(*args))
    assert np.array_equal(R.sample_instants(0.1, 0.3, 11), edi.sample_instants(0.1, 0.3, 11))
    assert np.array_equal(R.gain_tables(), edi.gain_tables())
    for c in (2.0 ** -16, 0.0271, 0.05, 0.1, 0.17, 0.2, 0.3, 1.0, 1.5 * 2.0 ** -16, 2.5 * 2.0 ** -16, 15.99999, 16.0):
        assert R.to_fixed(c) == edi.to_fixed(c), c             # (the restatement's copy of event_sim.to_fixed; ties go to even)


# ---- the closed loop: clip -> events + blurry key frames -> double integral -> the clip's frames ----

def _clip(n=23, h=48, w=64, speed=1.5):
    """A smooth texture that moves ``speed`` pixels per frame to the right."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for k in range(n):
        u = x - speed * k
        v = 0.5 + 0.25 * np.sin(2 * np.pi * u / 17.0) * np.cos(2 * np.pi * y / 23.0) + 0.2 * np.sin(2 * np.pi * (u + 2 * y) / 41.0)
        rgb = np.stack([v, 0.9 * v + 0.05, 0.8 * v + 0.1], axis=-1)
        out.append(np.rint(255.0 * np.clip(rgb, 0, 1)).astype(np.uint8))
    return np.stack(out)


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


@pytest.fixture(scope="module")
def clip():
    frames = _clip()
    stamps = np.arange(len(frames), dtype=np.float64) / 240.0
    return frames, stamps


def _closed_loop(clip, c, firsts, flip=False, shift=0, m=11):
    """PSNR gains over the blurry key frame, one per recovered frame, of the windows starting at ``firsts``."""
    frames, stamps = clip
    cf = R.to_fixed(c)
    lut = S.default_lut()
    rows, _, _, over = S.simulate(frames, stamps, S.reset(frames[0], lut), lut, cf, cf)
    assert not over
    if flip:
        rows = rows.copy()
        rows[:, 3] = -rows[:, 3]
    windows = np.array([[f, m] for f in firsts], dtype=np.int32)
    keys = blur_ref.blur_synth(frames, windows)
    expo = blur_ref.exposures(stamps, windows)
    bounds = np.array([[s - shift / 240.0, e - shift / 240.0, 0, 0] for s, e in expo], dtype=np.float32)
    instants = np.stack([R.sample_instants(b[0], b[1], m) for b in bounds])
    out, _ = R.edi(keys, R.load(rows, *frames.shape[1:3]), [[k, -1] for k in range(len(firsts))], bounds, instants, m, R.SAMPLES, cf, cf)
    return [[_psnr(out[k, j], frames[f + j]) - _psnr(keys[k], frames[f + j]) for j in range(m)] for k, f in enumerate(firsts)]


def test_the_closed_loop_beats_the_blurry_frame_and_a_flipped_stream_loses_to_it(clip):
    record = {"clip": "48x64 smooth texture, 1.5 px/frame, 23 frames at 240 fps, M = 11, code-domain blur, windows at frames 0 and 6",
              "unit": "dB of PSNR over the blurry key frame against the same sharp frame, per recovered frame"}
    for c in (0.05, 0.1):
        gains = np.array(_closed_loop(clip, c, (0, 6)))
        record[f"c={c}"] = {"min": round(float(gains.min()), 2), "max": round(float(gains.max()), 2), "mean": round(float(gains.mean()), 2)}
        assert np.all(gains > 0), (c, gains)
    gains = np.array(_closed_loop(clip, 0.1, (0, 6), flip=True))
    record["c=0.1, polarities flipped"] = {"min": round(float(gains.min()), 2), "max": round(float(gains.max()), 2),
                                          "mean": round(float(gains.mean()), 2)}
    assert np.all(gains < 0), gains
    gains = np.array(_closed_loop(clip, 0.2, (0, 6)))                  # measured only: the model itself misses single frames here
    record["c=0.2 (not asserted)"] = {"min": round(float(gains.min()), 2), "max": round(float(gains.max()), 2),
                                     "mean": round(float(gains.mean()), 2)}
    gains = np.array(_closed_loop(clip, 0.05, (6,), shift=3))
    record["c=0.05, events three frames late (not asserted)"] = {"min": round(float(gains.min()), 2), "max": round(float(gains.max()), 2),
                                                                "mean": round(float(gains.mean()), 2)}
    with open(os.path.join(ROOT, "profiles", "edi_closed_loop.json")) as f:
        kept = json.load(f)
    print(json.dumps(record, indent=1))
    assert sorted(kept) == sorted(record), json.dumps(record, indent=1)
    # The kept figures of the ASSERTED cases are these: one pixel that moves by one code (an exp that differs in its last bit
    # between numpy builds) changes a frame's PSNR by less than 0.01 dB, so 0.05 dB holds the file to its two decimals.  The
    # cases labelled "not asserted" are recorded for the reader and compared with nothing.
    for key in ("c=0.05", "c=0.1", "c=0.1, polarities flipped"):
        assert all(abs(kept[key][k] - v) <= 0.05 for k, v in record[key].items()), json.dumps(record, indent=1)
