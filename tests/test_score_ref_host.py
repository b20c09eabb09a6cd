"""CPU-only: the numpy restatement of the scoring contract (tests/score_ref.py) against what the reference's own
``calculate_psnr`` / ``calculate_ssim`` recorded in tests/golden/score.npz (tools/make_score_golden.py).

Bars (per frame of every fixture entry):
  cropped RGB PSNR   |d| < 1e-9 dB: the numerator is an integer sum, the rest a handful of float64 operations.
  PSNR on Y          |d| <= 1e-4 dB: the reference's value is a float32 -- its MSE is a float32 pairwise np.mean (relative
                     error at most about 1e-5 for up to 1e6 non-negative terms: 4.3e-5 dB), its log10 and division round
                     in float32 (up to 3 ulp of at most 128 dB: 2.3e-5 dB).  Measured: score_ref.MEASURED_PSNR_Y_ABS.
  SSIM on Y          |d| <= 1e-12: measured 2.2e-16 against the scipy stand-in; the margin is for a summation order
                     inside cv2 that nobody here can observe."""
import functools
import math
import os

import numpy as np
import pytest

import score_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score.npz")
PSNR_BAR, PSNR_Y_BAR, SSIM_Y_BAR = 1e-9, 1e-4, 1e-12


@functools.lru_cache(maxsize=None)
def _golden():
    z = np.load(GOLDEN)
    entries = [e.split() for e in z["entries"].tolist()]
    return {k: z[k] for k in z.files}, [(n, g, p, int(cb)) for n, g, p, cb in entries]


ENTRY_NAMES = ["c0_noise", "c0_pm2", "c0_flip", "c1_noise", "c1_pm2", "c1_flip", "c2_noise", "c2_pm2", "c2_flip", "c3_noise",
               "c3_pm2", "c3_flip", "identical", "flat_vs_noise"]


def test_fixture_holds_the_cases():
    arrays, entries = _golden()
    assert [e[0] for e in entries] == ENTRY_NAMES
    shapes = {e[0]: arrays[e[1]].shape[:3] + (e[3],) for e in entries}
    assert shapes["c0_noise"] == (1, 7, 9, 0) and shapes["c1_pm2"] == (1, 17, 16, 0)
    assert shapes["c2_flip"] == (1, 23, 37, 3) and shapes["c3_noise"] == (3, 40, 50, 4)
    for name, gk, pk, cb in entries:
        assert arrays[gk].dtype == np.uint8 and arrays[gk].shape == arrays[pk].shape
        assert arrays[f"ref_{name}"].shape == (arrays[gk].shape[0], 3)
    assert int((arrays["c2_gt"] != arrays["c2_flip"]).sum()) == 1            # one bit in one green value
    d = arrays["c3_gt"].astype(int) - arrays["c3_pm2"].astype(int)
    assert set(np.unique(np.abs(d)).tolist()) <= {0, 1, 2}                   # gt +- 2 (clipped at the ends of the range)
    assert os.path.getsize(GOLDEN) < 100 * 1024


@pytest.mark.parametrize("name", ENTRY_NAMES)
def test_restatement_against_the_reference(name):
    arrays, entries = _golden()
    _, gk, pk, cb = next(e for e in entries if e[0] == name)
    ref = arrays[f"ref_{name}"]
    for f, (g, p) in enumerate(zip(arrays[gk], arrays[pk])):
        ours = R.scores(R.frame_stages(p, g, bgr=True, crop_border=cb))
        print(f"{name}[{f}]: psnr {ours[0]:.9f} (ref {ref[f, 0]:.9f}), psnr_y {ours[1]:.9f} (ref {ref[f, 1]:.9f}), "
              f"ssim_y {ours[2]:.15f} (ref {ref[f, 2]:.15f})")
        for k, bar in enumerate((PSNR_BAR, PSNR_Y_BAR, SSIM_Y_BAR)):
            if math.isinf(ref[f, k]):
                assert ours[k] == ref[f, k]
            elif k == 0:
                assert abs(ours[k] - ref[f, k]) < bar
            else:
                assert abs(ours[k] - ref[f, k]) <= bar


def test_identical_frames_and_the_measured_constants():
    arrays, _ = _golden()
    g = arrays["c2_gt"][0]
    st = R.frame_stages(g, g, bgr=True, crop_border=3)
    assert st["sq_rgb"] == 0 and not st["sq_y_terms"].any()
    assert np.all(st["ssim_y_map"] == 1.0)                                  # numerator and denominator are the same bits
    assert R.scores(st) == (float("inf"), float("inf"), 1.0)
    assert R.MEASURED_PSNR_ABS < PSNR_BAR and R.MEASURED_PSNR_Y_ABS <= PSNR_Y_BAR and R.MEASURED_SSIM_Y_ABS <= SSIM_Y_BAR
    assert R.C1 == (0.01 * 255) * (0.01 * 255) and R.C2 == (0.03 * 255) * (0.03 * 255)   # what csrc/score.hip computes


def test_y_plane_is_niqes():
    """The Y plane is NIQE's, bit for bit, where NIQE defines one (whole 96x96 blocks), in both channel orders and cropped."""
    import niqe_ref
    rng = np.random.Generator(np.random.PCG64(5))
    u8 = rng.integers(0, 256, (102, 198, 3), dtype=np.uint8)
    for bgr in (False, True):
        assert R.y_plane(u8, bgr, 3).tobytes() == niqe_ref.y_plane(u8, bgr, 3).tobytes()
    assert R.y_plane(u8[:96, :96], True).tobytes() != R.y_plane(u8[:96, :96], False).tobytes()


def test_window_and_filter():
    win = R.window()
    assert win.shape == (11, 11) and abs(win.sum() - 1.0) < 1e-15 and np.array_equal(win, win.T)
    x = np.full((7, 9), 3.25)
    assert np.allclose(R.filter121(x, win), 3.25, rtol=0, atol=1e-14)        # every tap clamped: a constant stays
    rng = np.random.Generator(np.random.PCG64(6))
    x = rng.standard_normal((13, 12))
    p = np.pad(x, 5, mode="edge")
    want = sum(win[i, j] * p[i + 4, j + 6] for i in range(11) for j in range(11))
    assert abs(R.filter121(x, win)[4, 6] - want) < 1e-14
    assert R.sq_rgb(np.zeros((4, 4, 3), np.uint8), np.full((4, 4, 3), 255, np.uint8), 1) == 2 * 2 * 3 * 255 * 255
