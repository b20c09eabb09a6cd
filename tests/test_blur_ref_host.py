"""CPU-only: the restatement tests/blur_ref.py of csrc/blur_synth.hip against float64 arithmetic and against the properties
the contract states ("Blur synthesis" in include/refid_hip.h), and the host helpers of refid_amd.blur_synth against the
restatement: the response table, the reference's window indexing and the exposure stamps."""
import numpy as np
import pytest

import blur_ref as R


def _stack(rng, count, shape=(5, 7, 3)):
    return rng.integers(0, 256, size=(count,) + shape, dtype=np.uint8)


@pytest.mark.parametrize("count", [1, 2, 3, 11, 64])
def test_plain_mode_is_the_float64_mean_rounded_half_up(count):
    rng = np.random.default_rng(100 + count)
    stack = _stack(rng, count, (9, 13, 3))
    want = np.floor(stack.astype(np.float64).mean(0) + 0.5)                    # exact in float64: sums below 2^14, count <= 64
    got = R.blur_window(stack)
    assert got.dtype == np.uint8 and np.array_equal(got.astype(np.float64), want)
    flat = stack.reshape(count, -1)
    for b in (0, 17, flat.shape[1] - 1):
        assert R.blur_byte(flat[:, b]) == int(got.reshape(-1)[b])


def test_plain_mode_rounds_ties_up():
    for c in range(0, 255):
        assert R.blur_byte([c, c + 1]) == c + 1                                 # mean c + 1/2
    for c in range(0, 254):
        assert R.blur_byte([c, c, c, c + 2]) == c + 1                           # mean c + 1/2
        assert R.blur_byte([c, c, c + 2, c]) == c + 1
    pair = np.array([[10, 200, 254]], dtype=np.uint8)
    assert R.blur_window(np.concatenate([pair, pair + 1])).tolist() == [11, 201, 255]


@pytest.mark.parametrize("count", [1, 7, 64])
def test_identical_frames_return_the_frame_in_both_modes(count):
    frame = np.arange(256, dtype=np.uint8).reshape(16, 16)
    stack = np.repeat(frame[None], count, axis=0)
    assert np.array_equal(R.blur_window(stack), frame)
    for gamma in (1.0, 2.2, 3.0):
        table = R.gamma_table(gamma)
        assert np.array_equal(R.blur_window(stack, table), frame), gamma
        thr = R.thresholds(table)
        assert all(thr[c] <= int(table[c]) < thr[c + 1] for c in range(1, 255)) and thr[255] <= int(table[255])
    for code in (0, 1, 128, 254, 255):
        assert R.blur_byte([code] * count, R.gamma_table(2.2)) == code


def test_gamma_table_is_increasing_and_equal_to_the_modules():
    from refid_amd import blur_synth
    from refid_amd._lib import RefidHipError
    for gamma in (1.0, 2.2, 3.0):
        table = R.gamma_table(gamma)
        assert table.dtype == np.uint32 and table.shape == (256,)
        assert np.all(table[1:].astype(np.int64) > table[:-1].astype(np.int64)), gamma
        assert int(table[0]) == 0 and int(table[255]) == 2 ** 24 == R.LINEAR_ONE == blur_synth.LINEAR_ONE
        R.check_table(table)
        mine = blur_synth.gamma_table(gamma)
        assert mine.dtype == np.uint32 and np.array_equal(mine, table), gamma
    assert R.gamma_table(1.0).tolist() == [(2 * c * 2 ** 24 + 255) // 510 for c in range(256)]    # c 2^24 / 255 to the nearest, in ints
    for bad in (0.99, 3.01, 0.0, -2.2, float("nan"), float("inf"), "wide"):
        with pytest.raises(RefidHipError, match="gamma_table: gamma"):
            blur_synth.gamma_table(bad)


def test_response_mode_of_64_white_frames_does_not_overflow():
    table = R.gamma_table(2.2)
    stack = np.full((64, 3, 4, 3), 255, dtype=np.uint8)
    assert 64 * int(table[255]) + 32 < 2 ** 31
    assert np.array_equal(R.blur_window(stack, table), stack[0])
    assert R.blur_byte([255] * 64, table) == 255
    stack[63] = 254
    assert int(R.blur_window(stack, table).max()) == 255 and R.blur_byte([255] * 63 + [254], table) == 255


@pytest.mark.parametrize("gamma", [1.0, 2.2])
def test_response_mode_of_a_black_and_white_mix_is_the_float64_gamma_average(gamma):
    """The mean of the levels (c / 255)^gamma in float64, then the code whose level is nearest.  The integer form rounds
    each level to 2^-24 (error <= 3e-8), the mean to 2^-24 and each threshold to 2^-24, so the two may disagree only where
    the mean lies within 1e-6 of a threshold: such bytes are skipped, and they must be few.  (Gamma 3 is left out on
    purpose: its first thresholds, 3e-8 and 2.7e-7, lie within 1e-6 of the mean of an all-black byte.  With gamma 1 an even
    count that is exactly half white has the mean 1/2 = 127.5 / 255, which IS a threshold, so that table is tried with odd
    counts and with 64 frames far from half white.)"""
    rng = np.random.default_rng(7)
    table = R.gamma_table(gamma)
    level = (np.arange(256, dtype=np.float64) / 255.0) ** gamma
    thr = (level[:-1] + level[1:]) / 2.0                                          # thr[c], c = 1 .. 255
    checked = skipped = 0
    mixes = ((2, 0.5), (7, 0.3), (11, 0.5), (64, 0.1), (64, 0.5), (64, 0.9)) if gamma != 1.0 else \
        ((3, 0.5), (7, 0.3), (11, 0.5), (63, 0.5), (64, 0.1), (64, 0.9))
    for count, white in mixes:
        stack = np.where(rng.random((count, 24, 31, 3)) < white, 255, 0).astype(np.uint8)
        mean = level[stack].sum(axis=0) / count
        want = np.searchsorted(thr, mean, side="right")
        near = np.abs(thr[None, :] - mean.reshape(-1, 1)).min(axis=1).reshape(mean.shape) < 1e-6
        got = R.blur_window(stack, table)
        assert np.array_equal(got[~near], want[~near].astype(np.uint8)), (gamma, count, white)
        checked += int((~near).sum())
        skipped += int(near.sum())
    assert skipped < 0.01 * (checked + skipped), (skipped, checked)
    assert checked > 10000
    if gamma == 2.2:                                                              # half white is code 186, not 128: linear light
        assert R.blur_byte([0, 255], table) == 186 and R.blur_byte([0, 255]) == 128


def test_blur_windows_follow_the_reference_indexing():
    from refid_amd import blur_synth
    from refid_amd._lib import RefidHipError
    windows, first = blur_synth.blur_windows(29, 3, 2)
    assert windows.dtype == np.int32 and windows.shape == (6, 2)
    assert first.tolist() == [0, 5, 10, 15, 20, 25] and windows[:, 0].tolist() == first.tolist() and windows[:, 1].tolist() == [3] * 6
    for n_frames, m, n in ((29, 3, 2), (27, 3, 2), (28, 3, 2), (11, 11, 1), (240, 11, 1), (240, 11, 3), (64, 64, 0), (9, 3, 1), (5, 1, 0)):
        windows, first = blur_synth.blur_windows(n_frames, m, n)
        ref_windows, ref_first = R.blur_windows(n_frames, m, n)
        assert np.array_equal(windows, ref_windows) and first.tolist() == ref_first, (n_frames, m, n)
        assert len(first) == (n_frames - m) // (m + n) + 1
        assert int(windows[-1, 0] + windows[-1, 1]) <= n_frames < int(windows[-1, 0]) + m + n + m      # the last that fits
    assert blur_synth.blur_windows(7, 7, 3)[0].tolist() == [[0, 7]]                # N = m: one window
    with pytest.raises(RefidHipError, match="6 frames do not hold one blurry frame of m = 7"):
        blur_synth.blur_windows(6, 7, 3)
    with pytest.raises(ValueError):
        R.blur_windows(6, 7, 3)
    for m, n, word in ((0, 1, "m 0 must be 1 .. 64"), (65, 1, "m 65"), (3, -1, "n -1 must not be negative")):
        with pytest.raises(RefidHipError, match=word):
            blur_synth.blur_windows(100, m, n)


@pytest.mark.parametrize("n_frames,s", [(9, 2), (17, 8), (16, 8), (5, 4), (2, 2), (100, 7)])
def test_one_frame_windows_select_the_frames_of_split(n_frames, s):
    from refid_amd import blur_synth
    windows, first = blur_synth.blur_windows(n_frames, 1, s - 1)
    assert first.tolist() == list(range(0, n_frames, s))                          # the key frames of `simulate --split S`
    assert windows[:, 1].tolist() == [1] * len(first)


def test_exposures_are_the_stamps_of_the_first_and_last_frame():
    from refid_amd import blur_synth, sequence
    from refid_amd._lib import RefidHipError
    stamps = np.cumsum(np.random.default_rng(3).random(29) + 0.01)
    windows, first = blur_synth.blur_windows(29, 3, 2)
    e = blur_synth.exposures(stamps, windows)
    assert e.dtype == np.float64 and e.shape == (6, 2)
    assert np.array_equal(e[:, 0], stamps[first]) and np.array_equal(e[:, 1], stamps[first + 2])
    assert np.array_equal(e, R.exposures(stamps, windows))
    sharp, first = blur_synth.blur_windows(29, 1, 3)
    e = blur_synth.exposures(stamps, sharp)
    assert np.array_equal(e[:, 0], e[:, 1]) and np.array_equal(e[:, 0], stamps[first])
    mine, theirs = sequence.exposure_windows(e[:, 0], e[:, 1]), sequence.sharp_windows(stamps[first])
    assert all(np.array_equal(a, b) for a, b in zip(mine, theirs))                # m = 1: the sharp layout's windows
    with pytest.raises(RefidHipError, match="outside the 29 stamps"):
        blur_synth.exposures(stamps, [[27, 3]])
