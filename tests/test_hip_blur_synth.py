"""GPU: csrc/blur_synth.hip against tests/blur_ref.py, bit for bit -- both modes, frame sizes that are and are not multiples
of the kernel's 16-byte unit, misaligned bases on either side, overlapping and repeated windows, the longest window, the
launcher's stride loop -- and ``python -m refid_amd.simulate --blur`` end to end into the blur layout's assembler."""
import functools
import glob
import os

import numpy as np
import pytest

import blur_ref as R

pytestmark = pytest.mark.gpu

WINDOWS_9 = [[0, 1], [0, 2], [1, 3], [2, 7], [0, 9], [8, 1], [2, 7]]       # overlapping, one repeated, one on the last frame
WINDOWS_8 = [[0, 1], [0, 2], [1, 3], [1, 7], [0, 8], [7, 1], [1, 7]]       # the same pattern inside the 8 frames of frames[1:]
WINDOWS_6 = [[0, 1], [0, 2], [1, 3], [2, 4], [0, 6], [5, 1], [2, 4]]
MODES = ["plain", "gamma2.2"]


def _noise(seed, n, h, w):
    return np.random.default_rng(seed).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)


def _table(mode):
    return None if mode == "plain" else R.gamma_table(float(mode[5:]))


@functools.lru_cache(maxsize=None)
def _clip(name):
    """The host frames of a case; computed once and never written to."""
    frames = {"odd_17x35_n9": lambda: _noise(11, 9, 17, 35), "aligned_16x32_n6": lambda: _noise(12, 6, 16, 32),
              "two_tiles_40x40_n5": lambda: _noise(13, 5, 40, 40), "tiny_8x8_n9": lambda: _noise(14, 9, 8, 8)}[name]()
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def _want(name, windows, mode, skip=0):
    out = R.blur_synth(_clip(name)[skip:], np.array(windows, dtype=np.int32), _table(mode))
    out.setflags(write=False)
    return out


def _key(windows):
    return tuple(tuple(w) for w in windows)


def _run(frames, windows, mode, **kw):
    from refid_amd import ops
    return ops.blur_synth(frames, np.array(windows, dtype=np.int32), to_linear=_table(mode), **kw)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()               # (a copy: the shared host arrays are read-only)


@pytest.mark.parametrize("mode", MODES)
def test_an_odd_frame_size_equals_the_restatement(mode):
    """17 x 35 x 3 = 1785 bytes: no multiple of 16 (the general path; the last unit of a frame has 9 bytes) and odd, so the
    frames and the outputs behind the first start at every alignment."""
    got = _run(_dev(_clip("odd_17x35_n9")), WINDOWS_9, mode)
    assert str(got.dtype) == "torch.uint8" and tuple(got.shape) == (7, 17, 35, 3)
    assert got.cpu().numpy().tobytes() == _want("odd_17x35_n9", _key(WINDOWS_9), mode).tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_an_aligned_frame_size_equals_the_restatement_on_both_paths(mode):
    """16 x 32 x 3 = 1536 bytes: the 16-byte path.  The same frames at a base 3 bytes into a buffer take the general path
    and must give the same bytes."""
    import torch
    host = _clip("aligned_16x32_n6")
    want = _want("aligned_16x32_n6", _key(WINDOWS_6), mode).tobytes()
    frames = _dev(host)
    assert frames.data_ptr() % 16 == 0
    assert _run(frames, WINDOWS_6, mode).cpu().numpy().tobytes() == want
    buf = torch.zeros((host.size + 16,), dtype=torch.uint8, device="cuda")
    shifted = buf[3:3 + host.size].view(host.shape)
    shifted.copy_(frames)
    assert shifted.data_ptr() % 16 == 3 and shifted.is_contiguous()
    assert _run(shifted, WINDOWS_6, mode).cpu().numpy().tobytes() == want


@pytest.mark.parametrize("mode", MODES)
def test_a_slice_of_the_frames_moves_the_base_to_an_odd_offset(mode):
    frames = _dev(_clip("odd_17x35_n9"))[1:]
    assert frames.data_ptr() % 2 == 1 and frames.is_contiguous()
    got = _run(frames, WINDOWS_8, mode)
    assert got.cpu().numpy().tobytes() == _want("odd_17x35_n9", _key(WINDOWS_8), mode, 1).tobytes()


@pytest.mark.parametrize("name,windows", [("odd_17x35_n9", WINDOWS_9), ("aligned_16x32_n6", WINDOWS_6)])
@pytest.mark.parametrize("mode", MODES)
def test_out_at_a_byte_offset_leaves_its_surroundings(name, windows, mode):
    host = _clip(name)
    size = len(windows) * host[0].size
    pattern = (np.arange(size + 64) * 7 + 5).astype(np.uint8)
    buf = _dev(pattern)
    out = buf[3:3 + size]
    assert out.data_ptr() % 16 == 3
    got = _run(_dev(host), windows, mode, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (len(windows),) + host.shape[1:]
    after = buf.cpu().numpy()
    assert after[3:3 + size].tobytes() == _want(name, _key(windows), mode).tobytes()
    assert after[:3].tobytes() == pattern[:3].tobytes() and after[3 + size:].tobytes() == pattern[3 + size:].tobytes()
    from refid_amd._lib import RefidHipError
    with pytest.raises(RefidHipError, match="out must be a contiguous uint8 tensor of"):
        _run(_dev(host), windows, mode, out=buf[:size - 1])


@pytest.mark.parametrize("mode", MODES + ["gamma1.0", "gamma3.0"])
def test_the_longest_window(mode):
    """8 x 8, 64 frames: all white (the largest sum the contract allows, 64 * 2^24 + 32 in response mode), and random codes."""
    white = np.full((64, 8, 8, 3), 255, dtype=np.uint8)
    got = _run(_dev(white), [[0, 64]], mode).cpu().numpy()
    assert got.tobytes() == white[:1].tobytes()
    noise = _noise(15, 64, 8, 8)
    windows = [[0, 64], [0, 63], [1, 63], [31, 33]]
    got = _run(_dev(noise), windows, mode).cpu().numpy()
    assert got.tobytes() == R.blur_synth(noise, windows, _table(mode)).tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_the_stride_loop_takes_a_second_pass(mode):
    """The launcher caps the grid at 4096 workgroups, a tile (256 units of 16 bytes of one window) each per pass.  An 8 x 8
    frame is one tile, so 4100 windows are 4100 tiles: the last four are a second pass of four workgroups.  Then the cap
    lowered through ``max_groups``: 7 one-tile windows on 2 workgroups (four passes), and 40 x 40 frames (4800 bytes, 300
    units: two tiles per window, the second one short) on 4 workgroups."""
    rng = np.random.default_rng(16)
    first = rng.integers(0, 9, size=4100)
    windows = np.stack([first, rng.integers(1, 10 - first)], axis=1).astype(np.int32)
    host = _clip("tiny_8x8_n9")
    got = _run(_dev(host), windows, mode).cpu().numpy()
    assert got.tobytes() == R.blur_synth(host, windows, _table(mode)).tobytes()
    got = _run(_dev(_clip("odd_17x35_n9")), WINDOWS_9, mode, max_groups=2).cpu().numpy()
    assert got.tobytes() == _want("odd_17x35_n9", _key(WINDOWS_9), mode).tobytes()
    windows = [[0, 5], [1, 2], [4, 1]]
    for cap in (4, 1, 0):
        got = _run(_dev(_clip("two_tiles_40x40_n5")), windows, mode, max_groups=cap).cpu().numpy()
        assert got.tobytes() == _want("two_tiles_40x40_n5", _key(windows), mode).tobytes(), cap


def test_two_runs_are_identical():
    import torch
    frames = _dev(_clip("odd_17x35_n9"))
    for mode in MODES:
        a, b = _run(frames, WINDOWS_9, mode), _run(frames, WINDOWS_9, mode)
        assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)


@pytest.mark.parametrize("count", [1, 7, 64])
def test_identical_frames_return_the_frame(count):
    import torch
    frame = np.concatenate([np.arange(256, dtype=np.uint8), _noise(17, 1, 1, 65).reshape(-1)[:173]]).reshape(1, 11, 13, 3)    # every code
    frames = _dev(np.repeat(frame, count, axis=0))
    for mode in MODES + ["gamma1.0", "gamma3.0"]:
        got = _run(frames, [[0, count], [count - 1, 1]], mode)
        assert torch.equal(got[0], frames[0]) and torch.equal(got[1], frames[0]), mode


def _write_clip(directory, frames):
    from refid_amd import png
    os.makedirs(directory)
    for k, f in enumerate(frames):
        png.write_png(os.path.join(directory, f"{k:04d}.png"), f)


def _png_dir(directory):
    from refid_amd import png
    return {name: png.read_png(os.path.join(directory, name)) for name in sorted(os.listdir(directory))}


def test_the_command_line_with_blur_writes_what_the_blur_layout_reads(tmp_path):
    import torch
    from refid_amd import blur_synth, sequence, simulate
    frames = _clip("odd_17x35_n9")
    _write_clip(str(tmp_path / "clip"), frames)
    out, sharp = str(tmp_path / "sim"), str(tmp_path / "sharp")
    base = ["--frames", str(tmp_path / "clip"), "--fps", "240", "--chunk", "4"]
    assert simulate.main(base + ["--out", out, "--blur", "3", "--gap", "1"]) == 0
    assert simulate.main(base + ["--out", sharp, "--split", "2"]) == 0
    windows, first = R.blur_windows(9, 3, 1)
    assert windows.tolist() == [[0, 3], [4, 3]]                                      # K = 2: one pair
    want = R.blur_synth(frames, windows)
    keys = _png_dir(os.path.join(out, "keys"))
    assert list(keys) == ["000000.png", "000001.png"]
    assert all(keys[f"{i:06d}.png"].tobytes() == want[i].tobytes() for i in range(2))
    stamps = np.loadtxt(os.path.join(out, "stamps.txt"))
    assert stamps.tobytes() == (np.arange(9) / 240.0).tobytes()
    exposures = np.loadtxt(os.path.join(out, "key_stamps.txt"), ndmin=2)
    assert exposures.tobytes() == blur_synth.exposures(stamps, windows).tobytes() == R.exposures(stamps, windows).tobytes()
    assert exposures.tolist() == [[0.0, 2 / 240.0], [4 / 240.0, 6 / 240.0]]
    # gt/: the names SequenceInterpolator gives the 2 m + n = 7 outputs of pair 0; gt_mid/: the middle of each exposure
    runner_names = [os.path.basename(p) for p in sequence.SequenceInterpolator._paths(None, "", "000000", np.zeros((7, 1)))]
    gt = _png_dir(os.path.join(out, "gt"))
    assert list(gt) == runner_names == [f"000000_{f:02d}.png" for f in range(7)]
    assert all(gt[f"000000_{f:02d}.png"].tobytes() == frames[f].tobytes() for f in range(7))
    mid = _png_dir(os.path.join(out, "gt_mid"))
    assert list(mid) == ["000000.png", "000001.png"]
    assert mid["000000.png"].tobytes() == frames[1].tobytes() and mid["000001.png"].tobytes() == frames[5].tobytes()
    # the events do not depend on what is done with the key frames
    files = sorted(glob.glob(os.path.join(out, "events", "*.npz")))
    other = sorted(glob.glob(os.path.join(sharp, "events", "*.npz")))
    assert [os.path.basename(f) for f in files] == [os.path.basename(f) for f in other] == [f"{k:06d}.npz" for k in range(8)]
    events = sequence.load_event_npz(files)
    assert events.shape[0] > 0 and events.tobytes() == sequence.load_event_npz(other).tobytes()
    assert open(os.path.join(out, "stamps.txt")).read() == open(os.path.join(sharp, "stamps.txt")).read()
    # ... and the blur layout takes them: lq = key 0 | m - 1 bins | key 1 | m - 1 bins, padded to a multiple of 8
    pairs = sequence.make_pairs(events[:, 0], *sequence.exposure_windows(exposures[:, 0], exposures[:, 1]))
    assert len(pairs) == 1 and pairs[0].row1 > pairs[0].row0
    stack = np.stack([keys["000000.png"], keys["000001.png"]])
    batch = sequence.SequenceAssembler(3, 1, "blur").load(stack, events).assemble(pairs)
    lq = batch["lq"]
    assert tuple(lq.shape) == (1, 6 + 2 * 2, 24, 40)
    key0 = torch.from_numpy(want[0].astype(np.float32).transpose(2, 0, 1) / np.float32(255.0)).cuda()
    assert torch.equal(lq[0, :3, :17, :35], key0)


def test_the_command_line_with_even_blur_and_gamma(tmp_path, capsys):
    """--blur 2 --gap 0 --blur-gamma 2.2 --bgr: response mode, an even M (no gt_mid, and a line that says so), BGR frames
    (the channels are independent: the PNGs are the RGB order of the averaged frames)."""
    from refid_amd import simulate
    frames = _clip("odd_17x35_n9")
    np.save(str(tmp_path / "clip.npy"), frames)
    out = str(tmp_path / "sim")
    assert simulate.main(["--frames", str(tmp_path / "clip.npy"), "--fps", "240", "--out", out, "--blur", "2", "--gap", "0",
                          "--blur-gamma", "2.2", "--bgr"]) == 0
    windows, _ = R.blur_windows(9, 2, 0)
    want = R.blur_synth(frames, windows, R.gamma_table(2.2))[..., ::-1]
    keys = _png_dir(os.path.join(out, "keys"))
    assert len(keys) == 4 and all(keys[f"{i:06d}.png"].tobytes() == want[i].tobytes() for i in range(4))
    assert not os.path.exists(os.path.join(out, "gt_mid"))
    assert "no gt_mid: --blur 2 is even" in capsys.readouterr().out
    gt = _png_dir(os.path.join(out, "gt"))
    assert list(gt) == [f"{i:06d}_{f:02d}.png" for i in range(3) for f in range(4)]
    assert all(gt[f"{i:06d}_{f:02d}.png"].tobytes() == frames[2 * i + f][..., ::-1].tobytes() for i in range(3) for f in range(4))


def test_blur_of_one_frame_writes_the_key_frames_of_split(tmp_path):
    """--blur 1 --gap 1 against --split 2: the same keys/ files, byte for byte, and the same key frames' instants; gt/ holds
    the same PNG bytes for every frame both write -- the blur layout also restores its two key frames, so its pair i has
    frames 2i, 2i + 1, 2i + 2 under _00 .. _02, of which _01 is the sharp layout's one held-out frame _00."""
    from refid_amd import simulate
    _write_clip(str(tmp_path / "clip"), _clip("odd_17x35_n9"))
    blur, sharp = str(tmp_path / "blur"), str(tmp_path / "sharp")
    base = ["--frames", str(tmp_path / "clip"), "--fps", "240"]
    assert simulate.main(base + ["--out", blur, "--blur", "1", "--gap", "1"]) == 0
    assert simulate.main(base + ["--out", sharp, "--split", "2"]) == 0

    def raw(*parts):
        with open(os.path.join(*parts), "rb") as f:
            return f.read()

    names = [f"{i:06d}.png" for i in range(5)]
    assert sorted(os.listdir(os.path.join(blur, "keys"))) == sorted(os.listdir(os.path.join(sharp, "keys"))) == names
    assert all(raw(blur, "keys", n) == raw(sharp, "keys", n) for n in names)
    assert all(raw(blur, "gt_mid", n) == raw(sharp, "keys", n) for n in names)       # m = 1: the middle frame is the key
    assert sorted(os.listdir(os.path.join(blur, "gt"))) == [f"{i:06d}_{f:02d}.png" for i in range(4) for f in range(3)]
    for i in range(4):
        assert raw(blur, "gt", f"{i:06d}_01.png") == raw(sharp, "gt", f"{i:06d}_00.png")
        assert raw(blur, "gt", f"{i:06d}_00.png") == raw(sharp, "keys", names[i])
        assert raw(blur, "gt", f"{i:06d}_02.png") == raw(sharp, "keys", names[i + 1])
    mine, theirs = np.loadtxt(os.path.join(blur, "key_stamps.txt"), ndmin=2), np.loadtxt(os.path.join(sharp, "key_stamps.txt"))
    assert mine[:, 0].tobytes() == mine[:, 1].tobytes() == theirs.tobytes()
