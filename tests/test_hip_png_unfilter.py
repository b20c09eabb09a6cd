"""MI355X: refid_png_unfilter (csrc/png.hip) through ops.png_unfilter, sequence.load_png_frames and the command line.

Every comparison is exact equality of uint8 arrays: the kernel is integer arithmetic modulo 256 defined by the PNG
specification, so there is no tolerance anywhere.  The expected value is the ORIGINAL image the rows were filtered from
(tests/png_filter_ref.py, pinned to png.read_png by test_png_filter_ref_host.py) and, for shapes up to 65x33, also
png._unfilter of the same rows.  Shapes are the smallest at which the scheme can go wrong: no left neighbour / no row
above, one row past a 64-row wave and past the 256-row block, two block hand-overs on rows narrower than the skew, both
extents above 64, and rows of more 12-byte groups than the skew has steps.  For one shape all filter programmes and
data families go through ONE launch as a batch of frames, once per way of cutting bands."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import png_filter_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 3), (1, 7, 1), (2, 1, 3), (5, 3, 3), (63, 17, 3), (64, 9, 1), (65, 33, 3), (129, 5, 3), (130, 70, 1), (70, 130, 3),
          (200, 300, 3),
          # the kernel's block is 256 rows (four waves): one row past it, two block hand-overs on rows narrower than the
          # 256-thread skew, and rows of 1030 RGB pixels = 258 groups of 12 bytes, more than the 256 steps of the skew
          (257, 9, 3), (520, 5, 3), (300, 40, 1), (258, 1030, 3)]
STRESS = [4, 4, 0, 4, 3, 1, 2, 4, 1, 1, 3]      # bands (rows of type 0 / 1 start one) of 1..3 rows; row 63 and row 64 both start one
FAMILIES = ("random", "small", "all255", "checker", "ramp")
PROGRAMMES = ("all0", "all1", "all2", "all3", "all4", "random", "stress", "adaptive")


def _image(family, h, w, ch, rng):
    shape = (h, w, 3) if ch == 3 else (h, w)
    if family == "random":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if family == "small":                       # Paeth ties on almost every byte: the order a, b, c decides
        return rng.integers(0, 4, shape, dtype=np.uint8)
    if family == "all255":                      # every sum wraps modulo 256
        return np.full(shape, 255, dtype=np.uint8)
    yy, xx = np.indices((h, w))
    if family == "checker":
        plane = 254 + ((yy + xx) & 1)
    else:
        plane = (3 * xx + 5 * yy) & 255         # a ramp that wraps
    plane = plane if ch == 1 else plane[:, :, None] + np.arange(3) * (1 if family == "checker" else 40)
    return (plane & 255).astype(np.uint8) if family == "ramp" else np.minimum(plane, 255).astype(np.uint8)


def _types(programme, img, rng):
    h = img.shape[0]
    if programme.startswith("all"):
        return np.full(h, int(programme[3]))
    if programme == "random":
        return rng.integers(0, 5, h)
    return np.resize(STRESS, h) if programme == "stress" else R.adaptive_types(img)


@functools.lru_cache(maxsize=None)
def _case(h, w, ch):
    """Every programme x family of one shape as a batch: (names, images (N, H, W, 3), rows (N, H, 1 + W*ch)).  Built once.
    The one wide shape takes two families only: its frames are 0.8 MB each and the reference is numpy on the host."""
    rng = np.random.Generator(np.random.PCG64(1000 * h + 10 * w + ch))
    names, imgs, rows = [], [], []
    for family in (FAMILIES if w < 1000 else ("random", "small")):
        for programme in PROGRAMMES:
            img = _image(family, h, w, ch, rng)
            names.append(f"{family}/{programme}")
            rows.append(R.apply_filters(img, _types(programme, img, rng)))
            imgs.append(img if ch == 3 else np.repeat(img[:, :, None], 3, axis=2))
    imgs, rows = np.stack(imgs), np.stack(rows)
    imgs.setflags(write=False)
    rows.setflags(write=False)
    return names, imgs, rows


def _same(got, want, names, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.dtype, got.shape)
    for k, name in enumerate(names):
        if not np.array_equal(got[k], want[k]):
            bad = np.argwhere(got[k] != want[k])
            raise AssertionError(f"{what}: frame {k} ({name}): {len(bad)} bytes differ, first at (y, x, c) = {bad[0].tolist()}: "
                                 f"got {got[k][tuple(bad[0])]}, want {want[k][tuple(bad[0])]}")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_programme_and_family_decodes_to_the_original(shape):
    from refid_amd import ops, png
    h, w, ch = shape
    names, imgs, rows = _case(h, w, ch)
    n = len(names)
    dev = torch.from_numpy(rows.copy()).cuda()
    whole = ops.png_unfilter(dev, n, h, w, ch, split_bands=False)
    _same(whole, imgs, names, "one band per frame")
    split = ops.png_unfilter(dev, n, h, w, ch)                                   # split_bands=True: bands of >= 64 rows
    _same(split, imgs, names, "split_bands=True")
    finest = png.find_bands(rows[:, :, 0], min_rows=1)                           # every independent run its own band
    if h >= 64:
        stress = finest[finest[:, 0] == names.index("random/stress")]
        assert 1 in (stress[:, 2] - stress[:, 1]) and 63 in stress[:, 2] and 64 in stress[:, 2]
    fine = ops.png_unfilter(dev, n, h, w, ch, bands=finest)
    _same(fine, imgs, names, "bands of min_rows=1")
    assert torch.equal(whole, split) and torch.equal(whole, fine)                # the bytes do not depend on the bands
    if h <= 65 and w <= 33:                                                      # the project's own decoder on the same rows
        ref = np.stack([png._unfilter(r, ch).reshape(h, w, ch) for r in rows])
        _same(whole, np.repeat(ref, 3, axis=3) if ch == 1 else ref, names, "png._unfilter")


def test_a_batch_of_three_different_frames_in_one_launch():
    from refid_amd import ops
    rng = np.random.Generator(np.random.PCG64(77))
    imgs = [_image(f, 67, 21, 3, rng) for f in ("random", "small", "ramp")]
    types = [rng.integers(0, 5, 67), np.resize(STRESS, 67), R.adaptive_types(imgs[2])]
    rows = np.stack([R.apply_filters(i, t) for i, t in zip(imgs, types)])
    dev = torch.from_numpy(rows).cuda()
    for split in (True, False):
        got = ops.png_unfilter(dev, 3, 67, 21, 3, split_bands=split)
        _same(got, np.stack(imgs), ["random/random", "small/stress", "ramp/adaptive"], f"split_bands={split}")
    one = ops.png_unfilter(dev[1:2].contiguous(), 1, 67, 21, 3)                  # a frame's bytes do not depend on its place
    assert np.array_equal(one.cpu().numpy()[0], imgs[1])


@pytest.mark.parametrize("ch", [3, 1])
def test_out_is_a_view_and_its_neighbours_stay_untouched(ch):
    from refid_amd import ops
    h, w = 65, 33
    names, imgs, rows = _case(h, w, ch)
    pick = [names.index("random/random"), names.index("small/all4")]
    big = torch.full((4, h, w, 3), 0x5A, dtype=torch.uint8, device="cuda")
    flat = big.view(-1)
    view = big[1:3]
    got = ops.png_unfilter(torch.from_numpy(rows[pick].copy()).cuda(), 2, h, w, ch, out=view)
    assert got.data_ptr() == view.data_ptr()
    _same(big[1:3], imgs[pick], [names[i] for i in pick], "out view")
    per = h * w * 3
    assert bool((flat[:per] == 0x5A).all()) and bool((flat[3 * per:] == 0x5A).all())   # the guard frames before and after


def test_rejected_arguments():
    from refid_amd import _lib, ops
    rows = np.zeros((1, 3, 1 + 4 * 3), dtype=np.uint8)
    dev = torch.from_numpy(rows).cuda()
    with pytest.raises(_lib.RefidHipError, match="channels=2"):
        ops.png_unfilter(dev, 1, 3, 4, 2)
    with pytest.raises(_lib.RefidHipError, match="rows must be"):
        ops.png_unfilter(dev, 1, 3, 5, 3)
    with pytest.raises(_lib.RefidHipError, match="out must be"):
        ops.png_unfilter(dev, 1, 3, 4, 3, out=torch.empty((1, 3, 4, 3), dtype=torch.float32, device="cuda"))
    with pytest.raises(_lib.RefidHipError, match="exceed the kernel's line"):
        ops.png_unfilter(dev, 1, 1, _lib.PNG_MAX_ROW_BYTES // 3 + 1, 3)
    with pytest.raises(_lib.RefidHipError, match="a band lies outside"):
        ops.png_unfilter(dev, 1, 3, 4, 3, bands=np.array([[0, 0, 4]]))
    rows[0, 1, 0] = 5
    with pytest.raises(ValueError, match="read_png: unknown filter type 5 in row 1"):    # checked on the host: nothing launched
        ops.png_unfilter(torch.from_numpy(rows).cuda(), 1, 3, 4, 3)


def _smooth_frames(n, h, w, seed):
    """Smooth content plus a little noise: what makes an adaptive encoder choose Sub / Up / Average / Paeth rows."""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for k in range(n):
        base = 110 + 70 * np.sin((xx + 9 * k) / 11.0) + 50 * np.cos((yy - 4 * k) / 7.0)
        img = base[:, :, None] + np.array([0.0, 18.0, -25.0]) + rng.normal(0, 2.5, (h, w, 3))
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return np.stack(out)


def test_load_png_frames_equals_the_host_route(tmp_path):
    """5 files and frames_per_launch=2: a short last chunk, and both staging buffers are used twice."""
    from refid_amd import _lib
    from refid_amd.interpolate import load_frames
    from refid_amd.sequence import load_png_frames
    frames = _smooth_frames(5, 70, 130, 21)
    seen = set()
    for k, img in enumerate(frames):
        types = R.adaptive_types(img) if k != 3 else np.resize(STRESS, 70)
        seen |= set(types.tolist())
        R.write_filtered_png(str(tmp_path / "seq" / f"{k:03d}.png"), img, types)
    assert seen == {0, 1, 2, 3, 4}
    want = torch.from_numpy(load_frames(str(tmp_path / "seq")))
    assert np.array_equal(want.numpy(), frames)
    got = load_png_frames(str(tmp_path / "seq"), frames_per_launch=2)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (5, 70, 130, 3)
    assert torch.equal(got.cpu(), want)
    files = sorted(str(p) for p in (tmp_path / "seq").iterdir())
    assert torch.equal(load_png_frames(files, workers=2).cpu(), want)             # one chunk, one staging buffer
    grey = frames[:3, :, :, 1]
    for k, img in enumerate(grey):
        R.write_filtered_png(str(tmp_path / "grey" / f"{k}.png"), img, R.adaptive_types(img))
    assert torch.equal(load_png_frames(str(tmp_path / "grey"), frames_per_launch=2).cpu(),
                       torch.from_numpy(load_frames(str(tmp_path / "grey"))))
    R.write_filtered_png(str(tmp_path / "seq" / "005.png"), frames[0][:, :100], np.zeros(70, dtype=np.int64))
    with pytest.raises(_lib.RefidHipError, match="005.png"):
        load_png_frames(str(tmp_path / "seq"), frames_per_launch=2)


def test_the_command_line_decodes_a_png_directory_on_the_gpu(tmp_path):
    """python -m refid_amd.interpolate in a fresh child process on adaptively filtered PNGs writes the PNG bytes the same
    command gives, in process, on the .npy stack of those frames."""
    from oracle import refid_oracle as O
    from refid_amd import interpolate
    from test_sequence_host import TEST_YAML
    frames = _smooth_frames(3, 37, 50, 5)
    for k, img in enumerate(frames):
        types = R.adaptive_types(img)
        assert (types != 0).any()
        R.write_filtered_png(str(tmp_path / "frames" / f"{k:03d}.png"), img, types)
    np.save(tmp_path / "frames.npy", frames)
    rng = np.random.Generator(np.random.PCG64(6))
    n = 2000
    t = np.sort(rng.uniform(10.0, 30.0, n))
    np.savez(tmp_path / "e.npz", x=rng.integers(0, 50, n), y=rng.integers(0, 37, n), timestamp=t, polarity=rng.integers(0, 2, n) * 2 - 1)
    (tmp_path / "stamps.txt").write_text("10.0\n20.0\n30.0\n")
    (tmp_path / "t.yml").write_text(TEST_YAML.replace("num_inter_interpolation: 7", "num_inter_interpolation: 3"))
    torch.save({"params": O.make_params(6, base_num_channels=8, mode="hash", seed=3)}, tmp_path / "w.pth")
    common = ["--opt", str(tmp_path / "t.yml"), "--checkpoint", str(tmp_path / "w.pth"), "--events", str(tmp_path / "e.npz"),
              "--stamps", str(tmp_path / "stamps.txt")]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    child = subprocess.run([sys.executable, "-m", "refid_amd.interpolate", *common, "--frames", str(tmp_path / "frames"), "--out",
                            str(tmp_path / "out_png")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stdout + child.stderr
    assert interpolate.main([*common, "--frames", str(tmp_path / "frames.npy"), "--out", str(tmp_path / "out_npy")]) == 0
    names = sorted(os.listdir(tmp_path / "out_npy"))
    assert names == [f"{k:06d}_{f:02d}.png" for k in range(2) for f in range(3)] and sorted(os.listdir(tmp_path / "out_png")) == names
    for name in names:
        a, b = (tmp_path / "out_png" / name).read_bytes(), (tmp_path / "out_npy" / name).read_bytes()
        assert a == b, name
    assert len({(tmp_path / "out_npy" / name).read_bytes() for name in names}) == len(names)      # six different frames
