"""MI355X: refid_png_filter (csrc/png_filter.hip) through ops.png_filter, validation.FrameWriter and the command line.

Every comparison is exact equality of integer arrays: the kernel is integer arithmetic modulo 256 and integer sums, so
there is no tolerance anywhere.  The expected rows, filter types and cost sums are tests/png_filter_ref.py's
(``apply_filters`` / ``adaptive_types``, pinned to png.read_png and PIL by test_png_filter_ref_host.py).  One frame per
shape and data family; the nine families of a shape go through one launch as a batch.  Shapes: no left byte / no row above
(1x1, 1x7, 7x1, 2x3), rows shorter than a wave's 256-byte pass, several 4-row workgroups per frame (130x21), rows longer
than one pass (3x343: 1029 bytes, 5x1367: 4101 bytes); the odd pitch puts the rows of a batch at every byte offset."""
import functools
import os

import numpy as np
import pytest
import torch

import png_filter_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (7, 1), (2, 3), (17, 35), (40, 56), (64, 64), (65, 33), (130, 21), (3, 343), (5, 1367)]
FAMILIES = ("zeros", "all255", "noise", "hramp", "vramp", "diagonal", "waves", "checker", "blocks")


def _frame(family, h, w, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    chan = np.arange(3)
    if family == "zeros":
        img = np.zeros((h, w, 3))
    elif family == "all255":
        img = np.full((h, w, 3), 255.0)
    elif family == "noise":                      # uniform noise: the one family on which Average wins rows
        img = rng.integers(0, 256, (h, w, 3)).astype(np.float64)
    elif family == "hramp":                      # every row the same: Up leaves zeros
        img = (2 * xx)[:, :, None] + 30 * chan
    elif family == "vramp":                      # every column the same: Sub leaves zeros but for the first pixel, Paeth takes that from above
        img = (3 * yy)[:, :, None] + 30 * chan
    elif family == "diagonal":                   # a plane: Paeth predicts it; the noise keeps the sums apart
        img = (2 * xx + 3 * yy)[:, :, None] + 20 * chan + rng.integers(0, 3, (h, w, 3))
    elif family == "waves":
        img = (120 + 60 * np.sin(xx / 9.0) + 50 * np.cos(yy / 6.0))[:, :, None] + 15 * chan + rng.normal(0, 2.0, (h, w, 3))
    elif family == "checker":                    # 0 / 255: every difference wraps modulo 256 and reads as int8 +-1
        img = (255 * ((yy + xx) & 1))[:, :, None] + 0 * chan
    else:                                        # blocks: flat 8x8 blocks with hard edges
        img = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3))[yy // 8, xx // 8].astype(np.float64)
    return (np.rint(img).astype(np.int64) & 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _case(h, w):
    """One shape: frames (9, H, W, 3), and from the restatement the adaptive types (9, H), the cost sums (9, H, 5) and the
    rows of the five fixed modes and of the adaptive one, (6, 9, H, 1 + 3W).  Built once, read-only."""
    rng = np.random.Generator(np.random.PCG64(100 * h + w))
    frames = np.stack([_frame(f, h, w, rng) for f in FAMILIES])
    cand = np.stack([R._all_filtered(img) for img in frames])                            # (9, 5, H, 3W)
    costs = np.abs(cand.view(np.int8).astype(np.int64)).sum(axis=3).transpose(0, 2, 1)    # (9, H, 5)
    types = np.stack([R.adaptive_types(img) for img in frames])
    assert np.array_equal(types, costs.argmin(axis=2))
    rows = np.stack([np.stack([R.apply_filters(img, np.full(h, t) if t < 5 else types[k]) for k, img in enumerate(frames)])
                     for t in range(6)])
    for a in (frames, types, costs, rows):
        a.setflags(write=False)
    return frames, types, costs, rows


def _same(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {want.size} values differ, first at (frame, row, byte) = {bad[0].tolist()} "
                             f"(frame = {FAMILIES[bad[0][0]] if want.shape[0] == len(FAMILIES) else bad[0][0]}): "
                             f"got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")


def test_the_inputs_reach_every_type_and_a_tie():
    """On the restatement alone: every one of the five types is chosen on at least 10 rows of the set, and at least one row
    has its two lowest costs equal (the lowest type number must win there)."""
    chosen, ties = np.zeros(5, dtype=np.int64), 0
    average_by_family = np.zeros(len(FAMILIES), dtype=np.int64)
    for h, w in SHAPES:
        _, types, costs, _ = _case(h, w)
        chosen += np.bincount(types.reshape(-1), minlength=5)
        two = np.sort(costs, axis=2)[:, :, :2]
        ties += int((two[:, :, 0] == two[:, :, 1]).sum())
        average_by_family += (types == 3).sum(axis=1)
    print("rows chosen per type:", chosen.tolist(), "tie rows:", ties, "average rows per family:", average_by_family.tolist())
    assert chosen.sum() == len(FAMILIES) * sum(h for h, _ in SHAPES)
    assert (chosen >= 10).all(), chosen
    assert ties >= 1
    assert average_by_family[FAMILIES.index("noise")] >= 10


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rows_and_costs_equal_the_restatement(shape):
    from refid_amd import ops
    h, w = shape
    frames, types, costs, rows = _case(h, w)
    n = len(FAMILIES)
    dev = torch.from_numpy(frames.copy()).cuda()
    got_costs = torch.full((n, h, 5), -1, dtype=torch.int32, device="cuda")
    got = ops.png_filter(dev, "adaptive", costs=got_costs)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, h, 1 + 3 * w)
    _same(got[:, :, 0], types.astype(np.uint8), "adaptive filter bytes")
    _same(got, rows[5], "adaptive rows")
    _same(got_costs, costs.astype(np.int32), "costs (adaptive)")
    assert torch.equal(ops.png_filter(dev), got)                                  # the default mode; no costs asked for
    for t in range(5):
        got_costs.fill_(-1)
        fixed = ops.png_filter(dev, t, costs=got_costs)
        _same(fixed, rows[t], f"mode {t} rows")
        _same(got_costs, costs.astype(np.int32), f"costs (mode {t})")
        assert torch.equal(ops.png_filter(dev, t), fixed)                         # without costs: pass 1 is skipped


def test_a_frame_does_not_depend_on_its_place_or_on_the_run():
    from refid_amd import ops
    frames, _, costs, rows = _case(65, 33)
    pick = [FAMILIES.index(f) for f in ("waves", "noise", "blocks")]
    dev = torch.from_numpy(frames[pick].copy()).cuda()
    c3 = torch.empty((3, 65, 5), dtype=torch.int32, device="cuda")
    three = ops.png_filter(dev, costs=c3)
    _same(three, rows[5][pick], "three frames in one call")
    for k in range(3):
        c1 = torch.empty((1, 65, 5), dtype=torch.int32, device="cuda")
        alone = ops.png_filter(dev[k:k + 1], costs=c1)
        assert torch.equal(alone[0], three[k]) and torch.equal(c1[0], c3[k]), k
    again = ops.png_filter(dev)
    assert torch.equal(again, three)


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (17, 35), (65, 33), (3, 343), (5, 1367)], ids=lambda s: "x".join(map(str, s)))
def test_nothing_is_written_outside_out_at_any_alignment(shape):
    """``out`` inside a larger buffer, 64 canary bytes on each side, starting at each of the four byte alignments."""
    from refid_amd import ops
    h, w = shape
    frames, _, _, rows = _case(h, w)
    dev = torch.from_numpy(frames.copy()).cuda()
    size = rows[5].size
    for mode, want in (("adaptive", rows[5]), (4, rows[4])):
        for shift in range(4):
            big = torch.full((256 + size + 64 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
            start = 64 + (shift - (big.data_ptr() + 64)) % 4          # (data_ptr + start) % 4 == shift, 64..67 canaries in front
            out = big[start:start + size]
            assert out.data_ptr() % 4 == shift
            got = ops.png_filter(dev, mode, out=out)
            assert got.data_ptr() == out.data_ptr()
            _same(got, want, f"{mode} rows at alignment {shift}")
            host = big.cpu().numpy()
            assert (host[:start] == 0xA5).all() and (host[start + size:] == 0xA5).all(), (mode, shift)


def test_round_trip_on_the_device():
    from refid_amd import ops
    for h, w in ((17, 35), (130, 21), (3, 343)):
        frames = torch.from_numpy(_case(h, w)[0].copy()).cuda()
        rows = ops.png_filter(frames)
        back = ops.png_unfilter(rows.view(-1), frames.shape[0], h, w, 3)
        assert torch.equal(back, frames), (h, w)


def test_rejected_arguments():
    from refid_amd import _lib, ops
    good = torch.zeros((2, 3, 4, 3), dtype=torch.uint8, device="cuda")
    for bad in (good.cpu(), good.float(), good[0], good[:, :, :, :2], good.permute(0, 2, 1, 3), good[:0], good.cpu().numpy()):
        with pytest.raises(_lib.RefidHipError, match="png_filter: a non-empty contiguous uint8 CUDA tensor"):
            ops.png_filter(bad)
    for mode in ("best", "paeth", 5, -1, 2.0, True, None):
        with pytest.raises(_lib.RefidHipError, match="png_filter: mode"):
            ops.png_filter(good, mode)
    for out in (torch.empty(2 * 3 * 13 - 1, dtype=torch.uint8, device="cuda"), torch.empty(2 * 3 * 13, dtype=torch.uint8),
                torch.empty(2 * 3 * 13, dtype=torch.int8, device="cuda"), torch.empty(2 * 2 * 3 * 13, dtype=torch.uint8, device="cuda")[::2]):
        with pytest.raises(_lib.RefidHipError, match="png_filter: out must be"):
            ops.png_filter(good, out=out)
    for costs in (torch.empty((2, 3, 4), dtype=torch.int32, device="cuda"), torch.empty((2, 3, 5), dtype=torch.int64, device="cuda"),
                  torch.empty((2, 3, 5), dtype=torch.int32)):
        with pytest.raises(_lib.RefidHipError, match="png_filter: costs must be"):
            ops.png_filter(good, costs=costs)


def _writer_frames():
    frames = _case(40, 56)[0]
    return frames, torch.from_numpy(frames.copy()).cuda()


def test_frame_writer_adaptive_files(tmp_path):
    """Two dumps through both pinned slots plus a third that reuses the first: every file decodes to its frame with read_png
    and with the GPU loader, and its filter-byte column is the restatement's adaptive choice."""
    from refid_amd import png
    from refid_amd.sequence import load_png_frames
    from refid_amd.validation import FrameWriter
    frames, dev = _writer_frames()
    types = _case(40, 56)[1]
    groups = [list(range(0, 4)), list(range(4, 7)), list(range(7, 9))]
    writer = FrameWriter(torch.device("cuda"), png_filter="adaptive")
    try:
        for g in groups[:2]:
            writer.dump([(dev[g[0]:g[-1] + 1], [str(tmp_path / "a" / f"{k:02d}.png") for k in g])])
        g = groups[2]                                         # two batches in one item, as save_gt gives
        writer.dump([(dev[g[0]:g[-1] + 1], [str(tmp_path / "a" / f"{k:02d}.png") for k in g]),
                     (dev[:2], [str(tmp_path / "a" / f"gt{k}.png") for k in range(2)])])
    finally:
        writer.close()
    files = [str(tmp_path / "a" / f"{k:02d}.png") for k in range(9)]
    for k, path in enumerate(files):
        assert np.array_equal(png.read_png(path), frames[k]), FAMILIES[k]
        w, h, ch, rows = png.read_filtered(path)
        assert (w, h, ch) == (56, 40, 3) and np.array_equal(rows[:, 0], types[k]), FAMILIES[k]
    assert np.array_equal(png.read_png(str(tmp_path / "a" / "gt1.png")), frames[1])
    assert torch.equal(load_png_frames(files), dev)
    try:
        from PIL import Image
    except ImportError:
        return
    for k, path in enumerate(files):
        with Image.open(path) as pil:
            assert np.array_equal(np.asarray(pil), frames[k]), FAMILIES[k]


def test_frame_writer_none_keeps_its_bytes(tmp_path):
    from refid_amd import png
    from refid_amd.validation import FrameWriter
    frames, dev = _writer_frames()
    for kwargs in ({}, {"png_filter": "none"}):
        writer = FrameWriter(torch.device("cuda"), **kwargs)
        try:
            writer.dump([(dev[:3], [str(tmp_path / f"{k}.png") for k in range(3)])])
        finally:
            writer.close()
        for k in range(3):
            assert (tmp_path / f"{k}.png").read_bytes() == png.encode_png(frames[k], 1)
    with pytest.raises(Exception, match="png_filter"):
        FrameWriter(torch.device("cuda"), png_filter="paeth")


def test_a_worker_failure_still_surfaces_from_close(tmp_path):
    from refid_amd.validation import FrameWriter
    _, dev = _writer_frames()
    blocker = tmp_path / "file"
    blocker.write_text("x")                                   # a path under a regular file: makedirs fails in the workers
    writer = FrameWriter(torch.device("cuda"), png_filter="adaptive")
    writer.dump([(dev[:2], [str(blocker / "vis" / f"{k}.png") for k in range(2)])])
    with pytest.raises(OSError):
        writer.close()


def test_the_command_line_writes_the_same_pixels(tmp_path):
    """python -m refid_amd.interpolate's argument parser and main, on the tiny fixture of the command-line test of
    test_hip_png_unfilter.py: --png-filter adaptive writes files with the pixels of the default run, which are still the
    bytes encode_png gives; val.png_filter of --opt is the default of the flag."""
    from oracle import refid_oracle as O
    from refid_amd import interpolate, png
    from test_sequence_host import TEST_YAML
    rng = np.random.Generator(np.random.PCG64(5))
    yy, xx = np.mgrid[0:37, 0:50]
    frames = np.stack([np.clip((110 + 70 * np.sin((xx + 9 * k) / 11.0) + 50 * np.cos((yy - 4 * k) / 7.0))[:, :, None] +
                               np.array([0.0, 18.0, -25.0]) + rng.normal(0, 2.5, (37, 50, 3)), 0, 255).astype(np.uint8) for k in range(3)])
    np.save(tmp_path / "frames.npy", frames)
    n = 2000
    t = np.sort(rng.uniform(10.0, 30.0, n))
    np.savez(tmp_path / "e.npz", x=rng.integers(0, 50, n), y=rng.integers(0, 37, n), timestamp=t, polarity=rng.integers(0, 2, n) * 2 - 1)
    (tmp_path / "stamps.txt").write_text("10.0\n20.0\n30.0\n")
    yml = TEST_YAML.replace("num_inter_interpolation: 7", "num_inter_interpolation: 3")
    (tmp_path / "t.yml").write_text(yml)
    torch.save({"params": O.make_params(6, base_num_channels=8, mode="hash", seed=3)}, tmp_path / "w.pth")
    common = ["--checkpoint", str(tmp_path / "w.pth"), "--events", str(tmp_path / "e.npz"), "--stamps", str(tmp_path / "stamps.txt"),
              "--frames", str(tmp_path / "frames.npy")]
    opt = ["--opt", str(tmp_path / "t.yml")]
    assert interpolate.main([*opt, *common, "--out", str(tmp_path / "none")]) == 0
    assert interpolate.main([*opt, *common, "--png-filter", "adaptive", "--out", str(tmp_path / "adaptive")]) == 0
    names = sorted(os.listdir(tmp_path / "none"))
    assert names == [f"{k:06d}_{f:02d}.png" for k in range(2) for f in range(3)] and sorted(os.listdir(tmp_path / "adaptive")) == names
    filtered = 0
    for name in names:
        a, b = png.read_png(str(tmp_path / "none" / name)), png.read_png(str(tmp_path / "adaptive" / name))
        assert a.shape == (37, 50, 3) and np.array_equal(a, b), name
        assert (tmp_path / "none" / name).read_bytes() == png.encode_png(a, 1), name
        rows = png.read_filtered(str(tmp_path / "adaptive" / name))[3]
        assert np.array_equal(rows[:, 0], R.adaptive_types(a)), name
        filtered += int((rows[:, 0] != 0).sum())
    assert filtered > 0
    if "\nval:" in yml:
        keyed = yml.replace("\nval:", "\nval:\n  png_filter: adaptive", 1)
    else:
        keyed = yml + "\nval:\n  png_filter: adaptive\n"
    (tmp_path / "k.yml").write_text(keyed)
    assert interpolate.main(["--opt", str(tmp_path / "k.yml"), *common, "--out", str(tmp_path / "keyed")]) == 0
    for name in names:
        assert (tmp_path / "keyed" / name).read_bytes() == (tmp_path / "adaptive" / name).read_bytes(), name


def test_the_validation_loop_reads_val_png_filter(tmp_path):
    """nondist_validation with val.png_filter: adaptive writes the files of the default run with the same pixels and the
    restatement's filter types; the default run's bytes are still encode_png's; another value is rejected by name."""
    from refid_amd import _lib, png
    from test_hip_validation_loop import _files, _loader, _model
    for sub, val in (("none", {}), ("adaptive", {"png_filter": "adaptive"})):
        model = _model(tmp_path / sub, **val)
        model.validation(_loader(), 7, None, save_img=True)
    files = _files(tmp_path / "none")
    assert len(files) == 40 and _files(tmp_path / "adaptive") == files
    for rel in files:
        a = png.read_png(str(tmp_path / "none" / rel))
        assert np.array_equal(png.read_png(str(tmp_path / "adaptive" / rel)), a), rel
        assert (tmp_path / "none" / rel).read_bytes() == png.encode_png(a, 1), rel
        assert np.array_equal(png.read_filtered(str(tmp_path / "adaptive" / rel))[3][:, 0], R.adaptive_types(a)), rel
    with pytest.raises(_lib.RefidHipError, match="val.png_filter: 'sub'"):
        _model(tmp_path / "bad", png_filter="sub").validation(_loader(), 7, None, save_img=True)
