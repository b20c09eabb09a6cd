"""MI355X: refid_jpeg_decode (csrc/jpeg_decode.hip) through ops.jpeg_decode, sequence.load_jpeg_frames / load_key_frames and
the command lines.

Every comparison is exact equality of uint8 arrays: the decoder is integer arithmetic (libjpeg's islow IDCT, fancy
upsampling, table-based colour conversion), restated in tests/jpeg_decode_ref.py, which tests/test_jpeg_decode_ref_host.py
pins to PIL byte for byte; the golden cases carry PIL's own pixels.  Shapes are the smallest at which the kernels can go
wrong: a single pixel, exact blocks, sizes that are no multiple of the MCU, chroma planes of 1 and 2 columns (replicated
instead of interpolated), a single chroma row, and per sampling one MCU row and one MCU column past what a workgroup
covers: the colour kernel's workgroup takes 256 lanes x 4 pixels = 1024 pixels of ONE row, so widths of 1033 (8-pixel MCUs)
and 1041 (16-pixel MCUs) add a second strip that holds one MCU column and a ragged last group, and heights of 17 / 33 add
an MCU row; the IDCT kernel's workgroup takes 256 consecutive blocks, which these shapes pass within a plane, across the
component planes and across frames.  For one shape and sampling all data families go through ONE launch as a batch."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpeg_decode_cases as K
import jpeg_decode_ref as R
import jpeg_ref as J

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (8, 8), (16, 16), (17, 35), (33, 65), (9, 4), (5, 3), (2, 17)]
PAST_A_WORKGROUP = {"grey": (17, 1033), "444": (17, 1033), "422": (17, 1041), "420": (33, 1041)}


@functools.lru_cache(maxsize=None)
def _case(h, w, sampling):
    """Every family of one shape and sampling: (coefs (F, B, 64), quant (F, C, 64), pixels (F, H, W, 3)).  Built once."""
    coefs, quant = zip(*(K.coefficients(h, w, sampling, family, seed=h * 1000 + w) for family in K.FAMILIES))
    want = np.stack([R.pixels(c, q, h, w, K.CODES[sampling]) for c, q in zip(coefs, quant)])
    out = np.stack(coefs), np.stack(quant), want
    for a in out:
        a.setflags(write=False)
    return out


def _dev(a):
    a = np.array(a)                                                              # (a writable, contiguous copy)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _same(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    for k in range(len(want)):
        if not np.array_equal(got[k], want[k]):
            bad = np.argwhere(got[k] != want[k])
            raise AssertionError(f"{what}: frame {k}: {len(bad)} bytes differ, first at (y, x, c) = {bad[0].tolist()}: "
                                 f"got {got[k][tuple(bad[0])]}, want {want[k][tuple(bad[0])]}")


@pytest.mark.parametrize("sampling", K.SAMPLINGS)
@pytest.mark.parametrize("shape", SHAPES + ["past"], ids=lambda s: s if isinstance(s, str) else f"{s[0]}x{s[1]}")
def test_every_family_decodes_to_the_restatements_pixels(shape, sampling):
    from refid_amd import ops
    h, w = PAST_A_WORKGROUP[sampling] if shape == "past" else shape
    coefs, quant, want = _case(h, w, sampling)
    assert want[K.FAMILIES.index("zeros")].max() <= 2 and want[K.FAMILIES.index("white")].min() >= 253
    extreme = want[K.FAMILIES.index("extreme")]
    assert h * w < 64 or (extreme.min() == 0 and extreme.max() == 255)             # the clamp is reached on both sides
    got = ops.jpeg_decode(_dev(coefs), _dev(quant), len(K.FAMILIES), h, w, sampling)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (len(K.FAMILIES), h, w, 3)
    _same(got, want, f"{h}x{w} {sampling} ({', '.join(K.FAMILIES)})")


@functools.lru_cache(maxsize=None)
def _nine(sampling):
    """Nine different frames of 17x35 whose tables differ from frame to frame."""
    h, w = 17, 35
    coefs, quant = [], []
    for f in range(9):
        c, q = K.coefficients(h, w, sampling, ("noise", "smooth", "extreme")[f % 3], seed=50 + f)
        coefs.append(c)
        quant.append((q - f if f % 3 == 2 else np.clip(q.astype(np.int64) * (1 + f % 4) + f, 1, 255)).astype(np.uint16))     # (extreme: 255 - f)
    want = np.stack([R.pixels(c, q, h, w, K.CODES[sampling]) for c, q in zip(coefs, quant)])
    return np.stack(coefs), np.stack(quant), want


@pytest.mark.parametrize("sampling", K.SAMPLINGS)
def test_batches_of_1_3_and_9_and_tables_that_differ_per_frame(sampling):
    from refid_amd import ops
    h, w = 17, 35
    coefs, quant, want = _nine(sampling)
    assert len({q.tobytes() for q in quant}) == 9 and len({p.tobytes() for p in want}) == 9
    nine = ops.jpeg_decode(_dev(coefs), _dev(quant), 9, h, w, sampling)
    _same(nine, want, "a batch of 9")
    three = ops.jpeg_decode(_dev(coefs[[7, 2, 5]]), _dev(quant[[7, 2, 5]]), 3, h, w, sampling)       # other positions
    _same(three, want[[7, 2, 5]], "a batch of 3")
    for f in (0, 5, 8):
        alone = ops.jpeg_decode(_dev(coefs[f:f + 1]), _dev(quant[f:f + 1]), 1, h, w, sampling)
        assert torch.equal(alone[0], nine[f]), f                                 # the same bytes alone as in the batch
    # frame 5's coefficients under frame 6's tables are another picture: the tables are taken per frame
    mixed = ops.jpeg_decode(_dev(coefs[[5, 5]]), _dev(quant[[5, 6]]), 2, h, w, sampling)
    assert torch.equal(mixed[0], nine[5]) and not torch.equal(mixed[1], nine[5])
    _same(mixed[1:], R.pixels(coefs[5], quant[6], h, w, K.CODES[sampling])[None], "frame 5 under the tables of frame 6")


@pytest.mark.parametrize("sampling", ["420", "grey"])
@pytest.mark.parametrize("shape,offset", [((17, 35), 13), ((17, 36), 13), ((17, 36), 16), ((5, 3), 7)], ids=str)
def test_guard_bytes_around_out_stay_untouched(shape, offset, sampling):
    """``out`` as a slice of a larger byte tensor at an odd (13, 7) and an aligned (16) byte offset.  A row of 35 pixels is
    105 bytes, so the rows of one frame start at every alignment and take both store paths; rows of 36 pixels at offset 13
    are all unaligned, at offset 16 all aligned."""
    from refid_amd import ops
    h, w = shape
    coefs, quant, want = _case(h, w, sampling)
    n, size = len(want), want.size
    flat = torch.full((offset + size + 29,), 0x5A, dtype=torch.uint8, device="cuda")
    view = flat[offset:offset + size].view(n, h, w, 3)
    assert view.data_ptr() % 4 == offset % 4 and view.is_contiguous()
    got = ops.jpeg_decode(_dev(coefs), _dev(quant), n, h, w, sampling, out=view)
    assert got.data_ptr() == view.data_ptr()
    _same(view, want, f"out at byte offset {offset}")
    assert bool((flat[:offset] == 0x5A).all()) and bool((flat[offset + size:] == 0x5A).all())
    # a view of the frames inside a tensor of two more: the frames before and after stay as they were
    big = torch.full((n + 2, h, w, 3), 0xA5, dtype=torch.uint8, device="cuda")
    ops.jpeg_decode(_dev(coefs), _dev(quant), n, h, w, sampling, out=big[1:n + 1])
    _same(big[1:n + 1], want, "out view")
    assert bool((big[0] == 0xA5).all()) and bool((big[n + 1] == 0xA5).all())


def test_byte_offsets_past_2_to_the_31_in_coefs_and_frames():
    """One 27000x27000 4:2:0 frame: 2.19e9 bytes of coefficients and of pixels, so the offsets into both pass 2^31 (the
    component planes in the scratch stay below it).  All coefficients are zero -- every pixel 128 -- but for the DC of three
    luma blocks (the first, one whose pixels lie past byte 2^31 of the frame, the last visible one): DC 80 under a quantiser
    of 1 is exactly 10 levels, (80 * 4 * 8192 + 2^17) >> 18.  Everything is made and checked on the device."""
    from refid_amd import ops
    h = w = 27000
    blocks, total = ops.jpeg_decode_blocks(h, w, "420")
    wide = blocks[0] // ((h + 15) // 16 * 2)                                      # luma blocks per row of the padded plane
    assert total * 128 > 2 ** 31 and 3 * h * w > 2 ** 31 and wide == 3376
    coefs = torch.zeros((1, total, 64), dtype=torch.int16, device="cuda")
    quant = torch.ones((1, 3, 64), dtype=torch.int16, device="cuda")
    marks = [(0, 0), (3370, 11), (3374, 3374)]
    assert (3370 * 8 * w + 11 * 8) * 3 > 2 ** 31
    for by, bx in marks:
        coefs[0, by * wide + bx, 0] = 80
    out = ops.jpeg_decode(coefs, quant, 1, h, w, "420")
    for by, bx in marks:
        assert bool((out[0, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8] == 138).all()), (by, bx)
    assert int((out != 128).sum()) == 3 * 64 * len(marks)
    del out, coefs


def test_load_jpeg_frames_equals_pils_pixels_on_the_golden_cases():
    from refid_amd.sequence import load_jpeg_frames
    for name, (data, rgb) in K.golden().items():
        got = load_jpeg_frames([data, data], frames_per_launch=1, workers=1)      # two chunks: both staging buffers
        assert got.is_cuda and tuple(got.shape) == (2,) + rgb.shape
        _same(got, np.stack([rgb, rgb]), name)


def _nine_files():
    frames = [np.roll(K.image(17, 35, ("noise", "smooth")[k % 2], seed=30 + k), k, axis=1) for k in range(9)]
    return [J.encode(f, (90, 50, 75)[k % 3], J.J420, (None, 1, 3)[k % 3]) for k, f in enumerate(frames)]


def test_load_jpeg_frames_keeps_the_order_and_names_the_file_that_is_wrong(tmp_path):
    """9 files, frames_per_launch=4, workers=2: a short last chunk, and both staging buffers are written twice."""
    from refid_amd._lib import RefidHipError
    from refid_amd.sequence import load_jpeg_frames, load_key_frames
    files = _nine_files()
    want = np.stack([R.decode(d) for d in files])
    assert len({w.tobytes() for w in want}) == 9
    os.makedirs(tmp_path / "seq")
    for k, data in enumerate(files):
        (tmp_path / "seq" / f"{k:03d}.{'jpeg' if k % 2 else 'jpg'}").write_bytes(data)
    _same(load_jpeg_frames(str(tmp_path / "seq"), frames_per_launch=4, workers=2), want, "a directory, 4 per launch")
    _same(load_jpeg_frames(files, frames_per_launch=4, workers=2), want, "byte strings, 4 per launch")
    _same(load_key_frames(str(tmp_path / "seq")), want, "load_key_frames, one launch")
    paths = sorted(str(p) for p in (tmp_path / "seq").iterdir())
    _same(load_jpeg_frames(paths[::-1], frames_per_launch=2), want[::-1], "paths in reverse")
    (tmp_path / "seq" / "006.jpg").write_bytes(J.encode(K.image(17, 36, "noise", 1), 90, J.J420))
    with pytest.raises(RefidHipError, match="006.jpg is 17x36, 3 components, sampling 420; .*000.jpg is 17x35"):
        load_jpeg_frames(str(tmp_path / "seq"), frames_per_launch=4, workers=2)
    (tmp_path / "seq" / "006.jpg").write_bytes(J.encode(K.image(17, 35, "noise", 1), 90, J.J444))
    with pytest.raises(RefidHipError, match="006.jpg is 17x35, 3 components, sampling 444"):
        load_jpeg_frames(str(tmp_path / "seq"), frames_per_launch=4)
    progressive = K.edit(files[6], 0xc0, lambda p: p, 0xc2)
    (tmp_path / "seq" / "006.jpg").write_bytes(progressive)
    with pytest.raises(RefidHipError, match="006.jpg: .*jpeg_decode: a progressive \\(SOF2\\) frame"):
        load_jpeg_frames(str(tmp_path / "seq"), frames_per_launch=4, workers=2)
    (tmp_path / "seq" / "006.jpg").write_bytes(files[6][:-20])
    with pytest.raises(RefidHipError, match="006.jpg: .*ends before the last MCU"):
        load_jpeg_frames(str(tmp_path / "seq"), frames_per_launch=4, workers=2)
    with pytest.raises(RefidHipError, match="frame 1 \\(.* bytes\\): .*progressive"):
        load_jpeg_frames([files[0], progressive])


@pytest.mark.parametrize("subsampling", ["420", "444"])
def test_encode_to_avi_and_back_equals_the_restatements_decode(tmp_path, subsampling):
    """ops.jpeg_encode -> MjpegAviWriter -> load_key_frames: the pixels are the restatement's decode of the very bytes the
    encoder wrote (the project's --video output read back in)."""
    from refid_amd import ops
    from refid_amd.sequence import load_key_frames
    from refid_amd.video import MjpegAviWriter
    frames = np.stack([np.roll(K.image(37, 50, "smooth"), 3 * k, axis=1) for k in range(5)])
    out, lens = ops.jpeg_encode(torch.from_numpy(frames).cuda(), quality=85, subsampling=subsampling, restart_mcus=3)
    out, lens = out.cpu().numpy(), lens.cpu().numpy()
    assert (lens > 0).all()
    files = [out[k, :lens[k]].tobytes() for k in range(5)]
    with MjpegAviWriter(str(tmp_path / "clip.avi"), 50, 37, 30) as wr:
        for data in files:
            wr.add(data)
    want = np.stack([R.decode(d) for d in files])
    assert R.probe(files[0]).sampling == subsampling and R.probe(files[0]).restart_interval == 3
    _same(load_key_frames(str(tmp_path / "clip.avi"), frames_per_launch=2), want, "AVI round trip")
    assert np.abs(want.astype(np.int64) - frames).mean() < 10                      # and they are the frames that went in, lossily


def test_the_command_lines_take_a_jpeg_directory_and_an_avi(tmp_path):
    """python -m refid_amd.interpolate, in fresh child processes, on --frames DIR_OF_JPEGS and on --frames clip.avi writes the
    PNG bytes the same command gives, in process, on the .npy stack of the expected decoded frames (the tiny network of
    tests/test_hip_png_unfilter.py's command-line test)."""
    from oracle import refid_oracle as O
    from refid_amd import interpolate
    from refid_amd.video import MjpegAviWriter
    from test_sequence_host import TEST_YAML
    files = [J.encode(K.image(37, 50, "smooth", seed=k) // 2 + K.image(37, 50, "noise", seed=k) // 8, 90, J.J420) for k in range(3)]
    os.makedirs(tmp_path / "frames")
    for k, data in enumerate(files):
        (tmp_path / "frames" / f"{k:03d}.jpg").write_bytes(data)
    with MjpegAviWriter(str(tmp_path / "clip.avi"), 50, 37, 30) as wr:
        for data in files:
            wr.add(data)
    np.save(tmp_path / "frames.npy", np.stack([R.decode(d) for d in files]))
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
    children = [subprocess.Popen([sys.executable, "-m", "refid_amd.interpolate", *common, "--frames", str(tmp_path / source), "--out",
                                  str(tmp_path / out)], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                for source, out in (("frames", "out_jpg"), ("clip.avi", "out_avi"))]
    assert interpolate.main([*common, "--frames", str(tmp_path / "frames.npy"), "--out", str(tmp_path / "out_npy")]) == 0
    for child in children:
        text, _ = child.communicate(timeout=300)
        assert child.returncode == 0, text
    names = sorted(os.listdir(tmp_path / "out_npy"))
    assert names == [f"{k:06d}_{f:02d}.png" for k in range(2) for f in range(3)]
    for out in ("out_jpg", "out_avi"):
        assert sorted(os.listdir(tmp_path / out)) == names
        for name in names:
            assert (tmp_path / out / name).read_bytes() == (tmp_path / "out_npy" / name).read_bytes(), (out, name)
    assert len({(tmp_path / "out_npy" / name).read_bytes() for name in names}) == len(names)      # six different frames
