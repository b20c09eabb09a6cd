"""MI355X: refid_png_deflate (csrc/png_deflate.hip) through ops.png_deflate, validation.FrameWriter, the validation loop and
both command lines.

Every comparison is exact equality of bytes: the kernels are integer arithmetic, so there is no tolerance anywhere.  The
expected streams are tests/deflate_ref.py's (pinned to zlib's inflate, png.read_png and PIL by test_deflate_ref_host.py),
over the streams of tests/deflate_cases.py: the adaptive rows of six frame shapes x nine data families (the nine streams
of a shape go through one launch as a batch), a Fibonacci-frequency stream that reaches the length repair, and one that
holds all 256 byte values -- each at block sizes 1, 64, 257, 4096, 65535 and the default.  Small blocks make a small frame
span many workgroups, and the segments then start at every byte alignment."""
import ctypes
import os

import numpy as np
import pytest
import torch

import deflate_cases as K
import deflate_ref as D

pytestmark = pytest.mark.gpu


def _run(data, block_bytes, **kw):
    from refid_amd import ops
    out, lens = ops.png_deflate(torch.from_numpy(np.array(data)).cuda(), block_bytes, **kw)
    assert out.dtype == torch.uint8 and lens.dtype == torch.int32 and tuple(lens.shape) == (data.shape[0],)
    return out.cpu().numpy(), lens.cpu().numpy()


def _same(out, lens, want, what):
    for k, stream in enumerate(want):
        assert int(lens[k]) == len(stream), (what, k, int(lens[k]), len(stream))
        got = out[k, :len(stream)].tobytes()
        if got != stream:
            bad = [i for i in range(len(stream)) if got[i] != stream[i]]
            raise AssertionError(f"{what}, stream {k}: {len(bad)} of {len(stream)} bytes differ, first at {bad[0]}: "
                                 f"got {got[bad[0]]:#04x}, want {stream[bad[0]]:#04x}")


@pytest.mark.parametrize("block_bytes", K.BLOCKS)
@pytest.mark.parametrize("case", K.CASES)
def test_streams_and_lengths_equal_the_restatement(case, block_bytes):
    data = K.streams(case)
    want = K.expected(case, block_bytes)[0]
    out, lens = _run(data, block_bytes)
    assert out.shape == (data.shape[0], D.bound(data.shape[1], block_bytes))
    _same(out, lens, want, f"{case} in blocks of {block_bytes}")
    if block_bytes == D.DEFAULT_BLOCK_BYTES:
        out, lens = _run(data, None)
        _same(out, lens, want, f"{case} at the default block size")
        if "x" in case:                                        # (N, H, 1 + 3W), as png_filter returns it
            h = int(case.split("x")[0])
            out, lens = _run(data.reshape(data.shape[0], h, -1), None)
            _same(out, lens, want, f"{case} as rows")


def test_a_stream_does_not_depend_on_its_place_or_on_the_run():
    from refid_amd import ops
    data = K.streams("65x33")
    pick = [K.FAMILIES.index(f) for f in ("waves", "noise", "blocks")]
    for block_bytes in (257, 4096):
        want = K.expected("65x33", block_bytes)[0]
        dev = torch.from_numpy(data[pick].copy()).cuda()
        three, lens3 = ops.png_deflate(dev, block_bytes)
        _same(three.cpu().numpy(), lens3.cpu().numpy(), [want[k] for k in pick], "three streams in one call")
        for k in range(3):
            alone, lens1 = ops.png_deflate(dev[k:k + 1], block_bytes)
            n = int(lens1[0])
            assert n == int(lens3[k]) and torch.equal(alone[0, :n], three[k, :n]), k
        again, lens_again = ops.png_deflate(dev, block_bytes)
        assert torch.equal(lens_again, lens3)
        for k in range(3):
            assert torch.equal(again[k, :int(lens3[k])], three[k, :int(lens3[k])]), k


@pytest.mark.parametrize("case,block_bytes", [("1x1", 1), ("2x3", 64), ("17x35", 257), ("65x33", 4096), ("5x1367", 257),
                                              ("all256", 65535)])
def test_nothing_is_written_outside_out_lens_and_work_at_any_alignment(case, block_bytes):
    """``src`` and ``out`` inside larger buffers at each of the four byte alignments, ``lens`` and ``work`` inside larger
    buffers too, canaries all round; the pitch is a little more than the bound, and the bytes behind a stream stay."""
    from refid_amd import _lib, ops
    data = K.streams(case)
    want = K.expected(case, block_bytes)[0]
    n, size = data.shape
    L = _lib.lib()
    pitch = D.bound(size, block_bytes) + 3
    work_words = D.work_bytes(n, size, block_bytes) // 4
    assert L.refid_png_deflate_work_bytes(n, size, block_bytes) == 4 * work_words
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for shift in range(4):
        big = torch.full((64 + n * pitch + 64 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        start = 64 + (shift - (big.data_ptr() + 64)) % 4
        out = big[start:start + n * pitch]
        src_big = torch.zeros((n * size + 8,), dtype=torch.uint8, device="cuda")
        src_start = (3 - shift - src_big.data_ptr()) % 4       # the input at another alignment than the output
        src = src_big[src_start:src_start + n * size]
        src.copy_(torch.from_numpy(data.reshape(-1).copy()))
        assert out.data_ptr() % 4 == shift and src.data_ptr() % 4 == 3 - shift
        lens_big = torch.full((n + 32,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        work_big = torch.full((work_words + 32,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        desc = _lib.PngDeflateDesc(src=src.data_ptr(), out=out.data_ptr(), lens=lens_big[16:].data_ptr(), work=work_big[16:].data_ptr(),
                                   n_streams=n, stream_bytes=size, block_bytes=block_bytes, out_pitch=pitch)
        ops.check(L.refid_png_deflate(ctypes.byref(desc), stream), "refid_png_deflate")
        host = big.cpu().numpy()
        lens = lens_big.cpu().numpy()
        _same(host[start:start + n * pitch].reshape(n, pitch), lens[16:16 + n], want, f"{case} at alignment {shift}")
        assert (host[:start] == 0xA5).all() and (host[start + n * pitch:] == 0xA5).all(), shift
        for k in range(n):
            assert (host[start + k * pitch + len(want[k]):start + (k + 1) * pitch] == 0xA5).all(), (shift, k)
        assert (lens[:16] == 0x5A5A5A5A).all() and (lens[16 + n:] == 0x5A5A5A5A).all(), shift
        work = work_big.cpu().numpy()
        assert (work[:16] == 0x5A5A5A5A).all() and (work[16 + work_words:] == 0x5A5A5A5A).all(), shift


def test_rejected_arguments():
    from refid_amd import _lib, ops
    good = torch.zeros((2, 3, 13), dtype=torch.uint8, device="cuda")
    for bad in (good.cpu(), good.float(), good[0, 0], good[:, :, :5], good[:0], good.cpu().numpy(), good[None]):
        with pytest.raises(_lib.RefidHipError, match="png_deflate: a non-empty contiguous uint8 CUDA tensor"):
            ops.png_deflate(bad)
    for block in (0, -1, 65536, 2.0, True, "big"):
        with pytest.raises(_lib.RefidHipError, match="png_deflate: block_bytes"):
            ops.png_deflate(good, block)
    bound = D.bound(39, 64)
    for out in (torch.empty((2, bound - 1), dtype=torch.uint8, device="cuda"), torch.empty((2, bound), dtype=torch.uint8),
                torch.empty((2, bound), dtype=torch.int8, device="cuda"), torch.empty((3, bound), dtype=torch.uint8, device="cuda"),
                torch.empty((2, 2 * bound), dtype=torch.uint8, device="cuda")[:, ::2], torch.empty(2 * bound, dtype=torch.uint8, device="cuda")):
        with pytest.raises(_lib.RefidHipError, match="png_deflate: out must be"):
            ops.png_deflate(good, 64, out=out)
    out = torch.empty((2, bound + 5), dtype=torch.uint8, device="cuda")
    got, lens = ops.png_deflate(good, 64, out=out)
    assert got.data_ptr() == out.data_ptr() and lens.tolist() == [len(D.deflate(np.zeros(39, dtype=np.uint8), 64))] * 2


def _writer_frames():
    frames = K.frames_of(65, 33)
    return frames, torch.from_numpy(frames.copy()).cuda()


@pytest.mark.parametrize("png_filter", ["none", "adaptive"])
def test_frame_writer_device_files(tmp_path, png_filter):
    """Two dumps through both pinned slots plus a third that reuses the first and holds two batches: every file is the
    restatement's stream of the frame's rows in PNG framing, and decodes to its frame with read_png, the GPU loader and PIL."""
    import png_filter_ref as R
    from refid_amd import png
    from refid_amd.sequence import load_png_frames
    from refid_amd.validation import FrameWriter
    frames, dev = _writer_frames()
    groups = [list(range(0, 4)), list(range(4, 7)), list(range(7, 9))]
    writer = FrameWriter(torch.device("cuda"), png_filter=png_filter, png_deflate="device")
    try:
        for g in groups[:2]:
            writer.dump([(dev[g[0]:g[-1] + 1], [str(tmp_path / "a" / f"{k:02d}.png") for k in g])])
        g = groups[2]
        writer.dump([(dev[g[0]:g[-1] + 1], [str(tmp_path / "a" / f"{k:02d}.png") for k in g]),
                     (dev[:2], [str(tmp_path / "a" / f"gt{k}.png") for k in range(2)])])
    finally:
        writer.close()
    files = [str(tmp_path / "a" / f"{k:02d}.png") for k in range(9)]
    for k, path in enumerate(files):
        types = R.adaptive_types(frames[k]) if png_filter == "adaptive" else np.zeros(65, dtype=np.int64)
        rows = R.apply_filters(frames[k], types)
        assert open(path, "rb").read() == png.wrap_zlib_stream(D.deflate(rows), 33, 65), K.FAMILIES[k]
        assert np.array_equal(png.read_png(path), frames[k]), K.FAMILIES[k]
        assert np.array_equal(png.read_filtered(path)[3], rows), K.FAMILIES[k]
    assert np.array_equal(png.read_png(str(tmp_path / "a" / "gt1.png")), frames[1])
    assert torch.equal(load_png_frames(files), dev)
    try:
        from PIL import Image
    except ImportError:
        return
    for k, path in enumerate(files):
        with Image.open(path) as pil:
            assert np.array_equal(np.asarray(pil), frames[k]), K.FAMILIES[k]


def test_frame_writer_host_keeps_its_bytes(tmp_path):
    from refid_amd import png
    from refid_amd.validation import FrameWriter
    frames, dev = _writer_frames()
    for kwargs in ({}, {"png_deflate": "host"}, {"png_filter": "adaptive"}, {"png_filter": "adaptive", "png_deflate": "host"}):
        writer = FrameWriter(torch.device("cuda"), **kwargs)
        try:
            writer.dump([(dev[:3], [str(tmp_path / f"{k}.png") for k in range(3)])])
        finally:
            writer.close()
        for k in range(3):
            if kwargs.get("png_filter") == "adaptive":
                want = png.encode_png_rows(K.adaptive_rows(frames[k]), 33, 65, 1)
            else:
                want = png.encode_png(frames[k], 1)
            assert (tmp_path / f"{k}.png").read_bytes() == want, (kwargs, k)
    with pytest.raises(Exception, match="png_deflate"):
        FrameWriter(torch.device("cuda"), png_deflate="gpu")


def test_a_worker_failure_still_surfaces_from_close(tmp_path):
    from refid_amd.validation import FrameWriter
    _, dev = _writer_frames()
    blocker = tmp_path / "file"
    blocker.write_text("x")                                   # a path under a regular file: makedirs fails in the workers
    writer = FrameWriter(torch.device("cuda"), png_filter="adaptive", png_deflate="device")
    writer.dump([(dev[:2], [str(blocker / "vis" / f"{k}.png") for k in range(2)])])
    with pytest.raises(OSError):
        writer.close()


def test_the_validation_loop_reads_val_png_deflate(tmp_path):
    """nondist_validation with val.png_deflate: device writes the files of the default run with the same pixels, as the
    restatement's streams; the default run's bytes are still encode_png's; another value is rejected by name."""
    from refid_amd import _lib, png
    from test_hip_validation_loop import _files, _loader, _model
    for sub, val in (("host", {}), ("device", {"png_deflate": "device", "png_filter": "adaptive"})):
        model = _model(tmp_path / sub, **val)
        model.validation(_loader(), 7, None, save_img=True)
    files = _files(tmp_path / "host")
    assert len(files) == 40 and _files(tmp_path / "device") == files
    for rel in files:
        a = png.read_png(str(tmp_path / "host" / rel))
        assert np.array_equal(png.read_png(str(tmp_path / "device" / rel)), a), rel
        assert (tmp_path / "host" / rel).read_bytes() == png.encode_png(a, 1), rel
        want = png.wrap_zlib_stream(D.deflate(K.adaptive_rows(a)), a.shape[1], a.shape[0])
        assert (tmp_path / "device" / rel).read_bytes() == want, rel
    with pytest.raises(_lib.RefidHipError, match="val.png_deflate: 'gpu'"):
        _model(tmp_path / "bad", png_deflate="gpu").validation(_loader(), 7, None, save_img=True)


def test_the_interpolation_command_line_writes_the_same_pixels(tmp_path):
    """python -m refid_amd.interpolate on the tiny fixture of test_hip_png_filter.py's command-line test: --png-deflate device
    writes files with the pixels of the default run, which are still the bytes encode_png gives; val.png_deflate of --opt is
    the default of the flag."""
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
    assert interpolate.main([*opt, *common, "--out", str(tmp_path / "host")]) == 0
    assert interpolate.main([*opt, *common, "--png-deflate", "device", "--out", str(tmp_path / "device")]) == 0
    assert interpolate.main([*opt, *common, "--png-deflate", "device", "--png-filter", "adaptive", "--out", str(tmp_path / "both")]) == 0
    names = sorted(os.listdir(tmp_path / "host"))
    assert names == [f"{k:06d}_{f:02d}.png" for k in range(2) for f in range(3)]
    assert sorted(os.listdir(tmp_path / "device")) == names and sorted(os.listdir(tmp_path / "both")) == names
    for name in names:
        a = png.read_png(str(tmp_path / "host" / name))
        assert a.shape == (37, 50, 3) and (tmp_path / "host" / name).read_bytes() == png.encode_png(a, 1), name
        assert np.array_equal(png.read_png(str(tmp_path / "device" / name)), a), name
        assert np.array_equal(png.read_png(str(tmp_path / "both" / name)), a), name
        rows0 = np.zeros((37, 151), dtype=np.uint8)
        rows0[:, 1:] = a.reshape(37, -1)
        assert (tmp_path / "device" / name).read_bytes() == png.wrap_zlib_stream(D.deflate(rows0), 50, 37), name
        assert (tmp_path / "both" / name).read_bytes() == png.wrap_zlib_stream(D.deflate(K.adaptive_rows(a)), 50, 37), name
    if "\nval:" in yml:
        keyed = yml.replace("\nval:", "\nval:\n  png_deflate: device", 1)
    else:
        keyed = yml + "\nval:\n  png_deflate: device\n"
    (tmp_path / "k.yml").write_text(keyed)
    assert interpolate.main(["--opt", str(tmp_path / "k.yml"), *common, "--out", str(tmp_path / "keyed")]) == 0
    for name in names:
        assert (tmp_path / "keyed" / name).read_bytes() == (tmp_path / "device" / name).read_bytes(), name


def test_the_deblurring_command_line_writes_the_same_pixels(tmp_path):
    """python -m refid_amd.deblur on the fixture of test_hip_sequence_single.py's command-line test, with and without the flag."""
    from refid_amd import deblur, png
    from test_hip_sequence_single import TEST_YAML, _net, _sequence
    frames, ev, windows = _sequence()
    for k in range(3):
        png.write_png(str(tmp_path / "frames" / f"{k:03d}.png"), frames[k])
    np.savez(tmp_path / "e.npz", x=ev[:, 1], y=ev[:, 2], timestamp=ev[:, 0], polarity=ev[:, 3])
    (tmp_path / "stamps.txt").write_text("".join(f"{a!r} {b!r}\n" for a, b in windows.tolist()))
    (tmp_path / "t.yml").write_text(TEST_YAML)
    torch.save({"params": {k: v.cpu() for k, v in _net().state_dict().items()}}, tmp_path / "w.pth")
    common = ["--opt", str(tmp_path / "t.yml"), "--checkpoint", str(tmp_path / "w.pth"), "--frames", str(tmp_path / "frames"),
              "--events", str(tmp_path / "e.npz"), "--stamps", str(tmp_path / "stamps.txt")]
    assert deblur.main([*common, "--out", str(tmp_path / "host")]) == 0
    assert deblur.main([*common, "--png-deflate", "device", "--png-filter", "adaptive", "--out", str(tmp_path / "device")]) == 0
    names = sorted(os.listdir(tmp_path / "host"))
    assert names == [f"{k:06d}.png" for k in range(3)] and sorted(os.listdir(tmp_path / "device")) == names
    for name in names:
        a = png.read_png(str(tmp_path / "host" / name))
        assert (tmp_path / "host" / name).read_bytes() == png.encode_png(a, 1), name
        assert np.array_equal(png.read_png(str(tmp_path / "device" / name)), a), name
        want = png.wrap_zlib_stream(D.deflate(K.adaptive_rows(a)), a.shape[1], a.shape[0])
        assert (tmp_path / "device" / name).read_bytes() == want, name
