"""MI355X: refid_jpeg_encode (csrc/jpeg.hip) through ops.jpeg_encode, validation.VideoWriter, both sequence runners and both
command lines.

Every comparison is exact equality of bytes: the kernels are integer arithmetic, so there is no tolerance anywhere.  The
expected files are tests/jpeg_ref.py's (pinned to PIL and a float64 DCT by test_jpeg_ref_host.py), over the cases of
tests/jpeg_cases.py: seven frame shapes x six data families (the six frames of a shape go through one launch as a batch) x
qualities 1, 50, 90, 100 x both subsamplings x restart intervals of 1, 2, 3 MCUs and one MCU row.  Small intervals make a
small frame span many workgroups, and the segments then start at every byte alignment."""
import ctypes

import numpy as np
import pytest
import torch

import jpeg_cases as K
import jpeg_ref as J

pytestmark = pytest.mark.gpu


def _run(frames, quality, subsampling, restart_mcus, **kw):
    from refid_amd import ops
    out, lens = ops.jpeg_encode(torch.from_numpy(np.array(frames)).cuda(), quality, subsampling, restart_mcus, **kw)
    assert out.dtype == torch.uint8 and lens.dtype == torch.int32 and tuple(lens.shape) == (frames.shape[0],)
    return out.cpu().numpy(), lens.cpu().numpy()


def _same(out, lens, want, what):
    for k, stream in enumerate(want):
        assert int(lens[k]) == len(stream), (what, k, int(lens[k]), len(stream))
        got = out[k, :len(stream)].tobytes()
        if got != stream:
            bad = [i for i in range(len(stream)) if got[i] != stream[i]]
            raise AssertionError(f"{what}, frame {k}: {len(bad)} of {len(stream)} bytes differ, first at {bad[0]}: "
                                 f"got {got[bad[0]]:#04x}, want {stream[bad[0]]:#04x}")


@pytest.mark.parametrize("subsampling", K.SUBSAMPLINGS)
@pytest.mark.parametrize("quality", K.QUALITIES)
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_files_and_lengths_equal_the_restatement(shape, quality, subsampling):
    h, w = shape
    frames = K.frames_of(h, w)
    ss = J.SUBSAMPLINGS[subsampling]
    for restart in K.RESTARTS:
        want = K.expected(h, w, quality, subsampling, restart)[0]
        out, lens = _run(frames, quality, subsampling, restart, pitch="bound")
        assert out.shape == (len(K.FAMILIES), J.bound(h, w, ss, restart))
        _same(out, lens, want, f"{h}x{w} q{quality} {subsampling} restart {restart}")
    fits = [k for k, stream in enumerate(want) if len(stream) <= J.default_pitch(h, w)]
    out, lens = _run(frames, quality, subsampling, None)      # the default pitch: the files that fit are the same
    assert out.shape == (len(K.FAMILIES), J.default_pitch(h, w))
    _same(out[fits], lens[fits], [want[k] for k in fits], f"{h}x{w} q{quality} {subsampling} at the default pitch")
    for k in set(range(len(want))) - set(fits):
        assert int(lens[k]) == -len(want[k]), (k, int(lens[k]), len(want[k]))


@pytest.mark.parametrize("shape,subsampling,restart", [((9, 700), "444", None), ((9, 700), "420", None), ((24, 410), "444", 50),
                                                       ((130, 140), "444", 1), ((40, 420), "420", 65535)])
def test_segments_longer_than_a_pass_and_frames_of_many_segments(shape, subsampling, restart):
    """The code kernel takes 128 blocks per pass, the place kernel 4096 parked bytes, the offsets kernel 256 segments per
    round: 9x700 has 264 blocks per MCU row (three passes, DC predictors and the open word carried across them), 24x410 at
    50 MCUs per interval 150 blocks and a short last segment, 130x140 at one MCU per interval 306 segments, and 40x420 as ONE
    segment of 486 blocks whose noise frame parks some 20 KiB."""
    h, w = shape
    frames = K.frames_of(h, w)
    for quality in (90, 100):
        want = K.expected(h, w, quality, subsampling, restart)[0]
        out, lens = _run(frames, quality, subsampling, restart, pitch="bound")
        _same(out, lens, want, f"{h}x{w} q{quality} {subsampling} restart {restart}")


def test_a_file_does_not_depend_on_its_place_or_on_the_run():
    from refid_amd import ops
    frames = K.frames_of(33, 65)
    pick = [K.FAMILIES.index(f) for f in ("waves", "noise", "saturated")]
    for subsampling, restart in (("420", 2), ("444", None)):
        want = K.expected(33, 65, 90, subsampling, restart)[0]
        dev = torch.from_numpy(frames[pick].copy()).cuda()
        three, lens3 = ops.jpeg_encode(dev, 90, subsampling, restart, pitch="bound")
        _same(three.cpu().numpy(), lens3.cpu().numpy(), [want[k] for k in pick], "three frames in one call")
        for k in range(3):
            alone, lens1 = ops.jpeg_encode(dev[k:k + 1], 90, subsampling, restart, pitch="bound")
            n = int(lens1[0])
            assert n == int(lens3[k]) and torch.equal(alone[0, :n], three[k, :n]), k
        again, lens_again = ops.jpeg_encode(dev, 90, subsampling, restart, pitch="bound")
        assert torch.equal(lens_again, lens3)
        for k in range(3):
            assert torch.equal(again[k, :int(lens3[k])], three[k, :int(lens3[k])]), k


@pytest.mark.parametrize("shape,quality,subsampling,restart", [((1, 1), 90, "420", None), ((7, 9), 100, "444", 1), ((17, 35), 50, "420", 2),
                                                               ((33, 65), 100, "444", 1), ((5, 131), 90, "420", 3)])
def test_nothing_is_written_outside_out_lens_and_work_at_any_alignment(shape, quality, subsampling, restart):
    """``frames`` and ``out`` inside larger buffers at each of the four byte alignments, ``lens`` and ``work`` inside larger
    buffers too, canaries all round; the pitch is a little more than the bound, and the bytes behind a file stay."""
    from refid_amd import _lib, ops
    h, w = shape
    frames = K.frames_of(h, w)
    want = K.expected(h, w, quality, subsampling, restart)[0]
    n, size, ss = frames.shape[0], h * w * 3, J.SUBSAMPLINGS[subsampling]
    L = _lib.lib()
    pitch = J.bound(h, w, ss, restart) + 3
    work_words = J.work_bytes(n, h, w, ss, restart) // 4
    assert L.refid_jpeg_work_bytes(n, h, w, ss, restart or 0) == 4 * work_words
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for shift in range(4):
        big = torch.full((64 + n * pitch + 64 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        start = 64 + (shift - (big.data_ptr() + 64)) % 4
        out = big[start:start + n * pitch]
        src_big = torch.zeros((n * size + 8,), dtype=torch.uint8, device="cuda")
        src_start = (3 - shift - src_big.data_ptr()) % 4       # the input at another alignment than the output
        src = src_big[src_start:src_start + n * size]
        src.copy_(torch.from_numpy(frames.reshape(-1).copy()))
        assert out.data_ptr() % 4 == shift and src.data_ptr() % 4 == 3 - shift
        lens_big = torch.full((n + 32,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        work_big = torch.full((work_words + 32,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        desc = _lib.JpegDesc(frames=src.data_ptr(), out=out.data_ptr(), lens=lens_big[16:].data_ptr(), work=work_big[16:].data_ptr(),
                             n_frames=n, height=h, width=w, quality=quality, subsampling=ss, restart_mcus=restart or 0, out_pitch=pitch)
        ops.check(L.refid_jpeg_encode(ctypes.byref(desc), stream), "refid_jpeg_encode")
        host = big.cpu().numpy()
        lens = lens_big.cpu().numpy()
        _same(host[start:start + n * pitch].reshape(n, pitch), lens[16:16 + n], want, f"{h}x{w} at alignment {shift}")
        assert (host[:start] == 0xA5).all() and (host[start + n * pitch:] == 0xA5).all(), shift
        for k in range(n):
            assert (host[start + k * pitch + len(want[k]):start + (k + 1) * pitch] == 0xA5).all(), (shift, k)
        assert (lens[:16] == 0x5A5A5A5A).all() and (lens[16 + n:] == 0x5A5A5A5A).all(), shift
        work = work_big.cpu().numpy()
        assert (work[:16] == 0x5A5A5A5A).all() and (work[16 + work_words:] == 0x5A5A5A5A).all(), shift


def test_a_file_that_does_not_fit_reports_its_need_and_leaves_its_neighbours():
    """Noise at quality 100 in 4:4:4 is longer than the default pitch: lens is minus the exact need, the slots either side hold
    their files, nothing is written outside the buffer; the same call with pitch='bound' fits."""
    from refid_amd import ops
    h, w = 33, 65
    frames = K.frames_of(h, w)
    want = K.expected(h, w, 100, "444", None)[0]
    noise = K.FAMILIES.index("noise")
    pitch = J.default_pitch(h, w)
    assert len(want[noise]) > pitch and all(len(want[k]) <= pitch for k in (noise - 1, noise + 1))
    pick = [noise - 1, noise, noise + 1]
    dev = torch.from_numpy(frames[pick].copy()).cuda()
    big = torch.full((64 + 3 * pitch + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    out, lens = ops.jpeg_encode(dev, 100, "444", None, out=big[64:64 + 3 * pitch].view(3, pitch))
    host, lens = big.cpu().numpy(), lens.cpu().numpy()
    assert lens.tolist() == [len(want[noise - 1]), -len(want[noise]), len(want[noise + 1])]
    slots = host[64:64 + 3 * pitch].reshape(3, pitch)
    for k in (0, 2):
        assert slots[k, :lens[k]].tobytes() == want[pick[k]] and (slots[k, lens[k]:] == 0xA5).all(), k
    assert (host[:64] == 0xA5).all() and (host[64 + 3 * pitch:] == 0xA5).all()
    out, lens = ops.jpeg_encode(dev, 100, "444", None, pitch="bound")
    _same(out.cpu().numpy(), lens.cpu().numpy(), [want[k] for k in pick], "with pitch='bound'")


def test_rejected_arguments():
    from refid_amd import _lib, ops
    good = torch.zeros((2, 9, 13, 3), dtype=torch.uint8, device="cuda")
    for bad in (good.cpu(), good.float(), good[0], good[..., :2], good[:0], good.cpu().numpy(), good[:, :, ::2]):
        with pytest.raises(_lib.RefidHipError, match="jpeg_encode: a non-empty contiguous uint8 CUDA tensor"):
            ops.jpeg_encode(bad)
    for quality in (0, 101, -3, 90.0, True, "high"):
        with pytest.raises(_lib.RefidHipError, match="jpeg_encode: quality"):
            ops.jpeg_encode(good, quality)
    for subsampling in ("422", 420, None, "4:2:0"):
        with pytest.raises(_lib.RefidHipError, match="jpeg_encode: subsampling"):
            ops.jpeg_encode(good, 90, subsampling)
    for restart in (0, -1, 65536, 2.0, True):
        with pytest.raises(_lib.RefidHipError, match="jpeg_encode: restart_mcus"):
            ops.jpeg_encode(good, 90, "420", restart)
    for pitch in (626, 0, -1, 2 ** 31, 700.0, "big"):
        with pytest.raises(_lib.RefidHipError, match="jpeg_encode: pitch"):
            ops.jpeg_encode(good, pitch=pitch)
    for out in (torch.empty((2, 626), dtype=torch.uint8, device="cuda"), torch.empty((2, 700), dtype=torch.uint8),
                torch.empty((2, 700), dtype=torch.int8, device="cuda"), torch.empty((3, 700), dtype=torch.uint8, device="cuda"),
                torch.empty((2, 1400), dtype=torch.uint8, device="cuda")[:, ::2], torch.empty(1400, dtype=torch.uint8, device="cuda")):
        with pytest.raises(_lib.RefidHipError, match="jpeg_encode: out must be"):
            ops.jpeg_encode(good, out=out)
    with pytest.raises(_lib.RefidHipError, match="jpeg_encode: give pitch or out"):
        ops.jpeg_encode(good, pitch=700, out=torch.empty((2, 700), dtype=torch.uint8, device="cuda"))
    out = torch.empty((2, 700), dtype=torch.uint8, device="cuda")
    got, lens = ops.jpeg_encode(good, out=out)
    assert got.data_ptr() == out.data_ptr() and lens.tolist() == [len(J.encode(np.zeros((9, 13, 3), dtype=np.uint8)))] * 2


# ---- validation.VideoWriter --------------------------------------------------------------------------------------------------
def test_video_writer_appends_the_restatements_files_in_order(tmp_path):
    """Three batches through both pinned slots and back to the first: the container holds, in submission order, exactly the
    files the restatement gives for the frames; PIL opens each of them."""
    from refid_amd.validation import VideoWriter
    from refid_amd.video import read_mjpeg_avi
    frames = K.frames_of(33, 65)
    dev = torch.from_numpy(frames.copy()).cuda()
    for subsampling, quality in (("420", 90), ("444", 50)):
        path = tmp_path / subsampling / "clip.avi"
        writer = VideoWriter(torch.device("cuda"), str(path), 25, quality=quality, subsampling=subsampling)
        order = [0, 1, 2, 3, 4, 5, 1, 0]
        try:
            for lo, hi in ((0, 3), (3, 4), (4, 8)):
                writer.add(dev[order[lo:hi]])
        finally:
            writer.close()
        assert writer.paths == [str(path)] and writer.frames == 8
        head, got = read_mjpeg_avi(str(path))
        want = K.expected(33, 65, quality, subsampling, None)[0]
        assert got == [want[k] for k in order]
        assert (head["width"], head["height"], head["frames"], head["rate"], head["scale"]) == (65, 33, 8, 25, 1)
    try:
        from PIL import Image
    except ImportError:
        return
    import io
    for data in got:
        with Image.open(io.BytesIO(data)) as im:
            im.load()
            assert im.size == (65, 33)


def test_video_writer_names_the_frame_that_does_not_fit(tmp_path):
    from refid_amd import _lib
    from refid_amd.validation import VideoWriter
    from refid_amd.video import read_mjpeg_avi
    frames = K.frames_of(33, 65)
    noise = K.FAMILIES.index("noise")
    want = K.expected(33, 65, 100, "444", None)[0]
    dev = torch.from_numpy(frames.copy()).cuda()
    writer = VideoWriter(torch.device("cuda"), str(tmp_path / "short.avi"), 30, quality=100, subsampling="444")
    writer.add(dev[:2])
    writer.add(dev[2:])                                       # noise is frame 2 of the video
    with pytest.raises(_lib.RefidHipError, match=rf"frame {noise} needs {len(want[noise])} bytes.*jpeg_pitch='bound'"):
        writer.close()
    assert read_mjpeg_avi(str(tmp_path / "short.avi"))[1] == want[:2]           # the frames in front of it, a closed container
    writer = VideoWriter(torch.device("cuda"), str(tmp_path / "bound.avi"), 30, quality=100, subsampling="444", jpeg_pitch="bound")
    writer.add(dev)
    writer.close()
    assert read_mjpeg_avi(str(tmp_path / "bound.avi"))[1] == want
    for kw, word in ((dict(quality=0), "video_quality"), (dict(subsampling="422"), "video_subsampling"), (dict(fps=0), "video_fps"),
                     (dict(jpeg_pitch=5), "jpeg_pitch"), (dict(jpeg_pitch="all"), "jpeg_pitch")):
        with pytest.raises(_lib.RefidHipError, match=word):
            VideoWriter(**dict(dict(device=torch.device("cuda"), path=str(tmp_path / "x.avi"), fps=30), **kw))


# ---- the sequence runners ----------------------------------------------------------------------------------------------------
def _files(root):
    import os
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_interpolator_video_order_keys_and_untouched_pngs(tmp_path):
    """Pairs (0,1) (1,2) (2,3) (3,4) | (2,3) | (0,0): a run of four consecutive pairs, then two gaps.  With key frames the
    video is K0 o o o K1 o o o K2 o o o K3 o o o K4 | K2 o o o K3 | K0 o o o K0, every frame the restatement's file of the
    frame that belongs there; without them the outputs alone.  The PNGs and keep=True do not notice the video."""
    from refid_amd import _lib
    from refid_amd.sequence import SequenceInterpolator
    from refid_amd.video import read_mjpeg_avi
    from test_hip_sequence import _case, _net
    for name in ("sharp_37x50_rgb", "sharp_37x50_bgr"):
        c = _case(name, "events")
        pairs = c["pairs"][:6]
        assert [(p.left, p.right) for p in pairs] == [(0, 1), (1, 2), (2, 3), (3, 4), (2, 3), (0, 0)]
        keys = c["frames"][..., ::-1] if c["bgr"] else c["frames"]
        interp = SequenceInterpolator(_net(), 1, 3, "sharp", max_minibatch=4)       # minibatches of 4 and 2: a gap inside, a gap at the seam
        root = tmp_path / name
        names = [f"p{k}" for k in range(6)]                                         # (the default names, the left key frame's, repeat)
        plain = interp.run(c["frames"], c["events"], pairs, out_dir=str(root / "plain"), names=names, keep=True, bgr=c["bgr"])
        assert interp.video_paths is None
        got = interp.run(c["frames"], c["events"], pairs, out_dir=str(root / "both"), names=names, keep=True, bgr=c["bgr"],
                         video=str(root / "keys.avi"), video_fps=24)
        assert np.array_equal(got, plain) and interp.video_paths == [str(root / "keys.avi")]
        assert _files(root / "both") == _files(root / "plain") and len(_files(root / "plain")) == 18
        for rel in _files(root / "plain"):
            assert (root / "both" / rel).read_bytes() == (root / "plain" / rel).read_bytes(), rel
        want = []
        for k, (left, right) in enumerate([(p.left, p.right) for p in pairs]):
            want += [keys[left]] + list(got[k])
            if k + 1 == len(pairs) or pairs[k + 1].left != right:
                want.append(keys[right])
        assert len(want) == 6 * 3 + 6 + 3
        head, frames = read_mjpeg_avi(str(root / "keys.avi"))
        assert (head["width"], head["height"], head["frames"], head["rate"], head["scale"]) == (50, 37, 27, 24, 1)
        assert frames == [J.encode(np.ascontiguousarray(f), 90, J.J420) for f in want]
        assert interp.run(c["frames"], c["events"], pairs, bgr=c["bgr"], video=str(root / "outputs.avi"), video_keys=False,
                          video_quality=50, video_subsampling="444", jpeg_pitch="bound") is None
        head, frames = read_mjpeg_avi(str(root / "outputs.avi"))
        assert frames == [J.encode(f, 50, J.J444) for k in range(6) for f in got[k]] and head["rate"] == 30
    with pytest.raises(_lib.RefidHipError, match="video_quality"):
        interp.run(c["frames"], c["events"], pairs, video=str(tmp_path / "x.avi"), video_quality=101)


def test_video_keys_are_rejected_outside_the_sharp_layout():
    from refid_amd import _lib
    from refid_amd.sequence import SequenceDeblurrer
    from test_hip_sequence_single import _net, _sequence, _items
    frames, ev, _ = _sequence()
    deb = SequenceDeblurrer(_net(), 6, max_minibatch=2)
    with pytest.raises(TypeError):
        deb.run(frames, ev, _items(), video="x.avi", video_keys=True)                  # the deblurrer has no such keyword
    from refid_amd.sequence import _SequenceRunner
    with pytest.raises(_lib.RefidHipError, match="video_keys needs sharp key frames"):
        _SequenceRunner.run(deb, frames, ev, _items(), video="x.avi", video_keys=True)


def test_deblurrer_video_holds_the_outputs_in_order(tmp_path):
    from refid_amd.sequence import SequenceDeblurrer
    from refid_amd.video import read_mjpeg_avi
    from test_hip_sequence_single import _net, _sequence, _items
    frames, ev, _ = _sequence()
    items = _items()
    deb = SequenceDeblurrer(_net(), 6, max_minibatch=2)
    plain = deb.run(frames, ev, items, out_dir=str(tmp_path / "plain"), keep=True)
    got = deb.run(frames, ev, items, out_dir=str(tmp_path / "both"), keep=True, video=str(tmp_path / "v" / "clip.avi"),
                  video_fps=12.5, video_quality=75, video_subsampling="444")
    assert np.array_equal(got, plain) and _files(tmp_path / "both") == _files(tmp_path / "plain")
    for rel in _files(tmp_path / "plain"):
        assert (tmp_path / "both" / rel).read_bytes() == (tmp_path / "plain" / rel).read_bytes(), rel
    head, video = read_mjpeg_avi(str(tmp_path / "v" / "clip.avi"))
    assert video == [J.encode(f, 75, J.J444) for f in got]
    assert (head["frames"], head["rate"], head["scale"], head["width"], head["height"]) == (len(items), 25, 2, got.shape[2], got.shape[1])


# ---- the command lines -------------------------------------------------------------------------------------------------------
def test_the_interpolation_command_line_writes_a_video_without_out(tmp_path):
    """The fixture of test_hip_png_deflate.py's command-line test: --video without --out writes the AVI and no PNG; with both,
    the PNGs are those of a run without --video; --video-no-keys leaves the key frames out."""
    import os
    from oracle import refid_oracle as O
    from refid_amd import interpolate, png
    from refid_amd.video import read_mjpeg_avi
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
    (tmp_path / "t.yml").write_text(TEST_YAML.replace("num_inter_interpolation: 7", "num_inter_interpolation: 3"))
    torch.save({"params": O.make_params(6, base_num_channels=8, mode="hash", seed=3)}, tmp_path / "w.pth")
    common = ["--opt", str(tmp_path / "t.yml"), "--checkpoint", str(tmp_path / "w.pth"), "--events", str(tmp_path / "e.npz"),
              "--stamps", str(tmp_path / "stamps.txt"), "--frames", str(tmp_path / "frames.npy")]
    assert interpolate.main([*common, "--out", str(tmp_path / "plain")]) == 0
    assert interpolate.main([*common, "--video", str(tmp_path / "only" / "clip.avi"), "--video-fps", "30000/1001"]) == 0
    assert os.listdir(tmp_path / "only") == ["clip.avi"]
    assert interpolate.main([*common, "--out", str(tmp_path / "both"), "--video", str(tmp_path / "nokeys.avi"), "--video-no-keys",
                             "--video-quality", "75", "--video-subsampling", "444"]) == 0
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == [f"{k:06d}_{f:02d}.png" for k in range(2) for f in range(3)] and sorted(os.listdir(tmp_path / "both")) == names
    outputs = [png.read_png(str(tmp_path / "plain" / name)) for name in names]
    for name in names:
        assert (tmp_path / "both" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes(), name
    head, video = read_mjpeg_avi(str(tmp_path / "only" / "clip.avi"))
    order = [frames[0], *outputs[:3], frames[1], *outputs[3:], frames[2]]               # K0 o o o K1 o o o K2
    assert video == [J.encode(f, 90, J.J420) for f in order] and (head["rate"], head["scale"]) == (30000, 1001)
    head, video = read_mjpeg_avi(str(tmp_path / "nokeys.avi"))
    assert video == [J.encode(f, 75, J.J444) for f in outputs] and (head["rate"], head["scale"]) == (30, 1)
    for flags, word in ((["--video-quality", "0"], "--video-quality"), (["--video-fps", "fast"], "--video-fps"),
                        (["--video-subsampling", "422"], "--video-subsampling")):
        with pytest.raises(SystemExit, match=word):
            interpolate.main([*common, "--video", str(tmp_path / "x.avi"), *flags])
    with pytest.raises(SystemExit, match="--out, --video or both"):
        interpolate.main(common)


def test_the_deblurring_command_line_writes_a_video_without_out(tmp_path):
    import os
    from refid_amd import deblur, png
    from refid_amd.video import read_mjpeg_avi
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
    assert deblur.main([*common, "--out", str(tmp_path / "plain")]) == 0
    assert deblur.main([*common, "--video", str(tmp_path / "only" / "clip.avi"), "--video-fps", "15"]) == 0
    assert os.listdir(tmp_path / "only") == ["clip.avi"]
    names = sorted(os.listdir(tmp_path / "plain"))
    outputs = [png.read_png(str(tmp_path / "plain" / name)) for name in names]
    head, video = read_mjpeg_avi(str(tmp_path / "only" / "clip.avi"))
    assert len(names) == 3 and video == [J.encode(f, 90, J.J420) for f in outputs] and head["rate"] == 15
    with pytest.raises(SystemExit):
        deblur.main([*common, "--video", str(tmp_path / "x.avi"), "--video-no-keys"])       # an interpolation flag
    with pytest.raises(SystemExit, match="--video-quality"):
        deblur.main([*common, "--video", str(tmp_path / "x.avi"), "--video-quality", "200"])
