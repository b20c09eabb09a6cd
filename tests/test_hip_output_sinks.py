"""MI355X: the output side of the sequence runners as a whole -- the sinks of ``_SequenceRunner.run`` (PNG, video, NIQE, score,
keep) and the pinned relay under ``validation.FrameWriter`` and ``validation.VideoWriter``.

The kernels behind every output have their own per-element tests; here the outputs are run together and alone, the relay's
slots are reused, regrown and under-filled, and a failing PNG writer meets a video in the same run.  Every comparison is exact:
uint8 frames, integer kernels, and scores that must not depend on which other outputs ran beside them."""
import functools

import numpy as np
import pytest
import torch

from test_hip_niqe import _frames, _model, _net

pytestmark = pytest.mark.gpu

H, W, KEYS = 96, 192, 6                                    # 96x192: the smallest frame with finite NIQE scores; five pairs
STAMPS = [10.0 + 4.0 * k for k in range(KEYS)]


@functools.lru_cache(maxsize=None)
def _sequence():
    """Six key frames cut from the 1/f fixture frame (200x301: offsets up to 104 fit), events over all five windows, the pairs
    and a ground truth per output frame (the right key frame of its pair)."""
    from refid_amd.sequence import make_pairs, sharp_windows
    rng = np.random.Generator(np.random.PCG64(11))
    src = _frames()[1][..., ::-1]
    frames = np.stack([np.ascontiguousarray(src[4 * k:4 * k + H, 4 * k:4 * k + W]) for k in range(KEYS)])
    n = 6000
    ev = np.stack([np.sort(rng.uniform(STAMPS[0], STAMPS[-1], n)), rng.integers(0, W, n), rng.integers(0, H, n),
                   rng.integers(0, 2, n)], axis=1).astype(np.float32)
    ev = np.ascontiguousarray(ev)
    return frames, ev, make_pairs(ev[:, 0], *sharp_windows(STAMPS)), torch.from_numpy(frames[1:].copy())


@pytest.mark.parametrize("mb", [1, 2])
def test_all_outputs_together_equal_each_alone(tmp_path, mb):
    """Five pairs, one interpolated frame each: minibatches 1+1+1+1+1 (each relay slot taken more than once) or 2+2+1 (an
    uneven last one).  One run with PNGs, video, NIQE, ground truth and keep; then one run per output."""
    from refid_amd import png
    from refid_amd.sequence import SequenceInterpolator
    from refid_amd.video import read_mjpeg_avi
    frames, ev, pairs, gt = _sequence()
    assert len(pairs) == KEYS - 1 >= 3
    names = [f"p{k}" for k in range(len(pairs))]
    interp = SequenceInterpolator(_net(), 1, 1, "sharp", max_minibatch=mb)
    run = lambda **kw: interp.run(frames, ev, pairs, names=names, keep=True, **kw)      # noqa: E731
    kept = run(out_dir=str(tmp_path / "all"), video=str(tmp_path / "all.avi"), video_keys=False, niqe=_model(), gt=gt)
    assert kept.shape == (len(pairs), 1, H, W, 3) and interp.video_paths == [str(tmp_path / "all.avi")]
    niqe_all, scores_all = interp.niqe_scores, interp.scores
    video_all = read_mjpeg_avi(str(tmp_path / "all.avi"))[1]
    for k, name in enumerate(names):
        assert np.array_equal(png.read_png(str(tmp_path / "all" / f"{name}_00.png")), kept[k, 0]), name

    assert run().tobytes() == kept.tobytes()                                   # keep alone
    assert (interp.niqe_scores, interp.scores, interp.video_paths) == (None, None, None)
    assert run(out_dir=str(tmp_path / "png")).tobytes() == kept.tobytes()
    for name in names:
        assert (tmp_path / "png" / f"{name}_00.png").read_bytes() == (tmp_path / "all" / f"{name}_00.png").read_bytes(), name
    assert run(video=str(tmp_path / "only.avi"), video_keys=False).tobytes() == kept.tobytes()
    assert len(video_all) == len(pairs) and video_all == read_mjpeg_avi(str(tmp_path / "only.avi"))[1]
    assert run(niqe=_model()).tobytes() == kept.tobytes()
    assert [s[:2] for s in niqe_all] == [(name, 0) for name in names] and np.isfinite([s[2] for s in niqe_all]).all()
    assert interp.niqe_scores == niqe_all and interp.scores is None
    assert run(gt=gt).tobytes() == kept.tobytes()
    assert [s[:2] for s in scores_all] == [(name, 0) for name in names] and all(np.isfinite(s[2].psnr) for s in scores_all)
    assert interp.scores == scores_all and interp.niqe_scores is None


def _patterns(n, h, w, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:h, 0:w]
    base = (90 + 60 * np.sin(xx / 3.0) + 50 * np.cos(yy / 2.0))[None, :, :, None] + np.array([0.0, 20.0, -30.0])
    return np.clip(base + rng.normal(0, 12, (n, h, w, 3)), 0, 255).astype(np.uint8)


def test_relay_slots_are_reused_regrown_and_underfilled(tmp_path):
    """FrameWriter: dumps of 1, 1, 3, 3, 2 frames of 16x20, two batches each (as the validation loop's save_gt): both slots are
    taken, taken again by a larger dump and then by a smaller one.  VideoWriter: adds of 1, 3, 2 frames of 16x16 at a pitch of
    625 + 768 bytes (the header and 3 bytes per pixel; given as ``jpeg_pitch``, because the default pitch is that rounded up to
    4), so the files end off a multiple of 4 and the lengths sit at the next one."""
    from refid_amd import _lib, ops, png
    from refid_amd.validation import FrameWriter, VideoWriter
    from refid_amd.video import read_mjpeg_avi
    counts = [1, 1, 3, 3, 2]
    pred, truth = _patterns(sum(counts), 16, 20, 1), _patterns(sum(counts), 16, 20, 2)
    writer = FrameWriter(torch.device("cuda"), png_filter="adaptive", png_deflate="device")
    try:
        lo = 0
        for n in counts:
            batches = [(torch.from_numpy(a[lo:lo + n]).cuda(), [str(tmp_path / what / f"{k:02d}.png") for k in range(lo, lo + n)])
                       for what, a in (("pred", pred), ("gt", truth))]
            writer.dump(batches)
            lo += n
    finally:
        writer.close()
    for what, a in (("pred", pred), ("gt", truth)):
        for k in range(sum(counts)):
            assert np.array_equal(png.read_png(str(tmp_path / what / f"{k:02d}.png")), a[k]), (what, k)

    adds = [1, 3, 2]
    pitch = _lib.JPEG_HEADER_BYTES + 3 * 16 * 16
    assert pitch == 625 + 768 and all((n * pitch) % 4 for n in adds)
    dev = torch.from_numpy(_patterns(sum(adds), 16, 16, 3)).cuda()
    video = VideoWriter(torch.device("cuda"), str(tmp_path / "clip.avi"), 30, jpeg_pitch=pitch)
    try:
        lo = 0
        for n in adds:
            video.add(dev[lo:lo + n])
            lo += n
    finally:
        video.close()
    out, lens = ops.jpeg_encode(dev, 90, "420", pitch=pitch)
    assert out.shape[1] == pitch and int(lens.min()) > 0
    out, lens = out.cpu().numpy(), lens.cpu().numpy()
    assert read_mjpeg_avi(str(tmp_path / "clip.avi"))[1] == [out[k, :lens[k]].tobytes() for k in range(sum(adds))]


def test_a_failing_png_writer_leaves_a_closed_video_and_the_training_state(tmp_path):
    """The PNG directory lies under a regular file, so every PNG job fails in its worker.  Minibatch 2 takes the slot of
    minibatch 0 again and meets its failure there, in the PNG sink, before the video sink has seen minibatch 2: ``run`` raises
    the writer's error, the AVI is a closed container with the frames of minibatches 0 and 1, and the network trains again."""
    from refid_amd.sequence import SequenceInterpolator
    from refid_amd.video import read_mjpeg_avi
    frames, ev, pairs, _ = _sequence()
    net = _net()
    interp = SequenceInterpolator(net, 1, 1, "sharp", max_minibatch=1)
    assert interp.run(frames, ev, pairs, video=str(tmp_path / "good.avi"), video_keys=False) is None
    good = read_mjpeg_avi(str(tmp_path / "good.avi"))[1]
    blocker = tmp_path / "file"
    blocker.write_text("x")
    net.train()
    with pytest.raises(OSError):
        interp.run(frames, ev, pairs, out_dir=str(blocker / "out"), video=str(tmp_path / "cut.avi"), video_keys=False)
    assert net.training and interp.video_paths == [str(tmp_path / "cut.avi")]
    head, cut = read_mjpeg_avi(str(tmp_path / "cut.avi"))
    assert head["frames"] == 2 and cut == good[:2]
