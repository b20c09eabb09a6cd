"""GPU: csrc/edi.hip against tests/edi_ref.py, bit for bit, frames and flag -- widths that are no multiple of 4 or 64, bases
one byte off, pixels without events, a pixel with 5 000 events, a held pixel, events before s0 and after e1, duplicate
stamps and stamps on the instants, M = 1, 2 and 64, two pairs that share a key beside an item without a right key in one
launch, both exposure modes, an empty stream -- then the runners against the restatement with the network runners' file
names, a ``gt=`` run, and the command lines with ``--method edi`` on a tiny ``simulate`` output, without a checkpoint."""
import functools
import os

import numpy as np
import pytest

import edi_ref as R

pytestmark = pytest.mark.gpu

CP, CN = R.to_fixed(0.2), R.to_fixed(0.17)
ITEMS = [[0, 1], [1, 2], [2, -1]]                               # two pairs that share key 1, and a frame on its own
BOUNDS = [[1.0, 1.5, 2.0, 2.5], [2.0, 2.5, 3.0, 3.5], [3.0, 3.5, 0.0, 0.0]]
INSTANTS = [[1.0, 1.25, 1.75, 2.0, 2.5], [2.0, 2.53125, 2.75, 3.25, 3.5], [3.0, 3.015625, 3.25, 3.5, 3.5]]
CASES = [("5x67", 2, R.SAMPLES), ("5x67", 64, R.SAMPLES), ("3x130", 1, R.SAMPLES), ("3x130", 11, R.SAMPLES), ("5x67", 1, R.CONTINUOUS),
         ("3x130", 1, R.CONTINUOUS)]


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(frames uint8 (3, H, W, 3), events float32 (E, 4)) of a case, read-only.  Stamps lie on a grid of 1/64 from 0.5 to 4.5, so
    they repeat, fall on the bounds and the instants, and lie before the first s0 and after the last e1; a third of the
    pixels have no events; pixel 1 carries 5 000 events of alternating sign, pixel 2 enough of one sign to be held at
    exp(32), pixel 3 the same downwards; some rows lie outside the frame."""
    h, w = (int(v) for v in name.split("x"))
    rng = np.random.default_rng(h * 1000 + w)
    frames = rng.integers(0, 256, size=(3, h, w, 3), dtype=np.uint8)
    n = 12 * h * w
    pix = rng.integers(0, h * w, size=n)
    pix = pix[pix % 3 != 0]
    t = rng.integers(32, 289, size=len(pix)) / 64.0
    p = rng.choice([1.0, -1.0, 0.0], size=len(pix), p=[0.5, 0.4, 0.1])
    rows = [np.stack([t, pix % w + rng.random(len(pix)) * 0.9, pix // w, p], axis=1)]
    k = np.arange(5000)
    rows.append(np.stack([0.75 + k * (3.5 / 5000), np.full(5000, 1.0), np.zeros(5000), np.where(k % 2 == 0, 1.0, -1.0)], axis=1))
    k = np.arange(400)
    rows.append(np.stack([1.0 + (k + 1) / 128.0, np.full(400, 2.0), np.zeros(400), np.ones(400)], axis=1))
    rows.append(np.stack([1.0 + (k + 1) / 128.0, np.full(400, 3.0), np.zeros(400), -np.ones(400)], axis=1))
    rows.append(np.array([[1.5, -1.0, 0, 1], [1.5, w, 0, 1], [2.0, 0, h, 1], [2.5, 0, -3.0, -1], [3.0, float("nan"), 0, 1]]))
    ev = np.concatenate(rows).astype(np.float32)
    ev = ev[np.argsort(ev[:, 0], kind="stable")]
    frames.setflags(write=False)
    ev.setflags(write=False)
    return frames, ev


@functools.lru_cache(maxsize=None)
def _want(name, m, exposure):
    frames, ev = _scene(name)
    out, held = R.edi(frames, R.load(ev, *frames.shape[1:3]), ITEMS, BOUNDS, INSTANTS, m, exposure, CP, CN)
    out.setflags(write=False)
    return out, held


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _mode(exposure):
    return "samples" if exposure == R.SAMPLES else "continuous"


def _run(frames, ev, m, exposure, items=ITEMS, bounds=BOUNDS, instants=INSTANTS, **kw):
    from refid_amd import edi, ops
    stream = edi.EdiStream().load(_dev(ev) if len(ev) else ev, frames.shape[1], frames.shape[2])
    out, held = ops.edi(frames, stream, np.array(items), bounds, instants, m=m, exposure=_mode(exposure), c_pos=CP, c_neg=CN, **kw)
    return out, int(held.sum()), stream


@pytest.mark.parametrize("name,m,exposure", CASES)
def test_the_device_equals_the_restatement(name, m, exposure):
    frames, ev = _scene(name)
    want, want_held = _want(name, m, exposure)
    got, held, stream = _run(_dev(frames), ev, m, exposure)
    assert str(got.dtype) == "torch.uint8" and tuple(got.shape) == want.shape == (3, 5) + frames.shape[1:]
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert held == want_held and held >= 4                      # pixels 2 and 3, in the items that see their events
    assert stream.dropped == R.load(ev, *frames.shape[1:3])[1] == 5 and stream.unsorted == 0
    assert not np.array_equal(want[0, 0], want[0, 2])           # (the events do something)


@pytest.mark.parametrize("exposure", [R.SAMPLES, R.CONTINUOUS])
def test_bases_one_byte_off(exposure):
    import torch
    frames, ev = _scene("5x67")
    want, want_held = _want("5x67", 2, exposure)
    buf = torch.zeros((frames.size + 1,), dtype=torch.uint8, device="cuda")
    buf[1:].copy_(_dev(frames).reshape(-1))
    out = torch.full((want.size + 2,), 7, dtype=torch.uint8, device="cuda")
    got, held, _ = _run(buf[1:].view(frames.shape), ev, 2, exposure, out=out[1:-1])
    assert got.data_ptr() % 2 == 1 and got.cpu().numpy().tobytes() == want.tobytes() and held == want_held
    assert int(out[0]) == 7 and int(out[-1]) == 7               # nothing outside `out` is written


def test_an_empty_stream_and_a_stream_outside_the_items():
    frames, ev = _scene("3x130")
    for rows in (np.zeros((0, 4), dtype=np.float32), ev[(ev[:, 0] < 1.0) | (ev[:, 0] > 3.5)]):
        for exposure in (R.SAMPLES, R.CONTINUOUS):
            want, want_held = R.edi(frames, R.load(rows, 3, 130), ITEMS, BOUNDS, INSTANTS, 3, exposure, CP, CN)
            got, held, _ = _run(_dev(frames), rows, 3, exposure)
            assert got.cpu().numpy().tobytes() == want.tobytes() and held == want_held == 0
    assert np.array_equal(want[2, 0], frames[2]) and np.array_equal(want[0, 0], frames[0]) and np.array_equal(want[0, 4], frames[1])


def test_ops_edi_turns_bad_arguments_down():
    import torch
    from refid_amd import edi, ops
    from refid_amd._lib import RefidHipError
    frames, ev = _scene("5x67")
    dev, ev = _dev(frames), _dev(ev)
    stream = edi.EdiStream().load(ev, 5, 67)
    call = lambda **kw: ops.edi(**{**dict(frames_u8=dev, stream=stream, items=np.array(ITEMS), bounds=BOUNDS, instants=INSTANTS, m=2,  # noqa: E731
                                          c_pos=CP, c_neg=CN), **kw})
    for kw, word in ((dict(stream=edi.EdiStream().load(ev, 5, 66)), "stream is 5x66"), (dict(m=65), "m 65 must be 1 .. 64"),
                     (dict(c_pos=0.2), "c_pos 0.2 must be an int"), (dict(exposure="open"), "unknown exposure 'open'"),
                     (dict(instants=[[1.5, 1.25]] * 3), "instants\\[0\\] is not ascending"),
                     (dict(instants=[[1.0, 2.6]] * 3), "instants\\[0\\]\\[1\\] = 2.5999999 lies outside \\[1, 2.5\\]"),
                     (dict(items=np.array([[0, 3], [1, 2], [2, -1]])), "items\\[0\\]: right 3 lies outside the n_frames 3"),
                     (dict(bounds=[[1.0, 2.5, 2.0, 2.5]] * 3), "bounds\\[0\\] = .* is not ordered"),
                     (dict(out=torch.zeros(5, dtype=torch.uint8, device="cuda")), "out must be a contiguous uint8 tensor of 3\\*5\\*5\\*67\\*3")):
        with pytest.raises(RefidHipError, match=word):
            call(**kw)


# ---- the runners and the command lines ----

def _stamps(n):
    return np.arange(n, dtype=np.float64) / 240.0


@functools.lru_cache(maxsize=None)
def _simulated():
    """A 17 x 35 clip of 13 frames that drifts, its reference events, and blurry keys of M = 3, N = 1 (three keys, two pairs)."""
    import blur_ref
    import event_sim_ref as S
    h, w, n = 17, 35, 13
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    clip = np.stack([np.rint(127 + 100 * np.sin((x - 1.5 * k + 0.5 * y) / 4.0))[..., None].repeat(3, -1).astype(np.uint8) for k in range(n)])
    lut = S.default_lut()
    c = R.to_fixed(0.1)
    ev = S.simulate(clip, _stamps(n), S.reset(clip[0], lut), lut, c, c)[0]
    windows, _ = blur_ref.blur_windows(n, 3, 1)
    return clip, ev, blur_ref.blur_synth(clip, windows), blur_ref.exposures(_stamps(n), windows)


def test_the_interpolator_equals_the_restatement_and_names_its_files_as_the_network_runner(tmp_path):
    from refid_amd import edi, png, sequence
    clip, ev, keys, expo = _simulated()
    assert keys.shape[0] == 3
    pairs = edi.exposure_pairs(expo[:, 0], expo[:, 1])
    assert [tuple(p[:6]) for p in pairs] == [tuple(p) for p in sequence.make_pairs(ev[:0, 0], *sequence.exposure_windows(expo[:, 0], expo[:, 1]),
                                                                                  stamps="bounds")]
    runner = edi.EdiInterpolator(3, 1, "blur", c_pos=0.1, c_neg=0.1, max_minibatch=2)
    got = runner.run(keys, ev, pairs, out_dir=str(tmp_path / "out"), keep=True, gt=clip[[0, 1, 2, 3, 4, 5, 6, 4, 5, 6, 7, 8, 9, 10]])
    bounds = np.array([[p.first_stamp, p.left_end, p.right_start, p.last_stamp] for p in pairs], dtype=np.float32)
    instants = np.stack([R.output_instants("blur", b, 3, 1) for b in bounds])
    c = R.to_fixed(0.1)
    want, held = R.edi(keys, R.load(ev, 17, 35), [[0, 1], [1, 2]], bounds, instants, 3, R.SAMPLES, c, c)
    assert got.shape == (2, 7, 17, 35, 3) and got.tobytes() == want.tobytes()
    assert (runner.clamped, runner.dropped) == (held, 0)
    names = [os.path.basename(p) for k in range(2) for p in sequence.SequenceInterpolator._paths(None, "", f"{k:06d}", np.zeros((7, 1)))]
    assert sorted(os.listdir(tmp_path / "out")) == names
    assert png.read_png(str(tmp_path / "out" / "000001_03.png")).tobytes() == want[1, 3].tobytes()
    assert [(name, f) for name, f, _ in runner.scores] == [(f"{k:06d}", f) for k in range(2) for f in range(7)]
    blurry = [10 * np.log10(255.0 ** 2 / np.mean((keys[0].astype(float) - clip[f]) ** 2)) for f in range(3)]
    # the closed loop, on the device: the ends of the exposure gain 13 dB (the middle frame is what the blur resembles most)
    assert all(runner.scores[f][2].psnr > blurry[f] + 6.0 for f in (0, 2))
    # sharp key frames from make_pairs' bounds; the deblurrer at the middle of the exposures
    sharp = edi.EdiInterpolator(1, 2, "sharp", c_pos=0.1, c_neg=0.1)
    s = _stamps(13)[::4]
    got = sharp.run(clip[::4], ev, sequence.make_pairs(ev[:, 0], *sequence.sharp_windows(s), stamps="bounds"), keep=True)
    b = np.array([[s[k], s[k], s[k + 1], s[k + 1]] for k in range(3)], dtype=np.float32)
    want, _ = R.edi(clip[::4], R.load(ev, 17, 35), [[0, 1], [1, 2], [2, 3]], b, np.stack([R.output_instants("sharp", r, n=2) for r in b]), 1,
                    R.SAMPLES, c, c)
    assert got.shape == (3, 2, 17, 35, 3) and got.tobytes() == want.tobytes()
    deb = edi.EdiDeblurrer(3, c_pos=0.1, c_neg=0.1, exposure="continuous", max_minibatch=2)
    items = sequence.make_pairs(ev[:, 0], *sequence.frame_windows(expo[:, 0], expo[:, 1]), stamps="bounds")
    got = deb.run(keys, ev, items, out_dir=str(tmp_path / "deb"), keep=True)
    b = np.array([[p.first_stamp, p.last_stamp, 0, 0] for p in items], dtype=np.float32)
    want, _ = R.edi(keys, R.load(ev, 17, 35), [[k, -1] for k in range(3)], b, np.stack([R.output_instants("single", r) for r in b]), 3,
                    R.CONTINUOUS, c, c)
    assert got.shape == (3, 17, 35, 3) and got.tobytes() == want[:, 0].tobytes()
    assert sorted(os.listdir(tmp_path / "deb")) == [f"{k:06d}.png" for k in range(3)]


def test_the_closed_loop_of_the_command_lines_needs_no_checkpoint(tmp_path, capsys):
    import glob
    from refid_amd import deblur, interpolate, simulate
    clip = _simulated()[0]
    np.save(str(tmp_path / "clip.npy"), clip)
    sim = str(tmp_path / "sim")
    assert simulate.main(["--frames", str(tmp_path / "clip.npy"), "--fps", "240", "--out", sim, "--blur", "3", "--gap", "1",
                          "--c-pos", "0.1", "--c-neg", "0.1"]) == 0
    common = ["--method", "edi", "--frames", os.path.join(sim, "keys"), "--events", *sorted(glob.glob(os.path.join(sim, "events", "*.npz"))),
              "--stamps", os.path.join(sim, "key_stamps.txt"), "--c-pos", "0.1", "--c-neg", "0.1"]
    capsys.readouterr()
    assert interpolate.main(common + ["--layout", "blur", "--m", "3", "--n", "1", "--gt", os.path.join(sim, "gt"),
                                      "--out", str(tmp_path / "out")]) == 0
    said = capsys.readouterr()
    assert "edi: 0 clamped pixels, 0 dropped event rows" in said.out and "no checkpoint" not in said.err
    lines = open(tmp_path / "out" / "scores.txt").read().split("\n")
    assert len(lines) == 1 + 2 * 7 + 2 and lines[1].startswith("000000_00.png ") and lines[-2].startswith("mean ")
    assert float(lines[-2].split()[1]) > 25.0
    assert deblur.main(common + ["--m", "3", "--gt", os.path.join(sim, "gt_mid"), "--out", str(tmp_path / "deb")]) == 0
    assert "edi: 0 clamped pixels" in capsys.readouterr().out
    lines = open(tmp_path / "deb" / "scores.txt").read().split("\n")
    assert len(lines) == 1 + 3 + 2 and lines[1].startswith("000000.png ") and float(lines[-2].split()[1]) > 30.0
