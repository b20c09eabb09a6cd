"""MI355X: NIQE on the device -- refid_niqe_moments (csrc/niqe.hip) against its numpy restatement (tests/niqe_ref.py), the
sequence runners' ``niqe=`` keyword and the command lines' ``--niqe``.

The Y plane and both normalised maps are single correctly rounded operations in a fixed order, so they are compared BIT
for bit; the counts are integers; the three float64 sums of a map add at most 9216 non-negative terms in another order
than numpy does, so they agree to 2 * 9216 * 2^-53 relative, rounded up to 1e-11; features and scores follow to 1e-9.
Shapes: the four fixture frames (192x192, 200x301 with the crop and 6 blocks, 192x288 with a constant block, white
noise), one 96x96 frame (every filter edge clamped), three frames in one call, crop_border=3 on 198x294.  The launcher
does not cap its grid (one workgroup per block and scale), so there is no wrapped shape."""
import functools
import os
from copy import deepcopy

import numpy as np
import pytest
import torch

import niqe_ref as R
from oracle import refid_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SUM_REL = 1e-11


@functools.lru_cache(maxsize=None)
def _model():
    from refid_amd.niqe import NiqeModel
    return NiqeModel.load(os.path.join(GOLDEN, "niqe_pris_params.npz"))


@functools.lru_cache(maxsize=None)
def _frames():
    z = np.load(os.path.join(GOLDEN, "niqe.npz"))
    return tuple(np.ascontiguousarray(z[f"f{k}_bgr"]) for k in range(int(z["n_frames"])))


CASES = {                                                  # name: (frame, bgr, crop_border)
    "f0_192x192": (lambda: _frames()[0], True, 0),
    "f1_200x301": (lambda: _frames()[1], True, 0),
    "f2_192x288_flat_block": (lambda: _frames()[2], True, 0),
    "f3_192x192_noise": (lambda: _frames()[3], True, 0),
    "one_block_96x96": (lambda: np.ascontiguousarray(_frames()[3][50:146, 7:103]), True, 0),
    "crop3_198x294": (lambda: np.ascontiguousarray(_frames()[1][:198, :294]), False, 3),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The frame and the restatement's stages, computed once and frozen."""
    make, bgr, cb = CASES[name]
    frame = make()
    st = R.frame_stages(frame, _model().window, bgr=bgr, crop_border=cb)
    for v in st.values():
        v.setflags(write=False)
    return frame, bgr, cb, st


def _device(frames, bgr, cb, planes=True):
    from refid_amd import niqe
    u8 = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    out = niqe.moments(u8, _model(), bgr=bgr, crop_border=cb, planes=planes)
    torch.cuda.synchronize()
    if not planes:
        return out.cpu().numpy()
    return out[0].cpu().numpy(), [p.cpu().numpy() for p in out[1]]


def _check_sums(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(got[..., :2], want[..., :2]), f"{what}: counts"
    err = np.abs(got[..., 2:] - want[..., 2:])
    rel = err / np.where(want[..., 2:] != 0, np.abs(want[..., 2:]), 1.0)
    print(f"{what}: largest relative deviation of a float64 sum {rel.max():.3e}")
    assert np.all(err <= SUM_REL * np.abs(want[..., 2:])), f"{what}: sums off by {rel.max():.3e} relative"


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_restatement(name):
    from refid_amd import niqe
    frame, bgr, cb, st = _case(name)
    sums, (y, n1, n2) = _device(frame, bgr, cb)
    for got, key in ((y, "y"), (n1, "mscn1"), (n2, "mscn2")):
        assert got.shape == (1,) + st[key].shape and got.dtype == np.float32
        diff = got[0].view(np.int32) != st[key].view(np.int32)
        assert not diff.any(), f"{name}: {key} differs in {int(diff.sum())} of {diff.size} elements, first at {np.argwhere(diff)[0]}"
    _check_sums(sums[0], st["sums"], name)
    m = _model()
    scores, feats = niqe.finish(sums, m, with_features=True)
    want_score, want_feat = R.finish_ref(st["sums"], m.mu_pris, m.cov_pris)
    assert np.array_equal(np.isnan(feats[0]), np.isnan(want_feat))
    np.testing.assert_allclose(feats[0], want_feat, rtol=1e-9, atol=1e-9, equal_nan=True)
    if name == "one_block_96x96":
        assert np.isnan(scores[0]) and np.isnan(want_score)
    else:
        assert abs(scores[0] - want_score) <= 1e-9
        assert niqe.calculate_niqe_frames(frame, m, bgr=bgr, crop_border=cb) == scores       # the front door, from numpy


def test_fixture_scores_of_the_reference():
    """End to end against what the reference recorded: the device's score inside the restatement's measured bar."""
    from refid_amd import niqe
    z = np.load(os.path.join(GOLDEN, "niqe.npz"))
    for k, frame in enumerate(_frames()):
        got = niqe.calculate_niqe_frames(torch.from_numpy(frame).cuda(), _model(), bgr=True)
        assert len(got) == 1 and abs(got[0] - float(z[f"f{k}_score"])) <= R.SCORE_ABS_BAR, (k, got)


def test_three_frames_in_one_call():
    """Frames do not leak into each other and a frame's bits do not depend on its place: f0, the noise frame and the part
    of f2 that holds the constant block, in one call, against the one-frame calls."""
    fr = _frames()
    stack = np.stack([fr[0], fr[3], fr[2][:, 96:288]])
    sums, planes = _device(stack, True, 0)
    assert sums.shape == (3, 2, 4, 5, 5)
    for i in range(3):
        one, one_planes = _device(stack[i], True, 0)
        assert sums[i].tobytes() == one[0].tobytes(), i
        for a, b in zip(planes, one_planes):
            assert a[i].tobytes() == b[0].tobytes(), i
    _check_sums(sums[0], _case("f0_192x192")[3]["sums"], "nf=3, frame 0")
    _check_sums(sums[1], _case("f3_192x192_noise")[3]["sums"], "nf=3, frame 1")
    # the block of constant 255: the map is exactly zero except within three pixels of its textured neighbours, where
    # Y - mu > 0: no negative sample at either scale, which is what makes its row NaN
    assert np.all(sums[2, :, 0, 0, 0] == 0.0) and np.all(sums[2, :, 0, 0, 1] > 0.0) and np.all(sums[2, :, 0, 0, 1] < 96 * 12)
    _check_sums(sums[2], R.frame_stages(stack[2], _model().window, bgr=True)["sums"], "nf=3, frame 2")


def test_bgr_flag_and_determinism():
    frame = _frames()[1]
    as_bgr = _device(frame, True, 0, planes=False)
    as_rgb = _device(np.ascontiguousarray(frame[..., ::-1]), False, 0, planes=False)
    assert as_bgr.tobytes() == as_rgb.tobytes()
    assert _device(frame, False, 0, planes=False).tobytes() != as_bgr.tobytes()      # the flag is read
    assert _device(frame, True, 0, planes=False).tobytes() == as_bgr.tobytes()       # a second call: the same bytes
    a, pa = _device(frame, True, 0)
    assert a.tobytes() == as_bgr.tobytes() and all(np.isfinite(p).all() for p in pa)  # the planes do not change the sums


def test_rejected_arguments():
    from refid_amd import niqe
    from refid_amd._lib import RefidHipError, lib
    m = _model()
    for shape, cb in (((95, 200, 3), 0), ((200, 95, 3), 0), ((101, 300, 3), 3)):
        with pytest.raises(RefidHipError):
            niqe.moments(torch.zeros(shape, dtype=torch.uint8, device="cuda"), m, crop_border=cb)
    with pytest.raises(RefidHipError):
        niqe.moments(torch.zeros((96, 96, 3), dtype=torch.uint8), m)                 # a host tensor: no CPU path
    u8 = torch.zeros((96, 96, 3), dtype=torch.uint8, device="cuda")
    sums = torch.zeros(50, dtype=torch.float64, device="cuda")
    win = torch.from_numpy(m.window.reshape(-1).copy()).cuda()
    assert lib().refid_niqe_moments(u8.data_ptr(), 1, 95, 96, 0, 0, win.data_ptr(), sums.data_ptr(), None, None, None, None, None) != 0
    assert b"96x96" in lib().refid_last_error()
    assert lib().refid_niqe_moments(u8.data_ptr(), 1, 96, 96, 2, 0, win.data_ptr(), sums.data_ptr(), None, None, None, None, None) != 0
    torch.cuda.synchronize()
    assert float(sums.abs().sum()) == 0.0                                            # nothing was launched


# ---- the sequence runner and the command line -------------------------------------------------------------------------------
NET = dict(type="FinalBidirectionAttenfusion", img_chn=6, ev_chn=2, num_encoders=3, base_num_channels=8, num_block=1)
STAMPS = [10.0, 20.0, 30.0]


def _sequence(H, W, seed):
    """Three key frames cut from the 1/f fixture frame (so that the outputs are textured) and events over [10, 30)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    src = _frames()[1][..., ::-1]
    frames = np.stack([np.ascontiguousarray(src[o:o + H, o:o + W]) for o in (0, 4, 8)])
    n = 4000
    ev = np.stack([np.sort(rng.uniform(10.0, 30.0, n)), rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n)],
                  axis=1).astype(np.float32)
    return frames, np.ascontiguousarray(ev)


def _net():
    from refid_amd.archs import define_network
    net = define_network(deepcopy(NET)).to("cuda")
    net.load_state_dict(O.make_params(6, base_num_channels=8, mode="hash", seed=3))
    return net


@pytest.mark.parametrize("H,W,mb", [(96, 128, 2), (96, 192, 1)])
def test_interpolator_scores_its_frames(H, W, mb):
    """96x128 holds one block (every score is nan, by the reference's rule); 96x192 holds two, one pair per minibatch."""
    from refid_amd import niqe
    from refid_amd.sequence import SequenceInterpolator, make_pairs, sharp_windows
    frames, ev = _sequence(H, W, seed=5)
    pairs = make_pairs(ev[:, 0], *sharp_windows(STAMPS))
    assert len(pairs) == 2
    interp = SequenceInterpolator(_net(), 1, 1, "sharp", max_minibatch=mb)
    plain = interp.run(frames, ev, pairs, keep=True)
    assert interp.niqe_scores is None
    kept = interp.run(frames, ev, pairs, keep=True, niqe=_model(), names=["a", "b"])
    assert kept.shape == (2, 1, H, W, 3) and kept.tobytes() == plain.tobytes()
    want = niqe.calculate_niqe_frames(kept.reshape(-1, H, W, 3), _model())
    print(f"{H}x{W}: scores {want}")
    assert [(s[0], s[1]) for s in interp.niqe_scores] == [("a", 0), ("b", 0)]
    assert np.array_equal([s[2] for s in interp.niqe_scores], want, equal_nan=True)
    assert np.isnan(want).all() if W < 192 else np.isfinite(want).all()
    assert interp.run(frames, ev, pairs, niqe=_model()) is None and len(interp.niqe_scores) == 2   # the return value is keep's


def test_runner_rejects_small_frames():
    from refid_amd._lib import RefidHipError
    from refid_amd.sequence import SequenceInterpolator, make_pairs, sharp_windows
    frames, ev = _sequence(40, 128, seed=6)
    with pytest.raises(RefidHipError):
        SequenceInterpolator(_net(), 1, 1, "sharp").run(frames, ev, make_pairs(ev[:, 0], *sharp_windows(STAMPS)), niqe=_model())


def test_command_lines_write_niqe_txt(tmp_path, capsys):
    """--niqe on both front ends: niqe.txt holds one line per PNG plus the mean, and the printed mean is the file's."""
    from refid_amd import deblur, interpolate
    from refid_amd.png import write_png
    frames, ev = _sequence(96, 192, seed=7)
    for k in range(3):
        write_png(str(tmp_path / "frames" / f"{k:03d}.png"), frames[k])
    np.savez(tmp_path / "e.npz", x=ev[:, 1], y=ev[:, 2], timestamp=ev[:, 0], polarity=ev[:, 3])
    (tmp_path / "stamps.txt").write_text("".join(f"{s}\n" for s in STAMPS))
    (tmp_path / "exposures.txt").write_text("".join(f"{s} {s + 5.0}\n" for s in STAMPS))
    params = os.path.join(GOLDEN, "niqe_pris_params.npz")
    common = ["--frames", str(tmp_path / "frames"), "--events", str(tmp_path / "e.npz"), "--niqe", params]
    torch.manual_seed(11)                                                        # no checkpoint: the initial weights
    assert interpolate.main(common + ["--n", "1", "--layout", "sharp", "--stamps", str(tmp_path / "stamps.txt"),
                                      "--out", str(tmp_path / "i")]) == 0
    torch.manual_seed(11)
    assert deblur.main(common + ["--num-bins", "6", "--stamps", str(tmp_path / "exposures.txt"), "--out", str(tmp_path / "d")]) == 0
    printed = capsys.readouterr().out
    for out, pngs in (("i", ["000000_00.png", "000001_00.png"]), ("d", ["000000.png", "000001.png", "000002.png"])):
        assert sorted(os.listdir(tmp_path / out)) == sorted(pngs + ["niqe.txt"])
        lines = (tmp_path / out / "niqe.txt").read_text().splitlines()
        assert [ln.split()[0] for ln in lines] == pngs + ["mean"]
        scores = [float(ln.split()[1]) for ln in lines[:-1]]
        finite = [s for s in scores if np.isfinite(s)]
        assert finite and abs(float(lines[-1].split()[1]) - np.mean(finite)) < 1e-5
        assert f"NIQE mean {lines[-1].split()[1]} over {len(pngs)} frames" in printed
