"""MI355X: scoring uint8 frames against ground truth on the device -- refid_score_u8 (csrc/score.hip) against its numpy
restatement (tests/score_ref.py), against the existing 3-D SSIM kernel, ``refid_amd.score``'s front door and command line,
and the sequence runners' ``gt=`` / ``score=``.

The squared RGB error is an integer; the Y plane and the Y SSIM map are single correctly rounded operations in a fixed
order, so they are compared BIT for bit; the two float64 sums are fixed trees over at most 1e6 terms of one sign or of
magnitude at most 1, about 20 * 2^-53 relative from the exactly rounded sum: rtol 1e-13 against math.fsum.  The 3-D SSIM
sum is held to refid_ssim3d_u8's bits.  Shapes (h, w, crop_border, frames) from tests/golden/score.npz: (7, 9, 0, 1) every
tap clamped, (17, 16, 0, 1) a tile row of one line, (23, 37, 3, 1) every row segment misaligned and partial tiles both
ways, (40, 50, 4, 3) frame folding; three families each, identical frames, a flat frame against noise."""
import ctypes
import functools
import math
import os
from copy import deepcopy

import numpy as np
import pytest
import torch

import score_ref as R
from oracle import refid_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SUM_RTOL = 1e-13
ENTRY_NAMES = ["c0_noise", "c0_pm2", "c0_flip", "c1_noise", "c1_pm2", "c1_flip", "c2_noise", "c2_pm2", "c2_flip", "c3_noise",
               "c3_pm2", "c3_flip", "identical", "flat_vs_noise"]


@functools.lru_cache(maxsize=None)
def _golden():
    z = np.load(os.path.join(GOLDEN, "score.npz"))
    arrays = {k: z[k] for k in z.files}
    for v in arrays.values():
        v.setflags(write=False)
    return arrays, {e.split()[0]: (e.split()[1], e.split()[2], int(e.split()[3])) for e in z["entries"].tolist()}


def _entry(name):
    """(pred BGR (nf, h, w, 3), gt BGR, crop_border)"""
    arrays, entries = _golden()
    gk, pk, cb = entries[name]
    return arrays[pk], arrays[gk], cb


@functools.lru_cache(maxsize=None)
def _stages(name):
    """The restatement's stages per frame, computed once and frozen."""
    pred, gt, cb = _entry(name)
    out = []
    for p, g in zip(pred, gt):
        st = R.frame_stages(p, g, bgr=True, crop_border=cb)
        for v in st.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(st)
    return tuple(out)


def _device(pred, gt, bgr, cb, taps=True, **want):
    """ops.score_u8 -> (words int64 (4, nf) numpy, [ya, map] numpy or None)"""
    from refid_amd import ops
    a = torch.from_numpy(np.array(pred)).cuda()
    b = torch.from_numpy(np.array(gt)).cuda()
    want = dict(dict(sq_rgb=True, sq_y=True, ssim3d=True, ssim_y=True), **want)
    out = ops.score_u8(a, b, bgr, cb, taps=taps, **want)
    torch.cuda.synchronize()
    if not taps:
        return out.cpu().numpy(), None
    return out[0].cpu().numpy(), [None if t is None else t.cpu().numpy() for t in out[1]]


def _close(got, want, what):
    rel = abs(got - want) / abs(want) if want else abs(got)
    print(f"{what}: device {got!r}, exactly rounded sum {want!r}, relative deviation {rel:.3e}")
    assert abs(got - want) <= SUM_RTOL * abs(want), what


@pytest.mark.parametrize("name", ENTRY_NAMES)
def test_device_equals_the_restatement(name):
    from refid_amd import score
    pred, gt, cb = _entry(name)
    stages = _stages(name)
    words, (ya, ymap) = _device(pred, gt, True, cb)
    f64 = words.view(np.float64)
    hc, wc = stages[0]["hc"], stages[0]["wc"]
    assert ya.shape == ymap.shape == (len(stages), hc, wc) and ya.dtype == np.float32 and ymap.dtype == np.float64
    for f, st in enumerate(stages):
        assert int(words[0, f]) == st["sq_rgb"], (name, f)
        for got, key, bits in ((ya[f], "ya", np.int32), (ymap[f], "ssim_y_map", np.int64)):
            diff = got.view(bits) != st[key].view(bits)
            assert not diff.any(), f"{name}[{f}]: {key} differs in {int(diff.sum())} of {diff.size} elements, first at {np.argwhere(diff)[0]}"
        _close(float(f64[1, f]), math.fsum(st["sq_y_terms"].astype(np.float64).ravel().tolist()), f"{name}[{f}] sq_y")
        _close(float(f64[3, f]), math.fsum(st["ssim_y_map"].ravel().tolist()), f"{name}[{f}] ssim_y")
    # the other channel order: the same frames as RGB give the same bits
    rgb_words, (rgb_ya, rgb_map) = _device(pred[..., ::-1], gt[..., ::-1], False, cb)
    assert rgb_words.tobytes() == words.tobytes() and rgb_ya.tobytes() == ya.tobytes() and rgb_map.tobytes() == ymap.tobytes()
    # the front door against what the reference recorded, inside the bars of tests/test_score_ref_host.py
    ref = _golden()[0][f"ref_{name}"]
    sc = score.score_u8(pred, gt, bgr=True, crop_border=cb, psnr_y=True, ssim_y=True)
    for f in range(len(stages)):
        for got, want, bar in ((sc.psnr[f], ref[f, 0], 1e-9), (sc.psnr_y[f], ref[f, 1], 1e-4), (sc.ssim_y[f], ref[f, 2], 1e-12)):
            assert got == want if math.isinf(want) else abs(got - want) <= bar, (name, f, got, want)
    if name in ("identical", "c3_flip"):
        assert sc.psnr[0] == sc.psnr_y[0] == float("inf") and sc.ssim_y[0] == 1.0 and abs(sc.ssim[0] - 1.0) < 1e-6
    if name == "c2_flip":
        assert int(words[0, 0]) == 64 and f64[1, 0] > 0.0                   # one green value differs by 8


def test_the_bgr_flag_is_read():
    pred, gt, cb = _entry("c2_noise")
    a, _ = _device(pred, gt, True, cb, taps=False)
    b, _ = _device(pred, gt, False, cb, taps=False)
    assert a[0].tobytes() == b[0].tobytes()                                  # the RGB error does not care
    assert a[1].tobytes() != b[1].tobytes() and a[3].tobytes() != b[3].tobytes()


def test_same_bits_every_run_and_at_every_position():
    pred, gt, cb = _entry("c3_noise")
    words, (ya, ymap) = _device(pred, gt, True, cb)
    again, (ya2, ymap2) = _device(pred, gt, True, cb)
    assert words.tobytes() == again.tobytes() and ya.tobytes() == ya2.tobytes() and ymap.tobytes() == ymap2.tobytes()
    rev, (ya_r, ymap_r) = _device(pred[::-1], gt[::-1], True, cb)
    for f in range(3):
        one, (ya1, ymap1) = _device(pred[f:f + 1], gt[f:f + 1], True, cb)
        assert one[:, 0].tobytes() == words[:, f].tobytes() == rev[:, 2 - f].tobytes(), f
        assert ya1[0].tobytes() == ya[f].tobytes() == ya_r[2 - f].tobytes(), f
        assert ymap1[0].tobytes() == ymap[f].tobytes() == ymap_r[2 - f].tobytes(), f
    # a view that starts at an odd byte address: the aligned-word staging picks the same bytes
    flat = torch.zeros(pred.size + 1, dtype=torch.uint8, device="cuda")
    flat[1:] = torch.from_numpy(np.array(pred)).cuda().reshape(-1)
    from refid_amd import ops
    odd = ops.score_u8(flat[1:].view(pred.shape), torch.from_numpy(np.array(gt)).cuda(), True, cb, True, True, True, True)
    assert odd.cpu().numpy().tobytes() == words.tobytes()


def _planes(u8_bgr, cb):
    """cropped, contiguous float32 u8/255 planes (nf, 3, hc, wc) in R, G, B order"""
    c = u8_bgr[:, cb:u8_bgr.shape[1] - cb, cb:u8_bgr.shape[2] - cb, ::-1]
    return torch.from_numpy(np.ascontiguousarray(c.transpose(0, 3, 1, 2))).cuda().float() / 255.0


@pytest.mark.parametrize("name", ["c0_noise", "c1_pm2", "c2_noise", "c2_pm2", "c3_noise", "c3_flip", "flat_vs_noise"])
def test_ssim3d_is_the_existing_kernels(name):
    from refid_amd import metrics, score
    from refid_amd._lib import check, lib
    pred, gt, cb = _entry(name)
    words, _ = _device(pred, gt, True, cb, taps=False)
    a, b = _planes(pred, cb), _planes(gt, cb)
    nf, _, hc, wc = a.shape
    buf = torch.empty(nf + lib().refid_ssim3d_u8_parts(nf, hc, wc), dtype=torch.float64, device="cuda")
    check(lib().refid_ssim3d_u8(a.data_ptr(), b.data_ptr(), nf, hc, wc, buf.data_ptr(), buf[nf:].data_ptr(), None), "refid_ssim3d_u8")
    torch.cuda.synchronize()
    want = buf[:nf].cpu().numpy()
    got = words.view(np.float64)[2]
    print(f"{name}: ssim3d sums {got.tolist()} (existing kernel {want.tolist()})")
    assert got.tobytes() == want.tobytes()
    alone, _ = _device(pred, gt, True, cb, taps=False, sq_rgb=False, sq_y=False, ssim_y=False)
    assert alone[2].tobytes() == words[2].tobytes()
    # at crop_border 0 the front door gives metrics.val_tail's numbers for the same frames
    a0, b0 = _planes(pred, 0), _planes(gt, 0)
    tail = metrics.val_tail(a0, b0, bgr=True)
    assert np.array_equal(tail.pred_u8.cpu().numpy(), pred)
    sc = score.score_u8(pred, gt, bgr=True)
    assert sc.psnr == tail.psnr and sc.ssim == tail.ssim and sc.psnr_y is None and sc.ssim_y is None
    on_device = score.score_u8(tail.pred_u8, torch.from_numpy(np.array(gt)).cuda(), bgr=True)
    assert on_device == sc


def test_null_outputs_do_not_change_the_others():
    pred, gt, cb = _entry("c2_pm2")
    full, (ya, _) = _device(pred, gt, True, cb)
    keys = ("sq_rgb", "sq_y", "ssim3d", "ssim_y")
    for mask in (1, 2, 4, 8, 3, 5, 10, 12, 7, 14):
        want = {k: bool(mask >> i & 1) for i, k in enumerate(keys)}
        got, (ya_m, map_m) = _device(pred, gt, True, cb, **want)
        for i, k in enumerate(keys):
            if want[k]:
                assert got[i].tobytes() == full[i].tobytes(), (mask, k)
        assert ya_m.tobytes() == ya.tobytes() and (map_m is None) == (not want["ssim_y"])
    from refid_amd import score
    sc = score.score_u8(pred, gt, bgr=True, crop_border=cb, psnr=False, ssim=False, ssim_y=True)
    assert sc.psnr is None and sc.ssim is None and sc.psnr_y is None and len(sc.ssim_y) == 1


def test_refusals_launch_nothing():
    from refid_amd import ops, score
    from refid_amd._lib import RefidHipError, lib
    L = lib()
    u8 = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    other = torch.full((1, 8, 8, 3), 9, dtype=torch.uint8, device="cuda")
    out = torch.full((4 + 16,), -7, dtype=torch.int64, device="cuda")
    o = [ctypes.c_void_p(out[i:].data_ptr()) for i in range(4)]
    parts = ctypes.c_void_p(out[4:].data_ptr())
    a, b = ctypes.c_void_p(u8.data_ptr()), ctypes.c_void_p(other.data_ptr())
    for args, word in (((None, b, 1, 8, 8, 0, 0), b"NULL frames"), ((a, None, 1, 8, 8, 0, 0), b"NULL frames"),
                       ((a, b, 1, 8, 8, 0, -1), b"negative"), ((a, b, 1, 8, 8, 0, 4), b"leaves nothing"),
                       ((a, b, 1, 8, 9, 0, 4), b"leaves nothing"), ((a, b, 1, 8, 8, 4, 0), b"unknown flags"),
                       ((a, b, 100, 4000, 4000, 0, 0), b"31 bits"), ((a, b, 0, 8, 8, 0, 0), b"bad arguments")):
        assert L.refid_score_u8(*args, *o, parts, None, None, None) == 1, args
        assert word in L.refid_last_error(), (args, L.refid_last_error())
    torch.cuda.synchronize()
    assert bool((out == -7).all())                                           # nothing was launched
    assert L.refid_score_u8(a, b, 1, 8, 8, 0, 0, *o, parts, None, None, None) == 0   # the same buffers, accepted
    torch.cuda.synchronize()
    assert int(out[0]) == 8 * 8 * 3 * 81
    for bad in (dict(crop_border=4), dict(crop_border=-1)):
        with pytest.raises(RefidHipError):
            score.score_u8(u8, other, **bad)
    with pytest.raises(RefidHipError):
        ops.score_u8(u8, other[:, :7])                                       # shapes differ
    with pytest.raises(RefidHipError):
        ops.score_u8(u8.cpu(), other.cpu())                                  # host tensors: no CPU path below the front door
    with pytest.raises(RefidHipError):
        score.score_u8(u8.float(), other.float())


def test_frame_scorer_collects_calls_of_different_sizes():
    from refid_amd import score
    scorer = score.FrameScorer(bgr=True, crop_border=3, psnr_y=True, ssim_y=True, capacity=2)
    want = [[], [], [], []]
    for name in ("c2_noise", "c3_pm2", "c2_flip"):                           # 1 + 3 + 1 frames: the pinned block is renewed
        pred, gt, _ = _entry(name)
        scorer.add(torch.from_numpy(np.array(pred)).cuda(), torch.from_numpy(np.array(gt)).cuda())
        for dst, vals in zip(want, score.score_u8(pred, gt, bgr=True, crop_border=3, psnr_y=True, ssim_y=True)):
            dst.extend(vals)
    assert len(scorer) == 5
    assert scorer.finish() == score.Scores(*want)
    assert len(scorer) == 0


def _write_pairs(root, pred_name, gt_name, names_frames):
    from refid_amd.png import write_png
    for stem, (p, g) in names_frames.items():
        write_png(str(root / pred_name(stem)), np.ascontiguousarray(p[..., ::-1]))       # the PNGs hold RGB
        write_png(str(root / gt_name(stem)), np.ascontiguousarray(g[..., ::-1]))


def _parse(lines):
    assert lines[0].startswith("# file ")
    cols = lines[0].split()[2:]
    return cols, {ln.split()[0]: [float(v) for v in ln.split()[1:]] for ln in lines[1:]}


def test_command_line_end_to_end(tmp_path, capsys):
    """Two directories with frames of two sizes, --crop-border, --y and --out; then the X.png / X_gt.png siblings of one
    directory on stdout; every line is ``score_u8``'s value at the printed precision."""
    from refid_amd import score
    p3, g3, _ = _entry("c3_pm2")
    p2, g2, _ = _entry("c2_noise")
    frames = {"a_00": (p3[0], g3[0]), "a_01": (p3[1], g3[1]), "b_00": (p2[0], g2[0]), "c_00": (p3[2], g3[2])}
    _write_pairs(tmp_path, lambda s: f"pred/{s}.png", lambda s: f"gt/{s}.png", frames)
    assert score.main(["--pred", str(tmp_path / "pred"), "--gt", str(tmp_path / "gt"), "--crop-border", "3", "--y",
                       "--out", str(tmp_path / "report" / "scores.txt")]) == 0
    assert "4 frames: mean " in capsys.readouterr().out
    cols, rows = _parse((tmp_path / "report" / "scores.txt").read_text().splitlines())
    assert cols == ["psnr", "ssim", "psnr_y", "ssim_y"] and list(rows) == ["a_00.png", "a_01.png", "b_00.png", "c_00.png", "mean"]
    fmt = lambda v: float(f"{v:.6f}")                                        # noqa: E731
    per_col = [[], [], [], []]
    for stem, (p, g) in frames.items():
        sc = score.score_u8(p[None], g[None], bgr=True, crop_border=3, psnr_y=True, ssim_y=True)
        assert rows[stem + ".png"] == [fmt(c[0]) for c in sc], stem
        for dst, c in zip(per_col, sc):
            dst.append(c[0])
    assert rows["mean"] == [fmt(sum(c) / 4) for c in per_col]
    _write_pairs(tmp_path, lambda s: f"val/{s}.png", lambda s: f"val/{s}_gt.png", frames)
    assert score.main(["--pred", str(tmp_path / "val"), "--gt-suffix", "_gt"]) == 0
    cols, rows = _parse(capsys.readouterr().out.splitlines())
    assert cols == ["psnr", "ssim"] and list(rows) == ["a_00.png", "a_01.png", "b_00.png", "c_00.png", "mean"]
    for stem, (p, g) in frames.items():
        sc = score.score_u8(p[None], g[None], bgr=True)
        assert rows[stem + ".png"] == [fmt(sc.psnr[0]), fmt(sc.ssim[0])], stem


def test_command_line_with_niqe(tmp_path, capsys):
    from refid_amd import niqe, score
    rng = np.random.Generator(np.random.PCG64(9))
    pred = rng.integers(0, 256, (96, 192, 3), dtype=np.uint8)
    gt = np.clip(pred.astype(int) + rng.integers(-3, 4, pred.shape), 0, 255).astype(np.uint8)
    _write_pairs(tmp_path, lambda s: f"p/{s}.png", lambda s: f"g/{s}.png", {"x": (pred[..., ::-1], gt[..., ::-1])})
    params = os.path.join(GOLDEN, "niqe_pris_params.npz")
    assert score.main(["--pred", str(tmp_path / "p"), "--gt", str(tmp_path / "g"), "--niqe", params]) == 0
    cols, rows = _parse(capsys.readouterr().out.splitlines())
    assert cols == ["psnr", "ssim", "niqe"]
    want = niqe.calculate_niqe_frames(pred, niqe.NiqeModel.load(params))[0]
    assert math.isfinite(want) and rows["x.png"][2] == float(f"{want:.6f}") == rows["mean"][2]


# ---- the sequence runner and the command lines -----------------------------------------------------------------------------
NET = dict(type="FinalBidirectionAttenfusion", img_chn=6, ev_chn=2, num_encoders=3, base_num_channels=8, num_block=1)
STAMPS = [10.0, 20.0, 30.0]


def _sequence(H, W, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    frames = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    n = 2000
    ev = np.stack([np.sort(rng.uniform(10.0, 30.0, n)), rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n)],
                  axis=1).astype(np.float32)
    return frames, np.ascontiguousarray(ev)


def _net():
    from refid_amd.archs import define_network
    net = define_network(deepcopy(NET)).to("cuda")
    net.load_state_dict(O.make_params(6, base_num_channels=8, mode="hash", seed=3))
    return net


def test_interpolator_scores_its_frames(tmp_path):
    from refid_amd import score
    from refid_amd._lib import RefidHipError
    from refid_amd.png import write_png
    from refid_amd.sequence import SequenceInterpolator, make_pairs, sharp_windows
    H, W = 37, 50
    frames, ev = _sequence(H, W, seed=5)
    pairs = make_pairs(ev[:, 0], *sharp_windows(STAMPS))
    interp = SequenceInterpolator(_net(), 1, 3, "sharp", max_minibatch=1)
    plain = interp.run(frames, ev, pairs, keep=True, names=["a", "b"])
    assert interp.scores is None and plain.shape == (2, 3, H, W, 3)
    rng = np.random.Generator(np.random.PCG64(8))
    gt = np.clip(plain.reshape(-1, H, W, 3).astype(int) + rng.integers(-4, 5, (6, H, W, 3)), 0, 255).astype(np.uint8)
    # ground truth as frames: the default scorer
    kept = interp.run(frames, ev, pairs, keep=True, names=["a", "b"], gt=gt)
    assert kept.tobytes() == plain.tobytes()
    want = score.score_u8(plain.reshape(-1, H, W, 3), gt)
    assert [(s[0], s[1]) for s in interp.scores] == [(n, f) for n in ("a", "b") for f in range(3)]
    assert [s[2].psnr for s in interp.scores] == want.psnr and [s[2].ssim for s in interp.scores] == want.ssim
    assert all(s[2].psnr_y is None and s[2].ssim_y is None for s in interp.scores)
    # ground truth as a directory of the outputs' names, a scorer with a crop and the Y scores
    for i, (name, f) in enumerate((n, f) for n in ("a", "b") for f in range(3)):
        write_png(str(tmp_path / "gt" / f"{name}_{f:02d}.png"), gt[i])
    scorer = score.FrameScorer(crop_border=2, psnr=False, ssim=False, psnr_y=True, ssim_y=True)
    assert interp.run(frames, ev, pairs, names=["a", "b"], gt=str(tmp_path / "gt"), score=scorer) is None
    want = score.score_u8(plain.reshape(-1, H, W, 3), gt, crop_border=2, psnr=False, ssim=False, psnr_y=True, ssim_y=True)
    assert [s[2].psnr_y for s in interp.scores] == want.psnr_y and [s[2].ssim_y for s in interp.scores] == want.ssim_y
    assert all(s[2].psnr is None for s in interp.scores)
    os.remove(tmp_path / "gt" / "b_02.png")
    with pytest.raises(RefidHipError, match=r"no ground truth .*b_02\.png"):
        interp.run(frames, ev, pairs, names=["a", "b"], gt=str(tmp_path / "gt"))
    with pytest.raises(RefidHipError, match="gt holds 3 frames"):
        interp.run(frames, ev, pairs, names=["a", "b"], gt=gt[:3])
    with pytest.raises(RefidHipError, match="needs gt"):
        interp.run(frames, ev, pairs, score=score.FrameScorer())
    assert interp.run(frames, ev, pairs, keep=True).tobytes() == plain.tobytes() and interp.scores is None


def test_command_lines_write_scores_txt(tmp_path, capsys):
    """--gt on both front ends: scores.txt holds one line per PNG plus the mean, equal to scoring the written PNGs."""
    from refid_amd import deblur, interpolate, score
    from refid_amd.png import read_png, write_png
    frames, ev = _sequence(40, 48, seed=7)
    for k in range(3):
        write_png(str(tmp_path / "frames" / f"{k:03d}.png"), frames[k])
    np.savez(tmp_path / "e.npz", x=ev[:, 1], y=ev[:, 2], timestamp=ev[:, 0], polarity=ev[:, 3])
    (tmp_path / "stamps.txt").write_text("".join(f"{s}\n" for s in STAMPS))
    (tmp_path / "exposures.txt").write_text("".join(f"{s} {s + 5.0}\n" for s in STAMPS))
    rng = np.random.Generator(np.random.PCG64(10))
    runs = (("i", interpolate, ["--n", "1", "--layout", "sharp", "--stamps", str(tmp_path / "stamps.txt")],
             ["000000_00.png", "000001_00.png"]),
            ("d", deblur, ["--num-bins", "6", "--stamps", str(tmp_path / "exposures.txt")], ["000000.png", "000001.png", "000002.png"]))
    for out, mod, extra, pngs in runs:
        gts = {}
        for name in pngs:
            gts[name] = rng.integers(0, 256, (40, 48, 3), dtype=np.uint8)
            write_png(str(tmp_path / f"gt_{out}" / name), gts[name])
        torch.manual_seed(11)                                                # no checkpoint: the initial weights
        assert mod.main(["--frames", str(tmp_path / "frames"), "--events", str(tmp_path / "e.npz"), "--gt", str(tmp_path / f"gt_{out}"),
                         "--out", str(tmp_path / out)] + extra) == 0
        assert sorted(os.listdir(tmp_path / out)) == sorted(pngs + ["scores.txt"])
        cols, rows = _parse((tmp_path / out / "scores.txt").read_text().splitlines())
        assert cols == ["psnr", "ssim"] and list(rows) == pngs + ["mean"]
        for name in pngs:
            sc = score.score_u8(read_png(str(tmp_path / out / name))[None], gts[name][None])
            assert rows[name] == [float(f"{sc.psnr[0]:.6f}"), float(f"{sc.ssim[0]:.6f}")], (out, name)
        assert f"over {len(pngs)} frames" in capsys.readouterr().out
