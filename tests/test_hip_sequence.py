"""MI355X: the test-time entry -- refid_amd.sequence.SequenceAssembler (csrc/sequence.hip) against its numpy restatement
(tests/sequence_ref.py) and against DeviceBatchAssembler, bit for bit; the rejected arguments of refid_seq_assemble;
SequenceInterpolator on a tiny network; the sharp / test model family behind create_model.

Everything the kernels compute is integer arithmetic or a single correctly rounded fp32 operation, so the assembly
comparisons are BIT-identical.  Shapes are the smallest at which one thing can still go wrong: 40x56 (no padding, 2240
elements: several blocks of four-element lanes), 37x50 -> 40x56 (padding on both sides, frame rows that are no multiple
of four), 24x32 / 21x27 -> 24x32 for the blur layout with overlapping windows; 21x27 and 37x50 once more with multiple=1
(rows that are no multiple of four: the one-element kernels of both pair layouts)."""
import functools
import logging
import os
from copy import deepcopy

import numpy as np
import pytest
import torch

import sequence_ref as S
from oracle import refid_oracle as O

pytestmark = pytest.mark.gpu

STAMPS = [10.0, 20.0, 30.0, 31.0, 40.0]                   # five key frames
CASES = {                                                 # name: (layout, m, n, H, W, bgr, multiple)
    "sharp_40x56": ("sharp", 1, 3, 40, 56, True, 8),
    "sharp_37x50_bgr": ("sharp", 1, 3, 37, 50, True, 8),
    "sharp_37x50_rgb": ("sharp", 1, 3, 37, 50, False, 8),
    "blur_24x32": ("blur", 2, 1, 24, 32, False, 8),
    "blur_21x27": ("blur", 2, 1, 21, 27, True, 8),
    # multiple=1: no padding and rows that are no multiple of four -> the one-element kernels (seq_finish_kernel<1>,
    # seq_frames_kernel<1>) of both pair layouts, BGR and RGB, with lq's event channels (m = 2)
    "blur_21x27_x1": ("blur", 2, 1, 21, 27, True, 1),
    "sharp_37x50_rgb_x1": ("sharp", 1, 3, 37, 50, False, 1),
}


def _sequence(H, W, seed):
    """5 key frames and ~3000 events [t, x, y, p], sorted by time: coordinates at -1, 0, W-1, W and fractional, polarity in
    {-1, 0, 1}, runs of equal stamps exactly on the window bounds 10 and 20, ONE event in [30, 31), none in [31, 40), a few
    after the last key frame."""
    rng = np.random.Generator(np.random.PCG64(seed))
    frames = rng.integers(0, 256, (5, H, W, 3), dtype=np.uint8)
    n = 1480
    t = np.concatenate([rng.uniform(10.0, 20.0, n), rng.uniform(20.0, 30.0, n), rng.uniform(40.0, 44.0, 20)])
    x = np.where(rng.random(t.size) < 0.5, rng.integers(-1, W + 1, t.size), rng.uniform(-1.5, W + 0.5, t.size))
    y = np.where(rng.random(t.size) < 0.5, rng.integers(-1, H + 1, t.size), rng.uniform(-1.5, H + 0.5, t.size))
    p = rng.integers(-1, 2, t.size)
    ev = np.stack([t, x, y, p], axis=1)
    edge = [(10.0, 0, 0, 1), (10.0, W - 1, H - 1, -1), (10.0, -1, 3, 1),                  # a run on the first bound
            (20.0, W, 3, 1), (20.0, 3, H, 1), (20.0, W - 1, 0, 0), (20.0, 0, H - 1, 1), (20.0, -0.5, -0.5, 1),
            (20.0, W - 0.5, H - 0.5, -1),                                                   # a run on a shared bound
            (30.5, 5, 4, 1),                                                                # the single event of [30, 31)
            (15.0, 7, 7, 1), (15.0, 7, 7, 1), (15.0, 7, 7, 0)]                              # one pixel, +1 +1 -1
    ev = np.concatenate([ev, np.array(edge, dtype=np.float64)]).astype(np.float32)
    ev = ev[np.argsort(ev[:, 0], kind="stable")]
    return frames, np.ascontiguousarray(ev)


def _pairs(ev, layout, stamps):
    """The helper's pairs for the layout, then: an empty window, a window holding one event (first == last, dT -> 1), and
    two more pairs over the rows of pair 0 (windows that all cover the same rows) with other key frames."""
    from refid_amd.sequence import exposure_windows, make_pairs, sharp_windows
    t = ev[:, 0]
    if layout == "sharp":
        l, r, b, e = sharp_windows(STAMPS)                                          # [10,20) [20,30) [30,31) [31,40)
    else:
        l, r, b, e = exposure_windows(STAMPS, [s + 4.0 for s in STAMPS])            # [10,24) [20,34) [30,35) [31,44): overlap
    l, r = np.concatenate([l, [2, 0, 4, 3]]), np.concatenate([r, [3, 0, 0, 3]])
    b = np.concatenate([b, [35.0, 30.25, b[0], b[0]]])
    e = np.concatenate([e, [36.0, 30.75, e[0], e[0]]])
    return make_pairs(t, l, r, b, e, stamps=stamps)


@functools.lru_cache(maxsize=None)
def _case(name, stamps):
    layout, m, n, H, W, bgr, multiple = CASES[name]
    frames, ev = _sequence(H, W, seed=len(name) + H)
    pairs = _pairs(ev, layout, stamps)
    rows = [(p.row0, p.row1) for p in pairs]
    assert any(r1 == r0 for r0, r1 in rows) and any(r1 - r0 == 1 for r0, r1 in rows)     # an empty and a one-event window
    lq, voxel = S.assemble_pairs(frames, ev, pairs, m, n, layout, multiple=multiple, bgr=bgr)
    lq.setflags(write=False)
    voxel.setflags(write=False)
    return dict(frames=frames, events=ev, pairs=pairs, lq=lq, voxel=voxel, layout=layout, m=m, n=n, bgr=bgr, multiple=multiple)


def _same_bits(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (what, int(bad.sum()), "elements differ; first at", np.argwhere(bad)[0].tolist(),
                           float(got[bad][0]), float(want[bad][0]))


def _assembler(c):
    from refid_amd.sequence import SequenceAssembler
    return SequenceAssembler(c["m"], c["n"], c["layout"], multiple=c["multiple"]).load(c["frames"], c["events"], bgr=c["bgr"])


@pytest.mark.parametrize("stamps", ["events", "bounds"])
@pytest.mark.parametrize("name", list(CASES))
def test_assembly_equals_the_restatement_bit_for_bit(name, stamps):
    c = _case(name, stamps)
    asm = _assembler(c)
    out = asm.assemble(c["pairs"])
    assert sorted(out) == ["lq", "voxel"]
    _same_bits(out["lq"], c["lq"], f"{name} {stamps}: lq")
    _same_bits(out["voxel"], c["voxel"], f"{name} {stamps}: voxel")
    assert out["voxel"].abs().max().item() > 1                                   # events did land
    # a second call with fewer pairs (another cached geometry) reproduces the rows of the first
    part = asm.assemble(c["pairs"][1:4])
    assert torch.equal(part["lq"], out["lq"][1:4]) and torch.equal(part["voxel"], out["voxel"][1:4])


def test_padding_and_colour_order():
    """37x50 -> 40x56: zero voxels and replicated image rows / columns in the padding; the BGR and the RGB upload of the
    same frames differ exactly by the channel swap."""
    a, b = _case("sharp_37x50_bgr", "events"), _case("sharp_37x50_rgb", "events")
    assert np.array_equal(a["frames"], b["frames"])
    lq_a, lq_b = _assembler(a).assemble(a["pairs"])["lq"], _assembler(b).assemble(b["pairs"])["lq"]
    assert tuple(lq_a.shape) == (len(a["pairs"]), 2, 3, 40, 56)
    assert torch.equal(lq_a, lq_b.flip(2)) and not torch.equal(lq_a, lq_b)
    assert torch.equal(lq_a[..., 37:, :], lq_a[..., 36:37, :].expand(-1, -1, -1, 3, -1))
    assert torch.equal(lq_a[..., :, 50:], lq_a[..., :, 49:50].expand(-1, -1, -1, -1, 6))
    vox = _assembler(a).assemble(a["pairs"])["voxel"]
    assert vox[..., 37:, :].abs().max().item() == 0 and vox[..., :, 50:].abs().max().item() == 0


@pytest.mark.parametrize("name", ["sharp_37x50_rgb", "blur_21x27"])
def test_a_stream_without_events(name):
    from refid_amd.sequence import SequenceAssembler, make_pairs
    c = _case(name, "events")
    empty = np.zeros((0, 4), dtype=np.float32)
    pairs = make_pairs(empty[:, 0], [0, 3], [1, 4], [10.0, 30.0], [20.0, 40.0])
    assert [tuple(p)[2:] for p in pairs] == [(0, 0, 0.0, 0.0)] * 2
    asm = SequenceAssembler(c["m"], c["n"], c["layout"], multiple=8).load(c["frames"], empty, bgr=c["bgr"])
    out = asm.assemble(pairs)
    lq, voxel = S.assemble_pairs(c["frames"], empty, pairs, c["m"], c["n"], c["layout"], multiple=8, bgr=c["bgr"])
    _same_bits(out["lq"], lq, name + " E=0: lq")
    _same_bits(out["voxel"], voxel, name + " E=0: voxel")
    assert out["voxel"].abs().max().item() == 0


@pytest.mark.parametrize("stamps", ["events", "bounds"])
def test_agreement_with_the_batch_assembler(stamps):
    """Case 1 through DeviceBatchAssembler(1, 3, 'sharp', gt_size=None): per-pair event slices, the same stamps, dummy
    ground-truth frames.  Both paths are integer arithmetic with one rounding each: no tolerance."""
    from refid_amd.data import DeviceBatchAssembler
    c = _case("sharp_40x56", stamps)
    out = _assembler(c).assemble(c["pairs"])
    frames, ev = torch.from_numpy(c["frames"]), torch.from_numpy(c["events"])
    dummy = torch.zeros((3,) + tuple(frames.shape[1:]), dtype=torch.uint8)
    raw = [dict(frames=torch.cat([frames[[p.left, p.right]], dummy]), events=ev[p.row0:p.row1].contiguous(),
                first_stamp=p.first_stamp, last_stamp=p.last_stamp) for p in c["pairs"]]
    ref = DeviceBatchAssembler(1, 3, "sharp", gt_size=None)(raw)
    assert torch.equal(out["lq"].view(torch.int32), ref["lq"].view(torch.int32))
    assert torch.equal(out["voxel"].view(torch.int32), ref["voxel"].view(torch.int32))


def test_rejected_arguments_name_the_field_and_launch_nothing():
    from refid_amd import ops
    from refid_amd._lib import RefidHipError
    c = _case("sharp_37x50_rgb", "events")
    asm = _assembler(c)
    out = asm.assemble(c["pairs"])
    desc, table = asm._last
    n_events = len(c["events"])
    out["lq"].fill_(7.0)
    out["voxel"].fill_(7.0)

    def rejected(obj, field, value, match):
        saved = getattr(obj, field)
        setattr(obj, field, value)
        try:
            with pytest.raises(RefidHipError, match=match):
                ops.seq_assemble(desc)
        finally:
            setattr(obj, field, saved)

    rejected(table[0], "left", 5, r"pair 0: left 5")
    rejected(table[1], "left", -1, r"pair 1: left -1")
    rejected(table[2], "right", 5, r"pair 2: right 5")
    rejected(table[3], "right", -2, r"pair 3: right -2")
    rejected(table[0], "row0", table[0].row1 + 1, r"pair 0: row0 \d+ > row1")
    rejected(table[1], "row1", n_events + 1, rf"pair 1: row1 {n_events + 1} > n_events {n_events}")
    rejected(desc, "out_h", 36, r"out_h 36 < height 37")
    rejected(desc, "out_w", 48, r"out_w 48 < width 50")
    rejected(desc, "m", 2, r"sharp layout needs m == 1")
    rejected(desc, "n", 2, r"num_bins == 3")
    rejected(desc, "layout", 7, r"unknown layout 7")
    rejected(desc, "lq", None, r"null outputs")
    rejected(desc, "voxel", None, r"null outputs")
    rejected(desc, "n_pairs", 0, r"n_pairs 0")
    rejected(desc, "scratch", None, r"null scratch")
    rejected(desc, "pairs_dev", None, r"both pair tables")
    rejected(desc, "events", desc.events + 4, r"16-byte aligned")
    rejected(desc, "n_frames", 0, r"no frames \(n_frames 0")
    rejected(desc, "row_pitch", desc.row_pitch - 1, r"row_pitch 149 / frame_stride")
    rejected(table[2], "row0", -1, r"pair 2: row0 -1 > row1")
    torch.cuda.synchronize()
    assert bool((out["lq"] == 7.0).all()) and bool((out["voxel"] == 7.0).all())         # nothing was launched
    ops.seq_assemble(desc)                                                             # the untouched descriptor still runs
    _same_bits(out["lq"], c["lq"], "after the rejections: lq")
    _same_bits(out["voxel"], c["voxel"], "after the rejections: voxel")


# ---- SequenceInterpolator ---------------------------------------------------------------------------------------------------
NET = dict(type="FinalBidirectionAttenfusion", img_chn=6, ev_chn=2, num_encoders=3, base_num_channels=8, num_block=1)


def _net():
    from refid_amd.archs import define_network
    net = define_network(deepcopy(NET)).to("cuda")
    net.load_state_dict(O.make_params(6, base_num_channels=8, mode="hash", seed=3))
    return net


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_interpolator_frames_files_and_repeatability(tmp_path):
    from refid_amd.metrics import val_tail
    from refid_amd.png import read_png
    from refid_amd.sequence import SequenceInterpolator
    c = _case("sharp_37x50_rgb", "events")
    pairs = c["pairs"][:4]
    net = _net()
    # what the contract says: the same minibatch slices of the assembled inputs through the network and the tail
    batch = _assembler(c).assemble(pairs)
    net.eval()
    want = []
    with torch.no_grad():
        for i, j in ((0, 2), (2, 4)):
            out = net(x=batch["lq"][i:j], event=batch["voxel"][i:j])
            assert tuple(out.shape) == (2, 3, 3, 40, 56)
            want.append(val_tail(out[..., :37, :50], bgr=False).pred_u8)
    want = torch.cat(want).cpu().numpy()
    assert want.shape == (4, 3, 37, 50, 3) and len(np.unique(want)) > 20
    net.train()
    interp = SequenceInterpolator(net, 1, 3, "sharp", max_minibatch=2)
    assert interp.assembler.multiple == 8
    got = interp.run(c["frames"], c["events"], pairs, out_dir=str(tmp_path / "a"), keep=True)
    assert net.training is True                                                  # restored
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    names = [f"{k:06d}_{f:02d}.png" for k in range(4) for f in range(3)]          # the left key frame's index
    assert _files(tmp_path / "a") == names
    for k in range(4):
        for f in range(3):
            assert np.array_equal(read_png(str(tmp_path / "a" / f"{k:06d}_{f:02d}.png")), got[k, f]), (k, f)
    net.eval()
    again = interp.run(c["frames"], c["events"], pairs, out_dir=str(tmp_path / "b"), names=list("wxyz"), keep=True)
    assert net.training is False and np.array_equal(again, got)                   # a second run: the same bits
    assert _files(tmp_path / "b") == [f"{s}_{f:02d}.png" for s in "wxyz" for f in range(3)]
    before = _files(tmp_path)
    assert interp.run(c["frames"], c["events"], pairs[:3]) is None and _files(tmp_path) == before   # nothing asked for
    three = interp.run(c["frames"], c["events"], pairs[:3], keep=True)
    assert np.array_equal(three[:2], got[:2]) and three.shape == (3, 3, 37, 50, 3)


def test_command_line_front(tmp_path):
    """python -m refid_amd.interpolate, called in process: PNG key frames, two event files, a stamps file and a test YAML
    give the files SequenceInterpolator gives for the same sequence."""
    from refid_amd import interpolate
    from refid_amd.png import read_png, write_png
    from refid_amd.sequence import SequenceInterpolator, make_pairs, sharp_windows
    from test_sequence_host import TEST_YAML
    c = _case("sharp_37x50_rgb", "events")
    frames, ev = c["frames"], c["events"]
    for k in range(5):
        write_png(str(tmp_path / "frames" / f"{k:03d}.png"), frames[k])
    half = len(ev) // 2
    for name, part in (("e0.npz", ev[:half]), ("e1.npz", ev[half:])):
        np.savez(tmp_path / name, x=part[:, 1], y=part[:, 2], timestamp=part[:, 0], polarity=part[:, 3])
    (tmp_path / "stamps.txt").write_text("".join(f"{s}\n" for s in STAMPS))
    (tmp_path / "t.yml").write_text(TEST_YAML.replace("num_inter_interpolation: 7", "num_inter_interpolation: 3"))
    torch.manual_seed(11)                                                        # no checkpoint: the initial weights
    assert interpolate.main(["--opt", str(tmp_path / "t.yml"), "--frames", str(tmp_path / "frames"), "--events",
                             str(tmp_path / "e0.npz"), str(tmp_path / "e1.npz"), "--stamps", str(tmp_path / "stamps.txt"),
                             "--out", str(tmp_path / "out")]) == 0
    from refid_amd.archs import define_network
    torch.manual_seed(11)
    net = define_network(deepcopy(dict(NET, base_num_channels=8))).to("cuda")
    pairs = make_pairs(ev[:, 0], *sharp_windows(STAMPS))
    want = SequenceInterpolator(net, 1, 3, "sharp", max_minibatch=2).run(frames, ev, pairs, keep=True)
    assert _files(tmp_path / "out") == [f"{k:06d}_{f:02d}.png" for k in range(4) for f in range(3)]
    for k in range(4):
        for f in range(3):
            assert np.array_equal(read_png(str(tmp_path / "out" / f"{k:06d}_{f:02d}.png")), want[k, f]), (k, f)


# ---- the model family -------------------------------------------------------------------------------------------------------
H, W = 24, 40
PSNR, SSIM = dict(type="calculate_psnr", crop_border=0, test_y_channel=False), dict(type="calculate_ssim", crop_border=0,
                                                                                  test_y_channel=False)


def _opt(vis, model_type, dataset_key, m, n, **val):
    """Shaped like a shipped test YAML after options.parse: datasets.<key>, is_train False, no train block."""
    return {"name": "tinytest", "model_type": model_type, "is_train": False, "num_gpu": 1, "dist": False,
            "network_g": deepcopy(NET),
            "path": {"pretrain_network_g": None, "visualization": str(vis)},
            "datasets": {dataset_key: {"num_end_interpolation": m, "num_inter_interpolation": n}},
            "val": dict({"save_img": True, "save_gt": True, "metrics_interpo": dict(psnr=deepcopy(PSNR), ssim=deepcopy(SSIM))},
                        **val)}


def _loader(t):
    items = []
    for k, (seq, idx) in enumerate([("seqA", "000004"), ("seqA", "000011"), ("seqB", "000002")]):
        x, ev, gt = O.make_inputs(1, t, H, W, 6, seed=40 + k)
        items.append({"lq": x, "voxel": ev, "gt": gt, "seq": [seq], "origin_index": [idx]})
    return items


class _Tb:
    def __init__(self):
        self.calls = []

    def add_scalar(self, *a):
        self.calls.append(a)


def test_sharp_test_model_from_create_model(tmp_path, caplog):
    from refid_amd import train as T
    from refid_amd.metrics import calculate_psnr_frames, calculate_ssim_frames
    from refid_amd.png import read_png
    # metrics_deblur is ignored by the sharp classes, as in the reference: not even its options are looked at
    opt = _opt(tmp_path, "Test_TwoSharpImageEventRecurrentRestorationModel", "test", 1, 3,
               metrics_deblur=dict(psnr=dict(type="calculate_psnr", crop_border=4)))
    with caplog.at_level(logging.INFO, logger="basicsr"):
        model = T.create_model(opt)
    assert type(model) is T.Test_TwoSharpImageEventRecurrentRestorationModel
    assert [r.getMessage() for r in caplog.records] == ["Model [Test_TwoSharpImageEventRecurrentRestorationModel] is created."]
    caplog.clear()
    model.net_g.load_state_dict(O.make_params(6, base_num_channels=8, mode="hash", seed=3))
    ps, ss, outs = [], [], []
    for data in _loader(3):
        model.feed_data(data)
        model.test()
        outs.append(model.output.clone())
        ps += calculate_psnr_frames(model.output, model.gt)
        ss += calculate_ssim_frames(model.output, model.gt)
    assert len(ps) == len(ss) == 9
    want = dict(psnr=sum(ps) / 9, ssim=sum(ss) / 9)                               # the mean over ALL frames: cnt * T = 9
    tb = _Tb()
    with caplog.at_level(logging.INFO, logger="basicsr"):
        ret = model.validation(_loader(3), 5, tb, save_img=True)
    got = model.metric_results_interpo
    print(got, want)
    assert list(got) == ["psnr", "ssim"]
    assert abs(got["psnr"] - want["psnr"]) <= 1e-12 * abs(want["psnr"]) and abs(got["ssim"] - want["ssim"]) <= 2e-5
    assert ret == got["ssim"]                                                     # the last interpolation metric
    assert not hasattr(model, "metric_results_deblur") and not hasattr(model, "metric_results_total")
    lines = [r.getMessage() for r in caplog.records if r.name == "basicsr"]
    assert lines == ["Validation tinytest [interpolation],\t" + "".join(f"\t # {k}: {v:.4f}" for k, v in got.items())]
    assert tb.calls == [("metrics/psnr", got["psnr"], 5), ("metrics/ssim", got["ssim"], 5)]
    files = {}
    for data, out in zip(_loader(3), outs):
        for f in range(3):
            stem = os.path.join("tinytest", data["seq"][0], f"{data['origin_index'][0]}_{f:02d}")
            files[stem + ".png"] = O.tensor2img_u8(out[0, f]).permute(1, 2, 0).cpu().numpy()
            files[stem + "_gt.png"] = O.tensor2img_u8(data["gt"][0, f]).permute(1, 2, 0).cpu().numpy()
    assert _files(tmp_path) == sorted(files) and len(files) == 18
    for rel, img in files.items():
        assert np.array_equal(read_png(os.path.join(tmp_path, rel)), img), rel
    # seq and origin_index are required by the sharp classes' feed_data
    data = _loader(3)[0]
    del data["origin_index"]
    with pytest.raises(KeyError, match="origin_index"):
        model.feed_data(data)
    # the spelling of the GoPro 7- and 15-skip YAMLs resolves to the same class; a Test class never builds the training
    # settings (there is no train block here)
    other = T.create_model(dict(_opt(tmp_path, "TestTwoSharpImageEventRecurrentRestorationModel", "test", 1, 3), is_train=True))
    assert type(other) is type(model) and not hasattr(other, "exp_avg")


def test_blur_test_model_reads_datasets_test(tmp_path, caplog):
    """TestTwoImageEventRecurrentRestorationModel under datasets.test logs the three lines the existing class logs under
    datasets.val, with the same numbers."""
    from refid_amd import train as T
    deblur = dict(metrics_deblur=dict(psnr=deepcopy(PSNR), ssim=deepcopy(SSIM)), save_img=False)
    results = {}
    for model_type, key in (("TwoImageEventRecurrentRestorationModel", "val"),
                            ("TestTwoImageEventRecurrentRestorationModel", "test")):
        model = T.create_model(_opt(tmp_path, model_type, key, 1, 3, **deblur))
        model.net_g.load_state_dict(O.make_params(6, base_num_channels=8, mode="hash", seed=3))
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="basicsr"):
            ret = model.validation(_loader(5), 1, None, save_img=False)
        lines = [r.getMessage() for r in caplog.records if r.name == "basicsr"]
        results[key] = (ret, lines, model.metric_results_deblur, model.metric_results_interpo, model.metric_results_total)
    assert results["test"] == results["val"]
    lines = results["test"][1]
    assert [l.split(",")[0] for l in lines] == ["Validation tinytest [total]", "Validation tinytest [deblur]",
                                                "Validation tinytest [interpolation]"]
    assert _files(tmp_path) == []
    with pytest.raises(KeyError, match="val"):                                    # the existing class under a test YAML
        T.create_model(_opt(tmp_path, "TwoImageEventRecurrentRestorationModel", "test", 1, 3)).validation(_loader(5), 1, None)
