"""MI355X: deblurring whole sequences -- SequenceAssembler(layout='single') (csrc/sequence.hip: refid_seq_assemble_single)
against its numpy restatement (tests/sequence_single_ref.py, compared with the reference's __getitem__ by
test_sequence_single_host.py) and against DeviceBatchAssembler(layout='single'), bit for bit; the rejected arguments;
SequenceDeblurrer and python -m refid_amd.deblur on a tiny network; tiled inference (val.grids) for the 4-D network.

Everything the assembly computes is integer arithmetic, a float64 sum in a fixed order or a single correctly rounded
operation, so those comparisons are BIT-identical.  Shapes: the fixture's 26x38 frames with 6 bins are 5928 elements per
item -- one full 4096-element chunk of the statistics plus a tail -- padded to 28x40 (four-element stores, padding on both
sides) or kept at 26x38 (out_w % 4 != 0: the scalar stores); 2 bins are 1976 elements, one partial chunk; 24x32 x 6 = 4608,
two chunks without padding.  Tiling: 40x56 with crop 24 is 2x3 tiles whose overlap counts are 1, 2 and 4 -- dividing by a
power of two is exact, so the overlap average is compared bit for bit as well."""
import functools
import os
from copy import deepcopy

import numpy as np
import pytest
import torch

import sequence_single_ref as R
from oracle import evhinet_oracle as E

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {                                # name: (bins, multiple, norm, bgr, stamps)
    "pad4": (6, 4, True, False, "events"),
    "scalar": (6, 1, True, False, "events"),
    "bins2": (2, 4, True, False, "events"),
    "nonorm": (6, 4, False, False, "events"),
    "bgr": (6, 4, True, True, "events"),
    "bounds": (6, 4, True, False, "bounds"),
}


@functools.lru_cache(maxsize=None)
def _sequence():
    z, _ = R.load_fixture(GOLDEN)
    return z["frames"], z["events"], z["windows"]


def _items(stamps="events"):
    from refid_amd.sequence import frame_windows, make_pairs
    frames, ev, w = _sequence()
    return make_pairs(ev[:, 0], *frame_windows(w[:, 0], w[:, 1]), stamps=stamps)


@functools.lru_cache(maxsize=None)
def _case(name):
    bins, multiple, norm, bgr, stamps = CASES[name]
    frames, ev, _ = _sequence()
    items = _items(stamps)
    lq, voxel = R.assemble_items(frames, ev, items, bins, multiple=multiple, norm=norm, bgr=bgr)
    lq.setflags(write=False)
    voxel.setflags(write=False)
    return dict(items=items, lq=lq, voxel=voxel, bins=bins, multiple=multiple, norm=norm, bgr=bgr)


def _assembler(c, frames=None):
    from refid_amd.sequence import SequenceAssembler
    fr, ev, _ = _sequence()
    asm = SequenceAssembler(layout="single", num_bins=c["bins"], norm_voxel=c["norm"], multiple=c["multiple"])
    return asm.load(fr if frames is None else frames, ev, bgr=c["bgr"])


def _same_bits(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (what, int(bad.sum()), "elements differ; first at", np.argwhere(bad)[0].tolist(),
                           float(got[bad][0]), float(want[bad][0]))


@pytest.mark.parametrize("name", list(CASES))
def test_assembly_equals_the_restatement_bit_for_bit(name):
    c = _case(name)
    asm = _assembler(c)
    out = asm.assemble(c["items"])
    assert sorted(out) == ["lq", "voxel"]
    h, w = (28, 40) if c["multiple"] == 4 else (26, 38)
    assert tuple(out["lq"].shape) == (3, 3, h, w) and tuple(out["voxel"].shape) == (3, c["bins"], h, w)
    _same_bits(out["lq"], c["lq"], f"{name}: lq")
    _same_bits(out["voxel"], c["voxel"], f"{name}: voxel")
    assert out["voxel"].abs().max().item() > 1 and not torch.isnan(out["voxel"]).any()
    if c["norm"]:
        chunks = -(-c["bins"] * 26 * 38 // 4096)
        assert asm._cache[(3, 26, 38)]["parts"].numel() == 3 * chunks * 3 and chunks == (2 if c["bins"] == 6 else 1)
    if c["multiple"] == 4:
        assert out["voxel"][..., 26:, :].abs().max().item() == 0 and out["voxel"][..., :, 38:].abs().max().item() == 0
        assert torch.equal(out["lq"][..., 26:, :], out["lq"][..., 25:26, :].expand(-1, -1, 2, -1))
        assert torch.equal(out["lq"][..., :, 38:], out["lq"][..., :, 37:38].expand(-1, -1, -1, 2))


def _special_items():
    """An empty window, and a window holding one event (first == last: dT -> 1, one non-zero element, no spread)."""
    from refid_amd.sequence import Pair
    frames, ev, _ = _sequence()
    r = 1500
    return Pair(1, 1, 700, 700, 0.0, 0.0), Pair(2, 2, r, r + 1, float(ev[r, 0]), float(ev[r, 0]))


def test_one_call_with_a_normal_an_empty_and_a_one_event_item():
    c = _case("pad4")
    empty, one = _special_items()
    items = [c["items"][1], empty, one]
    frames, ev, _ = _sequence()
    out = _assembler(c).assemble(items)
    lq, voxel = R.assemble_items(frames, ev, items, 6, multiple=4)
    _same_bits(out["lq"], lq, "mixed: lq")
    _same_bits(out["voxel"], voxel, "mixed: voxel")
    assert not torch.isnan(out["voxel"]).any()
    assert out["voxel"][0].any() and not out["voxel"][1].any()
    assert not out["voxel"][2].any(), "one event: zeros, where the reference's 0/0 gives an all-NaN voxel"
    _same_bits(out["voxel"][0], c["voxel"][1], "the normal item is unchanged by its neighbours")
    plain = _assembler(_case("nonorm")).assemble(items)["voxel"]                # the one event did land before the norm
    assert plain[2].count_nonzero().item() == 1 and plain[2].sum().item() in (1.0, -1.0) and not plain[1].any()


def test_agreement_with_the_training_assembler():
    """A 24x32 crop of the frames (no padding; 4608 elements: two chunks): the items through DeviceBatchAssembler(
    layout='single', gt_size=None) -- per-item event slices, the same stamps, the blurry frame twice -- give the same bits."""
    from refid_amd.data import DeviceBatchAssembler
    frames, ev, _ = _sequence()
    crop = np.ascontiguousarray(frames[:, :24, :32])
    empty, one = _special_items()
    items = _items() + [empty, one]
    out = _assembler(dict(bins=6, norm=True, multiple=4, bgr=True), crop).assemble(items)
    assert tuple(out["voxel"].shape) == (5, 6, 24, 32)
    fr, evt = torch.from_numpy(crop), torch.from_numpy(ev)
    raw = [dict(frames=fr[[p.left, p.left]], events=evt[p.row0:p.row1].contiguous(), first_stamp=p.first_stamp,
                last_stamp=p.last_stamp) for p in items]
    ref = DeviceBatchAssembler(layout="single", num_bins=6, gt_size=None)(raw)
    assert torch.equal(out["lq"].view(torch.int32), ref["lq"].view(torch.int32))
    assert torch.equal(out["voxel"].view(torch.int32), ref["voxel"].view(torch.int32))
    assert out["voxel"][:3].abs().amax(dim=(1, 2, 3)).min().item() > 1


def test_table_position_item_count_and_repetition_do_not_change_a_bit():
    c = _case("pad4")
    asm = _assembler(c)
    empty, one = _special_items()
    base = c["items"][0]
    alone = asm.assemble([base])
    again = asm.assemble([base])
    three = asm.assemble([c["items"][2], empty, base])
    five = asm.assemble([one, c["items"][1], base, c["items"][1], base])
    for k in ("lq", "voxel"):
        assert torch.equal(alone[k], again[k]), ("two consecutive calls", k)
        assert torch.equal(alone[k][0], three[k][2]), ("position 2 of 3", k)
        assert torch.equal(alone[k][0], five[k][2]) and torch.equal(alone[k][0], five[k][4]), ("positions 2 and 4 of 5", k)
    _same_bits(alone["voxel"][0], c["voxel"][0], "alone")
    # statistics and finish again, into the outputs of the last call
    from refid_amd import _lib, ops
    want = five["voxel"].clone()
    five["voxel"].fill_(7.0)
    ops.seq_assemble_single(asm._last[0], _lib.ASSEMBLE_STATS | _lib.ASSEMBLE_FINISH)
    assert torch.equal(five["voxel"], want)


def test_rejected_arguments_name_the_field_and_launch_nothing():
    from refid_amd import ops
    from refid_amd._lib import RefidHipError
    c = _case("pad4")
    asm = _assembler(c)
    out = asm.assemble(c["items"])
    desc, table = asm._last
    n_events = len(_sequence()[1])
    out["lq"].fill_(7.0)
    out["voxel"].fill_(7.0)

    def rejected(obj, field, value, match):
        saved = getattr(obj, field)
        setattr(obj, field, value)
        try:
            with pytest.raises(RefidHipError, match=match):
                ops.seq_assemble_single(desc)
        finally:
            setattr(obj, field, saved)

    rejected(table[0], "left", 3, r"item 0: left 3 outside the 3 frames")
    rejected(table[1], "left", -1, r"item 1: left -1")
    rejected(table[2], "row0", table[2].row1 + 1, r"item 2: row0 \d+ > row1")
    rejected(table[0], "row0", -1, r"item 0: row0 -1")
    rejected(table[1], "row1", n_events + 1, rf"item 1: row1 {n_events + 1} > n_events {n_events}")
    rejected(desc, "out_h", 25, r"out_h 25 < height 26")
    rejected(desc, "out_w", 36, r"out_w 36 < width 38")
    rejected(desc, "bins", 3, r"num_bins == 3")
    rejected(desc, "bins", 0, r"num_bins >= 1")
    rejected(desc, "parts", None, r"parts .* non-null and 8-byte aligned")
    rejected(desc, "parts", desc.parts + 4, r"parts .* non-null and 8-byte aligned")
    rejected(desc, "lq", None, r"null outputs")
    rejected(desc, "voxel", None, r"null outputs")
    rejected(desc, "scratch", None, r"null scratch")
    rejected(desc, "n_items", 0, r"n_items 0")
    rejected(desc, "items_dev", None, r"both item tables")
    rejected(desc, "events", desc.events + 4, r"16-byte aligned")
    rejected(desc, "n_frames", 0, r"no frames")
    rejected(desc, "row_pitch", 3 * 38 - 1, r"row_pitch 113")
    table[0].right = -5                                                        # `right` is not read
    torch.cuda.synchronize()
    assert bool((out["lq"] == 7.0).all()) and bool((out["voxel"] == 7.0).all())         # nothing was launched
    ops.seq_assemble_single(desc)                                              # the untouched descriptor still runs
    _same_bits(out["lq"], c["lq"], "after the rejections: lq")
    _same_bits(out["voxel"], c["voxel"], "after the rejections: voxel")


# ---- SequenceDeblurrer and the command line ----------------------------------------------------------------------------------
# wf=8 is the smallest width the module accepts, depth=3 the shallowest depth the suite runs on the device
NET = dict(type="SingleMultiConnectEVHINet", wf=8, depth=3, ev_chn=6)


def _net():
    from refid_amd.archs import define_network
    net = define_network(deepcopy(NET)).to("cuda")
    net.load_state_dict(E.make_params(seed=4, wf=8, ev_chn=6))
    return net


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_deblurrer_frames_files_and_repeatability(tmp_path):
    from refid_amd.metrics import val_tail
    from refid_amd.png import read_png
    from refid_amd.sequence import SequenceDeblurrer
    c = _case("pad4")
    frames, ev, _ = _sequence()
    items = c["items"]
    net = _net()
    assert net.size_multiple == 4
    # what the contract says: the same minibatch slices of the assembled inputs through the network and the tail
    batch = _assembler(c).assemble(items)
    net.eval()
    want = []
    with torch.no_grad():
        for i, j in ((0, 2), (2, 3)):
            out = net(x=batch["lq"][i:j], event=batch["voxel"][i:j])[-1]
            assert tuple(out.shape) == (j - i, 3, 28, 40)
            want.append(val_tail(out[..., :26, :38], bgr=False).pred_u8)
    want = torch.cat(want).cpu().numpy()
    assert want.shape == (3, 26, 38, 3) and len(np.unique(want)) > 20
    net.train()
    deb = SequenceDeblurrer(net, 6, max_minibatch=2)
    assert deb.assembler.multiple == 4 and deb.assembler.layout == "single"
    got = deb.run(frames, ev, items, out_dir=str(tmp_path / "a"), keep=True)
    assert net.training is True                                                  # restored
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert _files(tmp_path / "a") == [f"{k:06d}.png" for k in range(3)]           # the frame index
    for k in range(3):
        assert np.array_equal(read_png(str(tmp_path / "a" / f"{k:06d}.png")), got[k]), k
    net.eval()
    again = deb.run(frames, ev, items, out_dir=str(tmp_path / "b"), names=list("xyz"), keep=True)
    assert net.training is False and np.array_equal(again, got)                   # a second run: the same bits
    assert _files(tmp_path / "b") == ["x.png", "y.png", "z.png"]
    before = _files(tmp_path)
    assert deb.run(frames, ev, items[:2]) is None and _files(tmp_path) == before  # nothing asked for


TEST_YAML = """
name: tiny-deblur
model_type: TestImageEventRestorationModel
num_gpu: 1
datasets:
  test:
    name: seq-test
    type: GoProSingleImageEventDataset
    num_bins: 6
network_g:
  type: SingleMultiConnectEVHINet
  wf: 8
  depth: 3
  ev_chn: 6
val:
  max_minibatch: 2
path:
  pretrain_network_g: ~
"""


def test_command_line_front(tmp_path):
    """python -m refid_amd.deblur, called in process: PNG frames, two event files, a stamps file, a test YAML and a
    checkpoint give the files SequenceDeblurrer gives for the same sequence."""
    from refid_amd import deblur
    from refid_amd.png import read_png, write_png
    from refid_amd.sequence import SequenceDeblurrer
    frames, ev, windows = _sequence()
    for k in range(3):
        write_png(str(tmp_path / "frames" / f"{k:03d}.png"), frames[k])
    half = len(ev) // 2
    for name, part in (("e0.npz", ev[:half]), ("e1.npz", ev[half:])):
        np.savez(tmp_path / name, x=part[:, 1], y=part[:, 2], timestamp=part[:, 0], polarity=part[:, 3])
    (tmp_path / "stamps.txt").write_text("".join(f"{a!r} {b!r}\n" for a, b in windows.tolist()))
    (tmp_path / "t.yml").write_text(TEST_YAML)
    net = _net()
    torch.save({"params": {"module." + k: v.cpu() for k, v in net.state_dict().items()}}, tmp_path / "w.pth")
    common = ["--opt", str(tmp_path / "t.yml"), "--checkpoint", str(tmp_path / "w.pth"), "--frames", str(tmp_path / "frames"),
              "--events", str(tmp_path / "e0.npz"), str(tmp_path / "e1.npz"), "--out", str(tmp_path / "out")]
    (tmp_path / "short.txt").write_text("2.02 2.2\n2.15 2.36\n")
    with pytest.raises(SystemExit, match="2 lines for 3 frames"):
        deblur.main(common + ["--stamps", str(tmp_path / "short.txt")])
    (tmp_path / "one.txt").write_text("2.02\n2.15\n2.38\n")
    with pytest.raises(SystemExit, match="start end"):
        deblur.main(common + ["--stamps", str(tmp_path / "one.txt")])
    assert _files(tmp_path / "out") == []
    assert deblur.main(common + ["--stamps", str(tmp_path / "stamps.txt")]) == 0
    want = SequenceDeblurrer(net, 6, max_minibatch=2).run(frames, ev, _items(), keep=True)
    assert _files(tmp_path / "out") == [f"{k:06d}.png" for k in range(3)]
    for k in range(3):
        assert np.array_equal(read_png(str(tmp_path / "out" / f"{k:06d}.png")), want[k]), k


# ---- val.grids for the 4-D network -------------------------------------------------------------------------------------------
TH, TW, CROP = 40, 56, 24


def _tiled_by_hand(net, x, ev, crop, mb):
    """The contract of tiled_forward in torch: the same tile order and minibatch composition, fp32 +=, then / count."""
    from refid_amd.tiling import grid_indices
    idx, ch, cw = grid_indices(x.shape[-2], x.shape[-1], crop)
    acc, cnt = torch.zeros_like(x[0]), torch.zeros_like(x[0, :1])
    with torch.no_grad():
        for k in range(0, len(idx), mb):
            part = idx[k:k + mb]
            xs = torch.cat([x[..., d["i"]:d["i"] + ch, d["j"]:d["j"] + cw] for d in part]).contiguous()
            es = torch.cat([ev[..., d["i"]:d["i"] + ch, d["j"]:d["j"] + cw] for d in part]).contiguous()
            out = net(x=xs, event=es)[-1]
            for n, d in enumerate(part):
                acc[:, d["i"]:d["i"] + ch, d["j"]:d["j"] + cw] += out[n]
                cnt[:, d["i"]:d["i"] + ch, d["j"]:d["j"] + cw] += 1
    return (acc / cnt).unsqueeze(0), cnt, len(idx)


def test_tiled_forward_of_the_4d_network():
    from refid_amd.tiling import tiled_forward
    net = _net().eval()
    x, ev, _ = E.make_inputs(1, TH, TW, ev_chn=6, seed=21)
    x, ev = x.cuda(), ev.cuda()
    for mb in (2, 4):
        want, cnt, tiles = _tiled_by_hand(net, x, ev, CROP, mb)
        assert tiles == 6 and sorted(cnt.unique().tolist()) == [1.0, 2.0, 4.0]
        got = tiled_forward(net, x, ev, CROP, max_minibatch=mb)
        assert tuple(got.shape) == (1, 3, TH, TW)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), mb
    with torch.no_grad():
        whole = net(x=x, event=ev)[-1]
    assert not torch.equal(got, whole), "half-instance-norm statistics are per tile: tiled and whole-frame outputs differ"
    big = tiled_forward(net, x, ev, 56)                                         # crop >= frame: one tile, the frame itself
    assert torch.equal(big.view(torch.int32), whole.view(torch.int32))
    with pytest.raises(RuntimeError, match="multiple of 4"):
        tiled_forward(net, x, ev, 22)
    with pytest.raises(AssertionError, match="batch 1"):
        tiled_forward(net, x.repeat(2, 1, 1, 1), ev.repeat(2, 1, 1, 1), CROP)


def test_validation_with_val_grids_runs_tiled_and_writes_its_files(tmp_path):
    from refid_amd.metrics import val_tail
    from refid_amd.png import read_png
    from refid_amd.tiling import tiled_forward
    from refid_amd.train import TestImageEventRestorationModel, create_model
    psnr = dict(type="calculate_psnr", crop_border=0, test_y_channel=False)
    opt = {"name": "tinygrids", "model_type": "TestImageEventRestorationModel", "is_train": False, "num_gpu": 1, "dist": False,
           "network_g": deepcopy(NET), "path": {"pretrain_network_g": None, "visualization": str(tmp_path)},
           "datasets": {"test": {"type": "GoProSingleImageEventDataset"}},
           "val": {"save_img": True, "grids": True, "crop_size": CROP, "max_minibatch": 4, "metrics": dict(psnr=psnr)}}
    model = create_model(opt)
    assert type(model) is TestImageEventRestorationModel
    model.net_g.load_state_dict(E.make_params(seed=4, wf=8, ev_chn=6))
    loader = []
    for k, (seq, idx) in enumerate([("seqA", "000004"), ("seqB", "000002")]):
        x, ev, gt = E.make_inputs(1, TH, TW, ev_chn=6, seed=50 + k)
        loader.append({"lq": x, "voxel": ev, "gt": gt, "seq": [seq], "origin_index": [idx]})
    model.validation(loader, 1, None, save_img=True)
    assert _files(tmp_path) == ["tinygrids/seqA/000004.png", "tinygrids/seqB/000002.png"]
    net = model.net_g.eval()
    for data in loader:
        tiled = tiled_forward(net, data["lq"].cuda(), data["voxel"].cuda(), CROP, max_minibatch=4)
        want = val_tail(tiled, bgr=False).pred_u8[0].cpu().numpy()
        with torch.no_grad():
            whole = val_tail(net(x=data["lq"].cuda(), event=data["voxel"].cuda())[-1], bgr=False).pred_u8[0].cpu().numpy()
        got = read_png(os.path.join(tmp_path, "tinygrids", data["seq"][0], data["origin_index"][0] + ".png"))
        assert np.array_equal(got, want) and not np.array_equal(got, whole)
    assert model.metric_results["psnr"] > 0


def test_deblurrer_with_crop_size_equals_tiled_forward_on_the_assembled_item():
    from refid_amd.metrics import val_tail
    from refid_amd.sequence import SequenceAssembler, SequenceDeblurrer
    from refid_amd.tiling import tiled_forward
    _, ev, _ = _sequence()
    rng = np.random.Generator(np.random.PCG64(12))
    frames = rng.integers(0, 256, (2, TH - 1, TW - 3, 3), dtype=np.uint8)        # 39x53 -> padded to 40x56
    items = _items()[:2]
    net = _net()
    deb = SequenceDeblurrer(net, 6, max_minibatch=2, crop_size=CROP)
    got = deb.run(frames, ev, items, keep=True)
    assert got.shape == (2, TH - 1, TW - 3, 3)
    batch = SequenceAssembler(layout="single", num_bins=6, multiple=4).load(frames, ev).assemble(items)
    assert tuple(batch["lq"].shape) == (2, 3, TH, TW)
    net.eval()
    for k in range(2):
        tiled = tiled_forward(net, batch["lq"][k:k + 1], batch["voxel"][k:k + 1], CROP, max_minibatch=2)
        want = val_tail(tiled[..., :TH - 1, :TW - 3], bgr=False).pred_u8[0].cpu().numpy()
        assert np.array_equal(got[k], want), k
    from refid_amd._lib import RefidHipError
    with pytest.raises(RefidHipError, match="multiple of"):
        SequenceDeblurrer(net, 6, crop_size=22)
