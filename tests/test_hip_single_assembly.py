"""MI355X: the single-image event deblurring path -- DeviceBatchAssembler(layout='single') (refid_assemble_single,
csrc/sample.hip) against the numpy restatement of its algorithm (tests/single_assembly_ref.py, pinned to the reference's
__getitem__ by test_single_assembly_host.py), the determinism of voxel_norm's reduction, and ImageEventRestorationModel's
validation loop.  Everything the kernels compute is integer arithmetic or one correctly rounded IEEE operation in a fixed
order, so the comparisons with the restatement are bit for bit (after + 0.0, which makes -0 and +0 the same)."""
import logging
import os
import random
from copy import deepcopy

import numpy as np
import pytest
import torch

import single_assembly_ref as S
from oracle import evhinet_oracle as E

pytestmark = pytest.mark.gpu

AUG = ("top", "left", "hflip", "vflip", "rot90")


def _raw(sample):
    out = {k: v for k, v in sample.items() if k != "crop_hw"}
    out["frames"] = torch.from_numpy(np.ascontiguousarray(sample["frames"]))
    out["events"] = torch.from_numpy(np.ascontiguousarray(sample["events"], dtype=np.float32).reshape(-1, 4))
    return out


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = (got + np.float32(0)).view(np.uint32) != (want + np.float32(0)).view(np.uint32)
    assert not bad.any(), (what, int(bad.sum()), "elements differ; first at", np.argwhere(bad)[0].tolist(),
                           float(got[bad][0]), float(want[bad][0]))


def _check(asm, samples, what):
    out = asm([_raw(s) for s in samples])
    lq, voxel, gt = S.assemble_batch(samples, asm.bins, asm.gt_size, asm.norm_voxel)
    for k, want in (("lq", lq), ("voxel", voxel), ("gt", gt)):
        _same(out[k], want, f"{what}: {k}")
    return out


def _fixture_samples(golden_dir, name):
    from refid_amd.data import draw_augmentation
    z, cfg = S.load_fixture(golden_dir, name)
    H, W = z["frames"].shape[1:3]
    samples = []
    for seed in cfg["seeds"]:
        aug = draw_augmentation(random.Random(seed), H, W, cfg["gt_size"], cfg["use_hflip"], cfg["use_rot"])
        samples.append(dict(frames=z["frames"], events=z["events"], **dict(zip(AUG, aug))))
    return cfg, samples


def _one_event(sample):
    """The sample with a single event at its first stamp: one non-zero element, no spread."""
    return dict(sample, events=np.array([[sample["events"][0, 0], sample["left"] + 3, sample["top"] + 2, 1]], np.float32))


# single_bins6: 32x32 crops x 6 bins = 6144 elements, the smallest fixture shape with MORE THAN ONE partial per sample
# (chunks of 4096), all eight flip / transpose combinations; single_bins2: 24x24 x 2 = 1152, one partial
@pytest.mark.parametrize("name", S.FIXTURES)
def test_fixtures_are_bit_identical_to_the_restatement(golden_dir, name):
    from refid_amd.data import DeviceBatchAssembler
    cfg, samples = _fixture_samples(golden_dir, name)
    asm = DeviceBatchAssembler(layout="single", num_bins=cfg["bins"], gt_size=cfg["gt_size"])
    out = _check(asm, samples, name)                                    # every seed of the fixture, as one batch
    assert out["lq"].shape == (len(samples), 3, cfg["gt_size"], cfg["gt_size"]) == out["gt"].shape
    assert out["voxel"].shape == (len(samples), cfg["bins"], cfg["gt_size"], cfg["gt_size"])
    assert out["voxel"].abs().max().item() > 3 and not torch.isnan(out["voxel"]).any()
    if name == "single_bins6":
        combos = {(s["hflip"], s["vflip"], s["rot90"]) for s in samples}
        assert len(combos) == 8 and asm._cache[(len(samples), 32, 32)]["parts"].numel() == 3 * 2 * len(samples)
    plain = DeviceBatchAssembler(layout="single", num_bins=cfg["bins"], gt_size=cfg["gt_size"], norm_voxel=False)
    _check(plain, samples[:2], name + " norm_voxel=False")


def test_mixed_batch_normal_empty_and_single_event(golden_dir):
    from refid_amd.data import DeviceBatchAssembler
    cfg, samples = _fixture_samples(golden_dir, "single_bins6")
    asm = DeviceBatchAssembler(layout="single", num_bins=6, gt_size=32)
    batch = [samples[1], dict(samples[2], events=samples[2]["events"][:0]), _one_event(samples[3])]
    out = _check(asm, batch, "mixed")
    assert out["voxel"][0].any() and not out["voxel"][1].any()
    assert not out["voxel"][2].any(), "one event: zeros, where the reference's 0/0 gives an all-NaN voxel"


# 21x37: neither the plane (777) nor the sample (777 * bins) is a multiple of 4 -- the scalar store path of both the
# finish and the frames stage; 20x37: the plane is (740), vector path; one bin: every event falls into bin 0
@pytest.mark.parametrize("crop_hw,bins", [((21, 37), 6), ((21, 37), 2), ((20, 37), 6), ((21, 37), 1)])
def test_non_square_crops(golden_dir, crop_hw, bins):
    import ctypes as C
    from refid_amd import _lib, ops
    z, cfg = S.load_fixture(golden_dir, "single_bins6")
    H, W = z["frames"].shape[1:3]
    samples = [dict(frames=z["frames"], events=z["events"], top=H - crop_hw[0], left=W - crop_hw[1], hflip=1, vflip=0, rot90=0,
                    crop_hw=crop_hw),
               dict(frames=z["frames"], events=z["events"], top=3, left=0, hflip=0, vflip=1, rot90=0, crop_hw=crop_hw)]
    # (DeviceBatchAssembler crops squares or keeps whole frames: a non-square crop goes through the descriptor itself)
    raws = [_raw(dict(s, frames=z["frames"][:, s["top"]:s["top"] + crop_hw[0], s["left"]:s["left"] + crop_hw[1]])) for s in samples]
    table, keep = (_lib.SampleDesc * 2)(), []
    for b, (s, r) in enumerate(zip(samples, raws)):
        fr, ev = r["frames"].contiguous().cuda(), r["events"].cuda()
        keep += [fr, ev]
        d = table[b]
        d.events, d.n_events = ev.data_ptr(), ev.shape[0]
        d.first_stamp, d.last_stamp = float(z["events"][0, 0]), float(z["events"][-1, 0])
        d.height, d.width = H, W
        d.frames, d.frame_stride, d.row_pitch = fr.data_ptr(), crop_hw[0] * crop_hw[1] * 3, crop_hw[1] * 3
        d.y0, d.x0, d.top, d.left = s["top"], s["left"], s["top"], s["left"]
        d.hflip, d.vflip, d.rot90 = s["hflip"], s["vflip"], 0
    tab_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    h, w = crop_hw
    lq, gt = torch.empty(2, 3, h, w, device="cuda"), torch.empty(2, 3, h, w, device="cuda")
    voxel = torch.empty(2, bins, h, w, device="cuda")
    desc = _lib.SingleDesc()
    desc.samples_host, desc.samples_dev = C.addressof(table), tab_dev.data_ptr()
    desc.batch, desc.bins, desc.crop_h, desc.crop_w, desc.norm = 2, bins, h, w, 1
    scratch = torch.empty(2, bins, h, w, dtype=torch.int64, device="cuda")
    parts = ops.voxel_norm_parts(2, bins * h * w, "cuda")
    desc.scratch, desc.parts = scratch.data_ptr(), parts.data_ptr()
    desc.lq, desc.voxel, desc.gt = lq.data_ptr(), voxel.data_ptr(), gt.data_ptr()
    ops.assemble_single(desc)
    want = S.assemble_batch(samples, bins, None)
    for got, ref, k in zip((lq, voxel, gt), want, ("lq", "voxel", "gt")):
        _same(got, ref, f"{crop_hw} bins {bins}: {k}")
    assert voxel.any()


def test_rejections_on_the_device(golden_dir):
    from refid_amd._lib import RefidHipError
    from refid_amd.data import DeviceBatchAssembler
    cfg, samples = _fixture_samples(golden_dir, "single_bins2")
    asm = DeviceBatchAssembler(layout="single", num_bins=2, gt_size=24)
    three = dict(_raw(samples[0]), frames=torch.zeros(3, 40, 56, 3, dtype=torch.uint8))
    with pytest.raises(RefidHipError, match=r"\(2, H, W, 3\)"):
        asm([three])


def test_batch_position_batch_size_and_repetition_do_not_change_a_bit(golden_dir):
    from refid_amd.data import DeviceBatchAssembler
    cfg, samples = _fixture_samples(golden_dir, "single_bins6")
    asm = DeviceBatchAssembler(layout="single", num_bins=6, gt_size=32)
    base = samples[4]
    alone = asm([_raw(base)])
    again = asm([_raw(base)])
    others = [samples[0], dict(samples[1], events=samples[1]["events"][:0]), _one_event(samples[2]), samples[5]]
    three = asm([_raw(s) for s in (others[0], others[1], base)])
    five = asm([_raw(s) for s in others + [base]])
    for k in ("lq", "voxel", "gt"):
        assert torch.equal(alone[k], again[k]), ("two consecutive calls", k)
        assert torch.equal(alone[k][0], three[k][2]), ("position 2 of 3", k)
        assert torch.equal(alone[k][0], five[k][4]), ("position 4 of 5", k)
    assert alone["voxel"].any()


def test_fused_route_equals_voxel_norm_of_the_unnormalised_output(golden_dir):
    from refid_amd import _lib, ops
    from refid_amd.data import DeviceBatchAssembler
    cfg, samples = _fixture_samples(golden_dir, "single_bins6")
    batch = samples[:3] + [_one_event(samples[3])]
    asm = DeviceBatchAssembler(layout="single", num_bins=6, gt_size=32)
    out = asm([_raw(s) for s in batch])
    fused = out["voxel"].clone()
    plain = DeviceBatchAssembler(layout="single", num_bins=6, gt_size=32, norm_voxel=False)([_raw(s) for s in batch])["voxel"]
    assert plain.any() and not torch.equal(plain, fused)
    assert torch.equal(ops.voxel_norm(plain), fused)
    # rerun() of the new stage: statistics and finish again, into the outputs of the last call
    out["voxel"].zero_()
    asm.rerun(_lib.ASSEMBLE_STATS | _lib.ASSEMBLE_FINISH)
    assert torch.equal(out["voxel"], fused)


# ---- the validation loop of ImageEventRestorationModel ------------------------------------------------------------------
H, W, BINS = 16, 24, 6
PSNR, SSIM = dict(type="calculate_psnr", crop_border=0, test_y_channel=False), dict(type="calculate_ssim", crop_border=0,
                                                                                  test_y_channel=False)
# wf=8 is the smallest width the module accepts (a multiple of 8); depth=3 (the default) is the shallowest depth the suite
# runs on the device, so the loop is tested on a configuration whose kernels are tested elsewhere
NET = dict(type="SingleMultiConnectEVHINet", wf=8, ev_chn=BINS)


def _opt(vis, is_train, model_type="ImageEventRestorationModel"):
    opt = {"name": "tinysingle", "model_type": model_type, "is_train": is_train, "num_gpu": 1, "dist": False,
           "network_g": dict(NET), "path": {"pretrain_network_g": None, "visualization": str(vis)},
           "datasets": {"val": {"type": "GoProSingleImageEventDataset"}, "test": {"type": "GoProSingleImageEventDataset"}},
           "val": {"save_img": True, "save_gt": True, "metrics": dict(psnr=deepcopy(PSNR), ssim=deepcopy(SSIM))}}
    if is_train:
        opt["train"] = {"optim_g": dict(type="AdamW", lr=2e-4, weight_decay=1e-4, betas=[0.9, 0.99]),
                        "scheduler": dict(type="TrueCosineAnnealingLR", T_max=50, eta_min=1e-7),
                        "pixel_opt": dict(type="PSNRLoss", loss_weight=0.5, reduction="mean")}
    return opt


def _model(vis, is_train, model_type="ImageEventRestorationModel"):
    from refid_amd.train import create_model
    model = create_model(_opt(vis, is_train, model_type))
    model.net_g.load_state_dict(E.make_params(seed=4, wf=8, ev_chn=BINS))
    return model


def _loader():
    """Three items over two sequences."""
    items = []
    for k, (seq, idx) in enumerate([("seqA", "000004"), ("seqA", "000011"), ("seqB", "000002")]):
        x, ev, gt = E.make_inputs(1, H, W, ev_chn=BINS, seed=30 + k)
        items.append({"lq": x, "voxel": ev, "gt": gt, "seq": [seq], "origin_index": [idx]})
    return items


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.fixture(scope="module")
def expected(tmp_path_factory):
    """Per item: the network's output through model.test() and metrics.val_tail on it."""
    from refid_amd import metrics
    model = _model(tmp_path_factory.mktemp("unused"), False)
    outs, psnr, ssim, pred_u8, gt_u8 = [], [], [], [], []
    for data in _loader():
        model.feed_data(data)
        model.test()
        assert model.output.shape == (1, 3, H, W)
        tail = metrics.val_tail(model.output, model.gt, bgr=False, want_gt_u8=True)
        outs.append(model.output.clone())
        psnr += tail.psnr
        ssim += tail.ssim
        pred_u8.append(tail.pred_u8[0].cpu().numpy())
        gt_u8.append(tail.gt_u8[0].cpu().numpy())
    return dict(outs=outs, psnr=sum(psnr) / 3, ssim=sum(ssim) / 3, pred_u8=pred_u8, gt_u8=gt_u8)


class _Tb:
    def __init__(self):
        self.calls = []

    def add_scalar(self, *a):
        self.calls.append(a)


def test_validation_in_test_mode_files_metrics_and_log(tmp_path, expected, caplog):
    from refid_amd.png import read_png
    from refid_amd.train import TestImageEventRestorationModel
    model = _model(tmp_path, False, "TestImageEventRestorationModel")
    assert type(model) is TestImageEventRestorationModel
    tb = _Tb()
    with caplog.at_level(logging.INFO, logger="basicsr"):
        ret = model.validation(_loader(), 7, tb, save_img=True)
    want = {}
    for k, data in enumerate(_loader()):
        stem = os.path.join("tinysingle", data["seq"][0], data["origin_index"][0])
        want[stem + ".png"], want[stem + "_gt.png"] = expected["pred_u8"][k], expected["gt_u8"][k]
    assert _files(tmp_path) == sorted(want) and len(want) == 6
    for rel, img in want.items():
        assert np.array_equal(read_png(os.path.join(tmp_path, rel)), img), rel
    assert list(model.metric_results) == ["psnr", "ssim"]
    assert model.metric_results["psnr"] == expected["psnr"] and model.metric_results["ssim"] == expected["ssim"]
    assert ret == model.metric_results["ssim"]                         # the last metric in dict order
    lines = [r.getMessage() for r in caplog.records if r.name == "basicsr" and r.getMessage().startswith("Validation")]
    assert lines == [f"Validation tinysingle,\t\t # psnr: {expected['psnr']:.4f}\t # ssim: {expected['ssim']:.4f}"]
    assert tb.calls == [("metrics/psnr", expected["psnr"], 7), ("metrics/ssim", expected["ssim"], 7)]
    assert not hasattr(model, "metric_results_deblur")


def test_validation_while_training_writes_the_second_item_only(tmp_path, expected):
    from refid_amd.png import read_png
    model = _model(tmp_path, True)
    ret = model.validation(_loader(), 250, None, save_img=True)
    assert _files(tmp_path) == [os.path.join("000011", "000011_250.png"), os.path.join("000011", "000011_250_gt.png")]
    assert np.array_equal(read_png(os.path.join(tmp_path, "000011", "000011_250.png")), expected["pred_u8"][1])
    assert np.array_equal(read_png(os.path.join(tmp_path, "000011", "000011_250_gt.png")), expected["gt_u8"][1])
    assert ret == expected["ssim"] and model.metric_results["psnr"] == expected["psnr"]
    model.opt["val"]["save_gt"] = False                                 # save_gt is honoured
    model.validation(_loader(), 300, None, save_img=True)
    assert os.path.join("000011", "000011_300.png") in _files(tmp_path) and len(_files(tmp_path)) == 3
    model.opt["val"]["metrics"] = None                                  # no metrics: 0., nothing published anew
    assert model.validation(_loader(), 1, None, save_img=False) == 0.


def test_prefetcher_feeds_one_training_step(golden_dir, tmp_path):
    from refid_amd.data import CUDAPrefetcher
    from refid_amd.options import assembler_from_dataset_opt
    z, cfg = S.load_fixture(golden_dir, "single_bins6")
    Hf, Wf = z["frames"].shape[1:3]
    asm = assembler_from_dataset_opt(dict(type="GoProSingleImageEventDataset", num_bins=BINS, gt_size=32, use_hflip=True,
                                          use_rot=True, device_assemble=True))
    rng = random.Random(5)
    raw = [[dict(frames=torch.from_numpy(z["frames"]), events=torch.from_numpy(z["events"]), seq="seqA",
                 origin_index=f"{k:06d}", **asm.draw(rng, Hf, Wf)) for k in range(2)]]
    model = _model(tmp_path, True)
    pre = CUDAPrefetcher(raw, model.opt, assemble=asm)
    batch = pre.next()
    assert batch["lq"].shape == (2, 3, 32, 32) and batch["voxel"].shape == (2, BINS, 32, 32) and batch["seq"] == ["seqA"] * 2
    assert pre.next() is None
    model.update_learning_rate(1)
    model.feed_data(batch)
    model.optimize_parameters(1)
    loss = model.get_current_log()["l_pix"]
    assert np.isfinite(loss), loss
    assert model.seq_name == "seqA" and model.origin_index == "000000"
