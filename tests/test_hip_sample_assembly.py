"""MI355X: refid_amd.data.DeviceBatchAssembler (csrc/sample.hip) against the numpy restatement of its algorithm
(tests/sample_assembly_ref.py, itself pinned to the reference's __getitem__ by test_sample_assembly_host.py).

Everything the kernels compute is integer arithmetic or a single correctly rounded fp32 operation, so every comparison
here is BIT-identical: a differing bit is a bug (FMA contraction, a reciprocal instead of a division, a float atomic)."""
import random

import numpy as np
import pytest
import torch

import sample_assembly_ref as R

pytestmark = pytest.mark.gpu

AUG = ("top", "left", "hflip", "vflip", "rot90")


def _raw(sample):
    """numpy raw sample -> the tensors DeviceBatchAssembler takes (host memory)."""
    out = dict(sample)
    out["frames"] = torch.from_numpy(np.ascontiguousarray(sample["frames"]))
    out["events"] = torch.from_numpy(np.ascontiguousarray(sample["events"], dtype=np.float32).reshape(-1, 4))
    return out


def _same_bits(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (what, int(bad.sum()), "elements differ; first at", np.argwhere(bad)[0].tolist(),
                           float(got[bad][0]), float(want[bad][0]))


def _check(asm, samples, what):
    """Assembles `samples` as one batch and compares all three outputs with the restatement; returns the device batch."""
    out = asm([_raw(s) for s in samples])
    lq, voxel, gt = R.assemble_batch(samples, asm.m, asm.n, asm.layout, asm.gt_size)
    _same_bits(out["lq"], lq, what + ": lq")
    _same_bits(out["voxel"], voxel, what + ": voxel")
    _same_bits(out["gt"], gt, what + ": gt")
    return out


def _fixture_samples(golden_dir, name):
    from refid_amd.data import draw_augmentation
    z, cfg = R.load_fixture(golden_dir, name)
    H, W = z["frames"].shape[1:3]
    samples = []
    for seed in cfg["seeds"]:
        aug = draw_augmentation(random.Random(seed), H, W, cfg["gt_size"], cfg["use_hflip"], cfg["use_rot"])
        samples.append(dict(frames=z["frames"], events=z["events"], **dict(zip(AUG, aug))))
    return cfg, samples


@pytest.mark.parametrize("name", R.FIXTURES)
def test_fixtures_are_bit_identical_to_the_restatement(golden_dir, name):
    from refid_amd.data import DeviceBatchAssembler
    cfg, samples = _fixture_samples(golden_dir, name)
    asm = DeviceBatchAssembler(cfg["m"], cfg["n"], cfg["layout"], cfg["gt_size"])
    out = _check(asm, samples, name)                                    # every seed of the fixture, as one batch
    assert out["voxel"].abs().max().item() > 10                          # the hot pixel is there
    _check(asm, samples[:1], name + " alone")                            # another batch size, cached geometry or not


def test_event_order_prefilter_and_batch_position_do_not_change_a_bit(golden_dir):
    from refid_amd.data import DeviceBatchAssembler
    cfg, samples = _fixture_samples(golden_dir, "sample_blur_m3")
    asm = DeviceBatchAssembler(cfg["m"], cfg["n"], cfg["layout"], cfg["gt_size"])
    base = samples[1]
    ev = base["events"]
    stamps = dict(first_stamp=float(ev[0, 0]), last_stamp=float(ev[-1, 0]))
    alone = asm([_raw(base)])
    rng = np.random.Generator(np.random.PCG64(3))
    shuffled = dict(base, events=ev[rng.permutation(len(ev))], **stamps)
    x, y, g = ev[:, 1].astype(np.int64), ev[:, 2].astype(np.int64), cfg["gt_size"]
    inside = (x >= base["left"]) & (x < base["left"] + g) & (y >= base["top"]) & (y < base["top"] + g)
    assert 2000 < inside.sum() < len(ev)
    filtered = dict(base, events=ev[inside], **stamps)
    empty_crop = dict(samples[2], events=ev[~inside], top=base["top"], left=base["left"], **stamps)   # no event in its crop
    no_events = dict(samples[0], events=ev[:0], **stamps)
    for variant, what in ((shuffled, "shuffled"), (filtered, "pre-filtered")):
        got = asm([_raw(variant)])
        for k in ("lq", "voxel", "gt"):
            assert torch.equal(got[k], alone[k]), (what, k)
    others = [shuffled, empty_crop, dict(samples[3], events=ev[::3], **stamps), no_events]
    for pos in range(3):
        batch = others[:3]
        batch[pos] = base if pos != 1 else filtered
        if pos == 1:
            batch[0] = empty_crop                                        # keep the empty sample in every batch
        got = _check(asm, batch, f"position {pos}")
        for k in ("lq", "voxel", "gt"):
            assert torch.equal(got[k][pos], alone[k][0]), (pos, k)
    got = _check(asm, [empty_crop, base, no_events], "empty samples")
    m = cfg["m"]
    for b in (0, 2):
        assert got["voxel"][b].abs().max().item() == 0
        lq = got["lq"][b].cpu().numpy()
        assert np.all(R.voxel_channels(lq, m, "blur") == 0)
        img = R.image_channels(lq, m, "blur")
        assert img.min() >= 0 and img.max() <= 1 and len(np.unique(img)) > 100     # the image channels are still filled


def _edge_events(H, W, first, last, bins):
    """Rows [t, x, y, p] on every edge of the scatter's domain (the restatement decides what each contributes)."""
    span = last - first
    rows = [
        (first, 3, 2, 1), (last, 3, 2, 1), (last, 5, 2, 0),                          # ti = bins-1: no right bin
        (first + span * 3 / (bins - 1), 4, 2, 1),                                       # dts == 0 (span chosen so it is exact)
        (first + span * 0.37, W - 1, 5, 1), (first + span * 0.37, 6, H - 1, 0), (first + span * 0.61, W - 1, H - 1, 1),
        (first + span * 0.5, W, 3, 1), (first + span * 0.5, 3, H, 1), (first + span * 0.5, -1, 3, 1),
        (first + span * 0.5, 3, -1, 0), (first + span * 0.5, -0.5, 4, 1),               # -0.5 truncates to pixel 0
        (first + span * 0.5, 1e9, 3, 1), (first + span * 0.5, 3, -1e9, 1),
        (first - span * 0.1, 3, 3, 1), (last + span * 0.01, 3, 3, 1), (last + span * 2, 3, 3, 0),   # ts < 0, ts > bins-1, ti >= bins
        (first + span * 0.25, 0, 0, -1), (first + span * 0.75, 0, 0, 0),                # polarity -1 and 0 both count as -1
    ]
    rng = np.random.Generator(np.random.PCG64(9))
    n = 600
    rnd = np.stack([rng.uniform(first, last, n), rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n)], axis=1)
    return np.concatenate([np.array(rows, dtype=np.float64), rnd]).astype(np.float32)


def test_edges_of_time_frame_and_crop():
    from refid_amd._lib import RefidHipError
    from refid_amd.data import DeviceBatchAssembler
    m, n, H, W = 3, 1, 24, 40
    bins = 2 * m + n + 1
    rng = np.random.Generator(np.random.PCG64(21))
    frames = rng.integers(0, 256, (bins + 1, H, W, 3), dtype=np.uint8)
    ev = _edge_events(H, W, 8.0, 15.0, bins)                                            # span 7 = bins - 1: ts = t - first
    stamps = dict(first_stamp=8.0, last_stamp=15.0)
    keep, ti, _, q, _ = R.event_terms(ev, 8.0, 15.0, bins, H, W, 0, 0, H, W, False, False, False)
    assert keep[:7].all() and not keep[7:11].any() and keep[11] and not keep[12:15].any() and keep[15] and not keep[16]
    assert ti[1] == bins - 1 and q[3] == 0 and ti[3] == 3
    crop16 = DeviceBatchAssembler(m, n, "blur", 16)
    corners = [dict(frames=frames, events=ev, top=t, left=l, hflip=h, vflip=v, rot90=r, **stamps)
               for (t, l, h, v, r) in ((0, 0, 0, 0, 0), (H - 16, W - 16, 1, 0, 1), (0, W - 16, 0, 1, 1), (H - 16, 0, 1, 1, 0))]
    _check(crop16, corners, "corner crops")
    whole = DeviceBatchAssembler(m, n, "blur", None)                                     # 24x40: not square, 960 = 15 x 64 lanes
    _check(whole, [dict(frames=frames, events=ev, hflip=1, vflip=1, **stamps),
                   dict(frames=frames, events=ev, **stamps)], "whole frame 24x40")
    same_t = ev.copy()
    same_t[:, 0] = 11.0                                                                  # dT == 0 -> 1: everything in bin 0
    got = _check(whole, [dict(frames=frames, events=same_t)], "dT == 0")
    assert got["voxel"][0, 0, 0].abs().max().item() > 0 and got["voxel"][0, :, 1].abs().max().item() == 0
    with pytest.raises(RefidHipError, match="square"):
        whole([_raw(dict(frames=frames, events=ev, rot90=1, **stamps))])
    with pytest.raises(RefidHipError, match="does not fit"):
        crop16([_raw(dict(frames=frames, events=ev, top=H - 15, left=0, **stamps))])
    with pytest.raises(RefidHipError, match="img2tensor"):
        DeviceBatchAssembler(1, 2, "sharp", 16)                                          # num_bins == 3
    # an uploaded window instead of whole frames: same bits as the whole frames
    top, left = 5, 13
    win = dict(frames=frames[:, 4:22, 10:31], origin=(4, 10), frame_hw=(H, W), events=ev, top=top, left=left, hflip=1, **stamps)
    a = crop16([_raw(win)])
    b = _check(crop16, [dict(frames=frames, events=ev, top=top, left=left, hflip=1, **stamps)], "window")
    for k in ("lq", "voxel", "gt"):
        assert torch.equal(a[k], b[k]), k


def test_planes_off_the_vector_path_and_over_several_blocks(golden_dir):
    """5x7 planes (35 elements: scalar stores) and 40x56 planes (2240 elements: three blocks of four-element lanes)."""
    from refid_amd.data import DeviceBatchAssembler
    z, cfg = R.load_fixture(golden_dir, "sample_blur_m3")
    whole = DeviceBatchAssembler(cfg["m"], cfg["n"], "blur", None)
    _check(whole, [dict(frames=z["frames"], events=z["events"], hflip=1), dict(frames=z["frames"], events=z["events"], vflip=1)],
           "40x56")
    ev = z["events"].copy()
    ev[:, 1] %= 7
    ev[:, 2] %= 5
    small = np.ascontiguousarray(z["frames"][:, 3:8, 2:9])
    _check(whole, [dict(frames=small, events=ev, hflip=1, vflip=1), dict(frames=small, events=ev[:100])], "5x7")
    odd = DeviceBatchAssembler(cfg["m"], cfg["n"], "blur", 5)                            # 25 elements, with the transpose
    _check(odd, [dict(frames=small, events=ev, top=0, left=2, hflip=1, rot90=1)], "5x5 transposed")


class _Loader:
    def __init__(self, batches):
        self.batches = batches

    def __iter__(self):
        return iter(self.batches)


def test_prefetcher_assembles_on_its_side_stream(golden_dir):
    from refid_amd.data import CUDAPrefetcher, DeviceBatchAssembler
    cfg, samples = _fixture_samples(golden_dir, "sample_blur_m11")
    asm = DeviceBatchAssembler(cfg["m"], cfg["n"], cfg["layout"], cfg["gt_size"])
    batches = [[dict(_raw(samples[i]), origin_index=str(i)), dict(_raw(samples[j]), origin_index=str(j))]
               for i, j in ((0, 1), (1, 2), (2, 0))]
    direct = [asm(b) for b in batches]
    torch.cuda.synchronize()                                             # (an assembler's scratch belongs to one stream at a time)
    pre = CUDAPrefetcher(_Loader(batches), {"num_gpu": 1}, assemble=asm)
    for epoch in range(2):
        for want in direct:
            got = pre.next()
            assert sorted(got) == ["gt", "lq", "origin_index", "voxel"] and got["origin_index"] == want["origin_index"]
            for k in ("lq", "voxel", "gt"):
                assert got[k].is_cuda and torch.equal(got[k], want[k]), k
        assert pre.next() is None
        pre.reset()
    # without an assembler: the tensors of the loader's dicts, moved to the device, as before
    plain = [{"lq": torch.randn(2, 6, 8, 8), "voxel": torch.randn(2, 3, 2, 8, 8), "seq": "s%d" % i} for i in range(3)]
    pre = CUDAPrefetcher(_Loader(plain), {"num_gpu": 1})
    for want in plain:
        got = pre.next()
        assert got["seq"] == want["seq"] and got["lq"].is_cuda
        assert torch.equal(got["lq"].cpu(), want["lq"]) and torch.equal(got["voxel"].cpu(), want["voxel"])
    assert pre.next() is None


def test_an_assembled_batch_trains_like_the_restated_one(golden_dir):
    """m=11, n=1 (26 channels, T=23) at 16x16 through feed_data + optimize_parameters of the tiny model of
    test_hip_train_step.py: finite loss, bit-equal to feeding the tensors the numpy restatement builds."""
    from oracle import refid_oracle as O
    from refid_amd.data import DeviceBatchAssembler
    from refid_amd.train import TwoImageEventRecurrentRestorationModel
    cfg, samples = _fixture_samples(golden_dir, "sample_blur_m11")
    asm = DeviceBatchAssembler(cfg["m"], cfg["n"], cfg["layout"], cfg["gt_size"])
    samples = samples[:2]
    dev = asm([_raw(s) for s in samples])
    host = dict(zip(("lq", "voxel", "gt"), (torch.from_numpy(a) for a in R.assemble_batch(samples, 11, 1, "blur", 16))))
    assert tuple(dev["lq"].shape) == (2, 26, 16, 16) and tuple(dev["voxel"].shape) == (2, 23, 2, 16, 16)
    opt = {
        "name": "t", "is_train": True, "num_gpu": 1,
        "network_g": dict(type="FinalBidirectionAttenfusion", img_chn=26, ev_chn=2, num_encoders=3, base_num_channels=8,
                          num_block=1, num_residual_blocks=2, compute_dtype="fp32"),
        "path": {"pretrain_network_g": None},
        "train": {"optim_g": dict(type="AdamW", lr=2e-4, weight_decay=1e-4, betas=[0.9, 0.99]),
                  "scheduler": dict(type="TrueCosineAnnealingLR", T_max=50, eta_min=1e-7),
                  "pixel_opt": dict(type="CharbonnierLoss", loss_weight=1, reduction="mean"), "use_grad_clip": True},
        "val": {"max_minibatch": 2},
    }
    P = O.make_params(26, base_num_channels=8, mode="hash", seed=5)
    losses = []
    for data in (dev, host):
        model = TwoImageEventRecurrentRestorationModel(opt)
        model.net_g.load_state_dict(P, strict=True)
        model.update_learning_rate(1)
        model.feed_data(data)
        model.optimize_parameters(1)
        losses.append(model.get_current_log()["l_pix"])
    assert np.isfinite(losses[0]) and losses[0] > 0
    assert losses[0] == losses[1], losses
