"""GPU: TwoImageEventRecurrentRestorationModel.validation / nondist_validation / dist_validation /
single_image_inference on a tiny network: the files written, their pixels, the metrics, the log lines and the failure
path of the PNG writer pool."""
import logging
import os
from copy import deepcopy

import numpy as np
import pytest
import torch

from oracle import refid_oracle as O

pytestmark = pytest.mark.gpu

M, N, H, W = 1, 3, 24, 40
T = 2 * M + N
PSNR, SSIM = dict(type="calculate_psnr", crop_border=0, test_y_channel=False), dict(type="calculate_ssim", crop_border=0,
                                                                                  test_y_channel=False)


def _opt(vis, **val):
    return {"name": "tinyval", "is_train": False, "num_gpu": 1, "dist": False,
            "network_g": dict(type="FinalBidirectionAttenfusion", img_chn=6, ev_chn=2, num_encoders=3, base_num_channels=8,
                              num_block=1),
            "path": {"pretrain_network_g": None, "visualization": str(vis)},
            "datasets": {"val": {"num_end_interpolation": M, "num_inter_interpolation": N}},
            "val": dict({"save_img": True, "save_gt": True, "metrics_deblur": dict(psnr=deepcopy(PSNR), ssim=deepcopy(SSIM)),
                         "metrics_interpo": dict(psnr=deepcopy(PSNR), ssim=deepcopy(SSIM))}, **val)}


def _model(vis, **val):
    from refid_amd.train import TwoImageEventRecurrentRestorationModel
    model = TwoImageEventRecurrentRestorationModel(_opt(vis, **val))
    model.net_g.load_state_dict(O.make_params(6, base_num_channels=8, mode="hash", seed=3))
    return model


def _loader():
    """3 items over 2 sequence names; the second item holds two samples."""
    items = []
    for k, (b, seq, idx) in enumerate([(1, ["seqA"], ["000004"]), (2, ["seqA", "seqB"], ["000011", "000002"]),
                                       (1, ["seqB"], ["000009"])]):
        x, ev, gt = O.make_inputs(b, T, H, W, 6, seed=20 + k)
        items.append({"lq": x, "voxel": ev, "gt": gt, "seq": seq, "origin_index": idx})
    return items


@pytest.fixture(scope="module")
def expected(tmp_path_factory):
    """Per item: the network's output through model.test() and the existing per-frame metric kernels on it."""
    from refid_amd.metrics import ValidationMetrics, calculate_psnr_frames, calculate_ssim_frames
    model = _model(tmp_path_factory.mktemp("unused"))
    book = ValidationMetrics(dict(psnr=PSNR, ssim=SSIM), dict(psnr=PSNR, ssim=SSIM), M, N)
    outs = []
    for data in _loader():
        model.feed_data(data)
        model.test()
        outs.append(model.output.clone())
        ps, ss = calculate_psnr_frames(model.output, model.gt), calculate_ssim_frames(model.output, model.gt)
        for i in range(model.output.shape[0]):
            book.add_item({"calculate_psnr": ps[i * T:(i + 1) * T], "calculate_ssim": ss[i * T:(i + 1) * T]})
    ret = book.finish()
    return dict(outs=outs, book=book, ret=ret)


def _rgb_u8(frame):
    return O.tensor2img_u8(frame).permute(1, 2, 0).cpu().numpy()


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _check_metrics(model, ret, expected):
    book = expected["book"]
    for got, want in ((model.metric_results_deblur, book.deblur), (model.metric_results_interpo, book.interpo),
                      (model.metric_results_total, book.total)):
        assert list(got) == ["psnr", "ssim"]
        print(got, want)
        assert abs(got["psnr"] - want["psnr"]) <= 1e-12 * abs(want["psnr"]) and abs(got["ssim"] - want["ssim"]) <= 2e-5
    assert ret == model.metric_results_interpo["ssim"]


class _Tb:
    def __init__(self):
        self.calls = []

    def add_scalar(self, *a):
        self.calls.append(a)


def test_files_pixels_metrics_and_log(tmp_path, expected, caplog):
    from refid_amd.png import read_png
    model = _model(tmp_path)
    model.net_g.eval()
    tb = _Tb()
    with caplog.at_level(logging.INFO, logger="basicsr"):
        ret = model.validation(_loader(), 7, tb, save_img=True)
    assert model.net_g.training is False                     # restored (test() itself leaves the network in train mode)
    want = {}
    for data, out in zip(_loader(), expected["outs"]):
        for i in range(out.shape[0]):
            for f in range(T):
                stem = os.path.join("tinyval", data["seq"][i], f"{data['origin_index'][i]}_{f:02d}")
                want[stem + ".png"] = _rgb_u8(out[i, f])
                want[stem + "_gt.png"] = _rgb_u8(data["gt"][i, f])
    assert _files(tmp_path) == sorted(want) and len(want) == 4 * T * 2
    for rel, img in want.items():
        assert np.array_equal(read_png(os.path.join(tmp_path, rel)), img), rel
    _check_metrics(model, ret, expected)
    lines = [r.getMessage() for r in caplog.records if r.name == "basicsr"]
    assert lines == model_lines(model)
    assert tb.calls == [(f"metrics/{k}", v, 7) for res in (model.metric_results_deblur, model.metric_results_interpo)
                        for k, v in res.items()]
    assert model.seq_name == "seqB" and model.origin_index == "000009"


def model_lines(model):
    out = []
    for tag, res in (("total", model.metric_results_total), ("deblur", model.metric_results_deblur),
                     ("interpolation", model.metric_results_interpo)):
        out.append(f"Validation tinyval [{tag}],\t" + "".join(f"\t # {k}: {v:.4f}" for k, v in res.items()))
    return out


def test_no_save_img_writes_nothing_and_gives_the_same_metrics(tmp_path, expected):
    model = _model(tmp_path)
    ret = model.nondist_validation(_loader(), 1, None, False, True, True)
    assert model.net_g.training is True and _files(tmp_path) == []
    _check_metrics(model, ret, expected)
    model.opt["val"]["save_gt"] = False                      # save_gt is honoured
    model.nondist_validation(_loader()[:1], 1, None, True, True, True)
    assert _files(tmp_path) == [os.path.join("tinyval", "seqA", f"000004_{f:02d}.png") for f in range(T)]


def test_grids_go_through_tiled_forward(tmp_path):
    from refid_amd.png import read_png
    from refid_amd.tiling import tiled_forward
    model = _model(tmp_path, grids=True, crop_size=16, max_minibatch=2, save_gt=False)
    data = _loader()[0]
    model.nondist_validation([data], 1, None, True, True, True)
    model.net_g.eval()
    want = tiled_forward(model.net_g, data["lq"].cuda(), data["voxel"].cuda(), 16, 2)
    assert torch.equal(model.output, want)
    for f in range(T):
        got = read_png(os.path.join(tmp_path, "tinyval", "seqA", f"000004_{f:02d}.png"))
        assert np.array_equal(got, _rgb_u8(want[0, f]))


def test_dist_validation_other_ranks_return_zero(tmp_path, expected):
    model = _model(tmp_path)
    model.opt["dist"] = True
    model.rank = 1
    assert model.validation(_loader(), 1, None, save_img=True) == 0. and _files(tmp_path) == []
    model.rank = 0
    ret = model.validation(_loader(), 1, None, save_img=False)
    _check_metrics(model, ret, expected)


def test_single_image_inference(tmp_path, expected):
    from refid_amd.png import read_png
    model = _model(tmp_path)
    data = _loader()[0]
    path = os.path.join(tmp_path, "sub", "one.png")
    model.single_image_inference(data["lq"][0], data["voxel"][0], path)
    want = np.concatenate([_rgb_u8(expected["outs"][0][0, f]) for f in range(T)], axis=0)
    assert _files(tmp_path) == [os.path.join("sub", "one.png")] and np.array_equal(read_png(path), want)
    vis = model.get_current_visuals()
    assert list(vis) == ["lq", "result"] and not vis["result"].is_cuda
    assert torch.equal(vis["result"], expected["outs"][0].cpu())


def test_worker_failure_raises(tmp_path):
    blocker = tmp_path / "file"
    blocker.write_text("not a directory")
    model = _model(blocker / "vis")                          # a path under a regular file: makedirs fails in the workers
    with pytest.raises(OSError):
        model.nondist_validation(_loader(), 1, None, True, True, True)
    assert model.net_g.training is True


def test_rejected_options(tmp_path):
    from refid_amd._lib import RefidHipError
    model = _model(tmp_path)
    with pytest.raises(RefidHipError, match="use_image"):
        model.nondist_validation(_loader(), 1, None, False, True, False)
    model.opt["val"]["metrics_interpo"]["psnr"]["crop_border"] = 4
    with pytest.raises(RefidHipError, match="crop_border"):
        model.nondist_validation(_loader(), 1, None, False, True, True)
    assert _files(tmp_path) == []
