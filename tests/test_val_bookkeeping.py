"""CPU-only: the validation loop's bookkeeping (refid_amd.metrics.ValidationMetrics) against values aggregated from the
reference's own per-frame PSNR / SSIM (tests/golden/val_tail.npz, tools/make_val_golden.py), its log lines, its return
value and the options it rejects."""
import math
import os

import numpy as np
import pytest

from refid_amd._lib import RefidHipError
from refid_amd.metrics import ValidationMetrics, check_metric_options, psnr_from_sqerr

PSNR, SSIM = dict(type="calculate_psnr", crop_border=0, test_y_channel=False), dict(type="calculate_ssim", crop_border=0,
                                                                                  test_y_channel=False)
BOTH = dict(psnr=PSNR, ssim=SSIM)


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "val_tail.npz"))


def _run(z, deblur=BOTH, interpo=BOTH):
    m, n = (int(v) for v in z["book/mn"])
    book = ValidationMetrics(deblur, interpo, m, n)
    for frames in z["book/frames"]:
        book.add_item({"calculate_psnr": [float(z["5x16x16/psnr"][f]) for f in frames],
                       "calculate_ssim": [float(z["5x16x16/ssim"][f]) for f in frames]})
    return book, book.finish()


def test_aggregates_equal_the_reference_formulas(z):
    book, ret = _run(z)
    for got, want in ((book.deblur, z["book/deblur"]), (book.interpo, z["book/interpo"]), (book.total, z["book/total"])):
        assert list(got) == ["psnr", "ssim"]
        assert abs(got["psnr"] - want[0]) <= 1e-12 and abs(got["ssim"] - want[1]) <= 1e-12
    assert ret == book.interpo["ssim"]                                   # the last metric assigned


def test_log_lines(z):
    book, _ = _run(z)
    d, i, t = z["book/deblur"], z["book/interpo"], z["book/total"]
    assert book.log_lines("GoPro-test") == [
        f"Validation GoPro-test [total],\t\t # psnr: {t[0]:.4f}\t # ssim: {t[1]:.4f}",
        f"Validation GoPro-test [deblur],\t\t # psnr: {d[0]:.4f}\t # ssim: {d[1]:.4f}",
        f"Validation GoPro-test [interpolation],\t\t # psnr: {i[0]:.4f}\t # ssim: {i[1]:.4f}"]


def test_return_value_rule(z):
    book, ret = _run(z, interpo={})
    assert ret == book.deblur["ssim"] and book.interpo == {} and book.total == book.deblur
    book, ret = _run(z, deblur=dict(ssim=SSIM, psnr=PSNR), interpo=dict(psnr=PSNR))
    assert ret == book.interpo["psnr"] and list(book.deblur) == ["ssim", "psnr"]
    book, ret = _run(z, deblur=None, interpo=None)                       # no metrics_deblur: with_metrics is False
    assert ret == 0. and book.cnt == 3
    assert ValidationMetrics({}, {}, 1, 3).finish() == 0.


def test_divisors_are_items_times_frames():
    book = ValidationMetrics(dict(psnr=PSNR), dict(psnr=PSNR), 2, 1)     # T = 5: deblur 0 1 3 4, interpolation 2
    book.add_item({"calculate_psnr": [1., 2., 100., 3., 4.]})
    book.add_item({"calculate_psnr": [5., 6., 200., 7., 8.]})
    book.finish()
    assert book.deblur["psnr"] == 36. / 8 and book.interpo["psnr"] == 300. / 2
    assert book.total["psnr"] == (4.5 * 4 + 150. * 1) / 5


def test_inf_propagates():
    assert psnr_from_sqerr(0, 48) == float("inf") and psnr_from_sqerr(48, 48) == 20.0 * math.log10(255.0)
    book = ValidationMetrics(dict(psnr=PSNR), dict(psnr=PSNR), 1, 1)
    book.add_item({"calculate_psnr": [30., float("inf"), 31.]})
    ret = book.finish()
    assert book.deblur["psnr"] == 30.5 and ret == float("inf") and book.total["psnr"] == float("inf")
    assert book.log_lines("x")[2].endswith("# psnr: inf")


@pytest.mark.parametrize("val, use_image, key", [
    (dict(metrics_deblur=dict(psnr=dict(type="calculate_psnr", crop_border=2))), True, "crop_border"),
    (dict(metrics_deblur=BOTH, metrics_interpo=dict(ssim=dict(type="calculate_ssim", test_y_channel=True))), True,
     "test_y_channel"),
    (dict(metrics_deblur=dict(niqe=dict(type="calculate_niqe"))), True, "metrics_deblur.niqe.type"),
    (dict(metrics_deblur=BOTH), False, "use_image"),
])
def test_rejected_options_name_their_key(val, use_image, key):
    with pytest.raises(RefidHipError, match=key):
        check_metric_options(val, use_image)


def test_shipped_style_options_pass():
    check_metric_options(dict(metrics_deblur=BOTH, metrics_interpo=BOTH, save_img=True, save_gt=True), True)
    check_metric_options({}, True)
