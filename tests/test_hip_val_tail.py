"""GPU: the fused validation tail (refid_val_tail / refid_amd.metrics.val_tail) against what the reference's own
tensor2img, calculate_psnr and calculate_ssim returned for the same frames (tests/golden/val_tail.npz, written by
tools/make_val_golden.py): uint8 images bit for bit, the squared error as an exact integer, PSNR to 1e-9, SSIM to 2e-5
(the bar of tests/test_hip_io.py) and bit-equal to refid_ssim3d_u8, whose tile geometry and partial order it keeps.

Shapes (n_frames, H, W): (1,1,1) every tap replicate-padded; (3,17,35) partial tiles on both axes, W*3 = 105 not a
multiple of 4, odd row starts; (5,16,16) exactly one tile; (2,40,56) several tiles, 16-byte row segments.  The kernel
folds the frame index into grid x, so no case is needed for a grid-z limit; test_many_frames runs 70000 frames against
the oracle's restatement instead of a fixture (6.7 MB of inputs would not be one)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import refid_oracle as O

pytestmark = pytest.mark.gpu

CASES = ["1x1x1", "3x17x35", "5x16x16", "2x40x56"]
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "val_tail.npz"))


def _dev(z, case):
    return torch.from_numpy(z[f"{case}/pred"]).cuda(), torch.from_numpy(z[f"{case}/gt"]).cuda()


def _raw(pred, gt, flags=1, gt_u8=True, sq=True, ssim=True, shift=0):
    """The C entry itself.  The uint8 outputs lie `shift` bytes into buffers filled with a sentinel, 64 bytes of it
    either side.  Returns (pred_u8, gt_u8 | None, sq int64 | None, ssim sums float64 | None) on the host."""
    from refid_amd._lib import check, lib
    nf, _, h, w = pred.shape
    n = nf * h * w * 3
    bufs = [torch.full((n + 128 + shift,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    words = torch.zeros(2 * nf + lib().refid_val_tail_parts(nf, h, w), dtype=torch.int64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib().refid_val_tail(pred.data_ptr(), gt.data_ptr() if gt is not None else None, nf, h, w, flags,
                               bufs[0].data_ptr() + 64 + shift, bufs[1].data_ptr() + 64 + shift if gt_u8 else None,
                               words.data_ptr() if sq else None, words[nf:].data_ptr() if ssim else None,
                               words[2 * nf:].data_ptr(), st), "refid_val_tail")
    out = []
    for k, b in enumerate(bufs):
        b = b.cpu().numpy()
        if k == 0 or gt_u8:
            assert (b[:64 + shift] == SENTINEL).all() and (b[64 + shift + n:] == SENTINEL).all(), "wrote outside the image"
            out.append(b[64 + shift:64 + shift + n].reshape(nf, h, w, 3))
        else:
            assert (b == SENTINEL).all(), "gt_u8 written although not asked for"
            out.append(None)
    words = words.cpu()
    out.append(words[:nf].numpy() if sq else None)
    out.append(words[nf:2 * nf].view(torch.float64).numpy() if ssim else None)
    return out


@pytest.mark.parametrize("case", CASES)
def test_images_and_metrics_against_the_reference(z, case):
    from refid_amd.metrics import calculate_psnr_frames, val_tail
    pred, gt = _dev(z, case)
    ref_p, ref_g = z[f"{case}/pred_u8_bgr"], z[f"{case}/gt_u8_bgr"]
    tail = val_tail(pred, gt, bgr=True, want_gt_u8=True)
    assert tail.pred_u8.dtype == torch.uint8 and tuple(tail.pred_u8.shape) == ref_p.shape
    assert np.array_equal(tail.pred_u8.cpu().numpy(), ref_p) and np.array_equal(tail.gt_u8.cpu().numpy(), ref_g)
    rgb = val_tail(pred, gt, bgr=False)
    assert rgb.gt_u8 is None and np.array_equal(rgb.pred_u8.cpu().numpy(), ref_p[..., ::-1])
    old = calculate_psnr_frames(pred, gt)
    for f in range(pred.shape[0]):
        want_p, want_s = float(z[f"{case}/psnr"][f]), float(z[f"{case}/ssim"][f])
        print(case, f, "psnr", tail.psnr[f], want_p, "ssim", tail.ssim[f], want_s)
        if np.array_equal(ref_p[f], ref_g[f]):
            assert want_p == float("inf") and tail.psnr[f] == float("inf") and abs(tail.ssim[f] - 1.0) <= 1e-6
        else:
            assert abs(tail.psnr[f] - want_p) < 1e-9
            assert abs(tail.psnr[f] - old[f]) <= 1e-12 * abs(old[f])
        assert abs(tail.ssim[f] - want_s) < 2e-5
        assert rgb.psnr[f] == tail.psnr[f] and rgb.ssim[f] == tail.ssim[f]


@pytest.mark.parametrize("case", CASES)
def test_integer_squared_error_and_ssim_bits(z, case):
    from refid_amd._lib import check, lib
    pred, gt = _dev(z, case)
    nf, _, h, w = pred.shape
    a, b = z[f"{case}/pred_u8_bgr"].astype(np.int64), z[f"{case}/gt_u8_bgr"].astype(np.int64)
    want = ((a - b) ** 2).reshape(nf, -1).sum(axis=1)
    p8, g8, sq, ss = _raw(pred, gt)
    assert sq.dtype == np.int64 and np.array_equal(sq, want)
    buf = torch.empty(nf + lib().refid_ssim3d_u8_parts(nf, h, w), dtype=torch.float64, device="cuda")
    check(lib().refid_ssim3d_u8(pred.data_ptr(), gt.data_ptr(), nf, h, w, buf.data_ptr(), buf[nf:].data_ptr(),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), "refid_ssim3d_u8")
    assert np.array_equal(ss.view(np.int64), buf[:nf].cpu().numpy().view(np.int64))
    again = _raw(pred, gt)                                               # two runs: identical bits
    assert all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
               for x, y in zip((p8, g8, sq, ss), again))
    only_sq = _raw(pred, gt, gt_u8=False, ssim=False)                     # each output on its own (the halo-free kernel)
    assert only_sq[1] is None and only_sq[3] is None and np.array_equal(only_sq[0], p8) and np.array_equal(only_sq[2], want)
    only_ssim = _raw(pred, gt, gt_u8=False, sq=False)
    assert only_ssim[2] is None and np.array_equal(only_ssim[3].view(np.int64), ss.view(np.int64))


@pytest.mark.parametrize("case", ["3x17x35", "2x40x56"])
@pytest.mark.parametrize("shift", [1, 2, 3, 16])
def test_unaligned_images_stay_inside_their_rows(z, case, shift):
    """Row heads and tails: the image starts `shift` bytes off a 16-byte boundary (with W*3 = 105 every row start moves too)."""
    pred, gt = _dev(z, case)
    for flags in (0, 1):
        p8, g8, _, _ = _raw(pred, gt, flags=flags, shift=shift, ssim=(flags == 1))
        sel = slice(None) if flags else slice(None, None, -1)
        assert np.array_equal(p8, z[f"{case}/pred_u8_bgr"][..., sel]) and np.array_equal(g8, z[f"{case}/gt_u8_bgr"][..., sel])


def test_null_gt_converts_only(z):
    from refid_amd._lib import RefidHipError
    from refid_amd.metrics import val_tail
    pred, gt = _dev(z, "3x17x35")
    p8, g8, sq, ss = _raw(pred, None, gt_u8=False, sq=False, ssim=False)
    assert np.array_equal(p8, z["3x17x35/pred_u8_bgr"])
    tail = val_tail(pred.view(1, 3, 3, 17, 35))
    assert tail.gt_u8 is None and tail.psnr is None and tail.ssim is None
    assert tuple(tail.pred_u8.shape) == (1, 3, 17, 35, 3) and np.array_equal(tail.pred_u8[0].cpu().numpy(), p8)
    with pytest.raises(RefidHipError, match="need gt"):
        _raw(pred, None, gt_u8=False, sq=True, ssim=False)
    with pytest.raises(RefidHipError, match="flags"):
        _raw(pred, gt, flags=6)


def test_frames_do_not_depend_on_their_position(z):
    pred, gt = _dev(z, "5x16x16")
    whole = _raw(pred, gt)
    for order in ([3], [1, 3, 0], [4, 4, 2, 1, 0, 3, 2]):
        part = _raw(pred[order].contiguous(), gt[order].contiguous())
        for x, y in zip(whole, part):
            assert np.array_equal(x[order].view(np.uint8), y.view(np.uint8))


def test_many_frames():
    """More frames than a grid's y / z extent (65535): the frame index is folded into x."""
    nf = 70000
    g = torch.Generator(device="cuda").manual_seed(5)
    pred = torch.rand((nf, 3, 2, 2), device="cuda", generator=g) * 1.4 - 0.2
    gt = torch.rand((nf, 3, 2, 2), device="cuda", generator=g) * 1.4 - 0.2
    qa, qb = O.tensor2img_u8(pred), O.tensor2img_u8(gt)
    from refid_amd._lib import lib
    from refid_amd.metrics import val_tail
    tail = val_tail(pred, gt, bgr=False, want_gt_u8=True, ssim=False)
    assert torch.equal(tail.pred_u8, qa.permute(0, 2, 3, 1)) and torch.equal(tail.gt_u8, qb.permute(0, 2, 3, 1))
    sq = ((qa.long() - qb.long()) ** 2).sum(dim=(1, 2, 3)).tolist()
    from refid_amd.metrics import psnr_from_sqerr
    assert tail.psnr == [psnr_from_sqerr(v, 12) for v in sq]
    assert lib().refid_val_tail_parts(nf, 2, 2) == 2 * nf
