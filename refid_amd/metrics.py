"""Validation tail on the GPU: tensor2img quantisation + calculate_psnr.

Reference: basicsr/utils/img_util.py:90-117 (clamp to [0,1], x255, round -> uint8; the RGB->BGR
flip is PSNR-invariant) and basicsr/metrics/psnr_ssim.py:48-63 (float64 MSE over H x W x 3,
20*log10(255/sqrt(mse)), inf when identical).  One fused kernel + a fixed-order finish (deterministic, no atomics),
no host round trip per frame."""
import collections
import ctypes as C
import math

import torch

from ._lib import VAL_TAIL_BGR, RefidHipError, check, lib


def calculate_psnr_frames(pred, gt):
    """pred, gt: (..., 3, H, W) float32 CUDA tensors in [0,1] range; returns a list of per-frame PSNRs."""
    if pred.shape != gt.shape or pred.dim() < 3:
        raise AssertionError(f"Image shapes are differnet: {tuple(pred.shape)}, {tuple(gt.shape)}.")
    if not (pred.is_cuda and gt.is_cuda) or pred.dtype != torch.float32 or gt.dtype != torch.float32:
        raise RefidHipError("calculate_psnr_frames: float32 CUDA tensors required")
    pred, gt = pred.contiguous(), gt.contiguous()
    fe = pred.shape[-1] * pred.shape[-2] * pred.shape[-3]
    nf = pred.numel() // fe
    buf = torch.empty(nf + lib().refid_sqerr_u8_parts(nf, fe), dtype=torch.float64, device=pred.device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib().refid_sqerr_u8(pred.data_ptr(), gt.data_ptr(), nf, fe, buf.data_ptr(), buf[nf:].data_ptr(), st), "refid_sqerr_u8")
    out = []
    for v in buf[:nf].tolist():                         # one device->host copy for all frames
        mse = v / fe
        out.append(float("inf") if mse == 0 else 20.0 * math.log10(255.0 / math.sqrt(mse)))
    return out


def calculate_ssim_frames(pred, gt):
    """The reference's calculate_ssim (3-D Gaussian variant, metrics/psnr_ssim.py:135-182,225-303) on the
    uint8-quantised frames; pred, gt: (..., 3, H, W) float32 CUDA tensors.  Per-frame list."""
    if pred.shape != gt.shape or pred.dim() < 3 or pred.shape[-3] != 3:
        raise AssertionError(f"Image shapes are differnet: {tuple(pred.shape)}, {tuple(gt.shape)}.")
    if not (pred.is_cuda and gt.is_cuda) or pred.dtype != torch.float32 or gt.dtype != torch.float32:
        raise RefidHipError("calculate_ssim_frames: float32 CUDA tensors required")
    pred, gt = pred.contiguous(), gt.contiguous()
    h, w = pred.shape[-2], pred.shape[-1]
    nf = pred.numel() // (3 * h * w)
    buf = torch.empty(nf + lib().refid_ssim3d_u8_parts(nf, h, w), dtype=torch.float64, device=pred.device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib().refid_ssim3d_u8(pred.data_ptr(), gt.data_ptr(), nf, h, w, buf.data_ptr(), buf[nf:].data_ptr(), st), "refid_ssim3d_u8")
    return [v / (3 * h * w) for v in buf[:nf].tolist()]


def split_deblur_interp(psnrs, m, n):
    """Mean PSNR over 'interpolation' frames (index in [m, m+n)) and the rest ('deblur'), as the
    reference's validation does (twoImage_event_recurrent_model.py:426-507).  psnrs: per-frame list of
    ONE sample (T = 2m+n frames)."""
    interp = [p for i, p in enumerate(psnrs) if m <= i < m + n]
    deblur = [p for i, p in enumerate(psnrs) if not (m <= i < m + n)]
    mean = lambda xs: sum(xs) / len(xs) if xs else float("nan")     # noqa: E731
    return mean(deblur), mean(interp)


ValTail = collections.namedtuple("ValTail", "pred_u8 gt_u8 psnr ssim")


def val_tail(pred, gt=None, *, bgr=True, want_gt_u8=False, psnr=True, ssim=True):
    """One launch for everything the reference's validation loop does to an item's frames after ``test()``
    (twoImage_event_recurrent_model.py:412-432, :460-491): tensor2img of ``pred`` (and of ``gt`` when ``want_gt_u8``) into
    uint8 (..., H, W, 3) device tensors -- BGR as tensor2img returns them, or RGB for a PNG -- and, with ``gt``, the
    per-frame calculate_psnr / calculate_ssim lists.  pred, gt: (..., 3, H, W) float32 CUDA tensors.  The PSNR numerator
    is an exact integer sum; all scalars of the call come back in one device->host copy.  Returns
    ValTail(pred_u8, gt_u8 | None, psnr list | None, ssim list | None)."""
    if pred.dim() < 3 or pred.shape[-3] != 3 or (gt is not None and gt.shape != pred.shape):
        raise AssertionError(f"Image shapes are differnet: {tuple(pred.shape)}, {None if gt is None else tuple(gt.shape)}.")
    if not pred.is_cuda or pred.dtype != torch.float32 or (gt is not None and (not gt.is_cuda or gt.dtype != torch.float32)):
        raise RefidHipError("val_tail: float32 CUDA tensors required")
    pred = pred.contiguous()
    gt = gt.contiguous() if gt is not None else None
    h, w = pred.shape[-2], pred.shape[-1]
    nf = pred.numel() // (3 * h * w)
    psnr, ssim, want_gt_u8 = (bool(v) and gt is not None for v in (psnr, ssim, want_gt_u8))
    shape = tuple(pred.shape[:-3]) + (h, w, 3)
    pred_u8 = torch.empty(shape, dtype=torch.uint8, device=pred.device)
    gt_u8 = torch.empty(shape, dtype=torch.uint8, device=pred.device) if want_gt_u8 else None
    # one buffer of 8-byte words: [nf] integer squared errors | [nf] SSIM sums (float64 bits) | the kernel's partials
    buf = torch.empty(2 * nf + lib().refid_val_tail_parts(nf, h, w), dtype=torch.int64, device=pred.device) \
        if (psnr or ssim) else None
    ptr = lambda t, on=True: t.data_ptr() if (t is not None and on) else None      # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib().refid_val_tail(pred.data_ptr(), ptr(gt), nf, h, w, VAL_TAIL_BGR if bgr else 0, pred_u8.data_ptr(),
                               ptr(gt_u8), ptr(buf, psnr), ptr(buf[nf:] if buf is not None else None, ssim),
                               ptr(buf[2 * nf:] if buf is not None else None), st), "refid_val_tail")
    psnrs = ssims = None
    if buf is not None:
        host = buf[:2 * nf].cpu()                           # the one device->host copy of the call
        if psnr:
            psnrs = [psnr_from_sqerr(v, 3 * h * w) for v in host[:nf].tolist()]
        if ssim:
            ssims = [v / (3 * h * w) for v in host[nf:].view(torch.float64).tolist()]
    return ValTail(pred_u8, gt_u8, psnrs, ssims)


def psnr_from_sqerr(sq, count):
    """calculate_psnr's last three lines (metrics/psnr_ssim.py:59-63) from the summed squared error of uint8 images."""
    mse = sq / count
    return float("inf") if mse == 0 else 20.0 * math.log10(255.0 / math.sqrt(mse))


METRIC_TYPES = ("calculate_psnr", "calculate_ssim")


def check_metric_options(val_opt, use_image=True, groups=("metrics_deblur", "metrics_interpo")):
    """What nondist_validation here supports of opt['val'] (no shipped YAML asks for more); names the offending key."""
    if not use_image:
        raise RefidHipError("use_image=False is not supported (the reference's branch feeds 5-D tensors to reorder_image "
                            "and cannot run)")
    for group in groups:
        for name, o in (val_opt.get(group) or {}).items():
            where = f"val.{group}.{name}"
            if o.get("type") not in METRIC_TYPES:
                raise RefidHipError(f"{where}.type {o.get('type')!r} is not supported (supported: {METRIC_TYPES})")
            if o.get("crop_border", 0) != 0:
                raise RefidHipError(f"{where}.crop_border {o['crop_border']!r} is not supported (only 0)")
            if o.get("test_y_channel", False):
                raise RefidHipError(f"{where}.test_y_channel is not supported")


class ValidationMetrics:
    """nondist_validation's bookkeeping (twoImage_event_recurrent_model.py:362-379, :460-512) and its three log lines
    (_log_validation_metric_values :515-536), without any GPU dependency.  A frame of a T = 2m+n item is an
    *interpolation* frame iff m <= idx < m+n, else a *deblur* frame; ``add_item`` takes the per-frame metric lists of one
    sample, ``finish`` divides by cnt*2m and cnt*n, forms total = (deblur*2m + interp*n)/(2m+n) per deblur metric name
    and returns the reference's `current_metric` (the last metric assigned: last interpolation one in dict order, else
    the last deblur one, else 0.)."""

    def __init__(self, metrics_deblur, metrics_interpo, m, n):
        self.opt_deblur = metrics_deblur
        self.with_metrics = metrics_deblur is not None
        self.opt_interpo = (metrics_interpo or {}) if self.with_metrics else {}
        self.m, self.n = m, n
        self.cnt = 0
        self.deblur = {k: 0 for k in (metrics_deblur or {})}
        self.interpo = {k: 0 for k in self.opt_interpo}
        self.total = {k: 0 for k in self.deblur}

    def metric_types(self):
        """The metric functions in use: what the loop asks metrics.val_tail for."""
        if not self.with_metrics:
            return set()
        return {o["type"] for o in list(self.opt_deblur.values()) + list(self.opt_interpo.values())}

    def add_item(self, per_frame):
        """per_frame: {'calculate_psnr': [T values], 'calculate_ssim': [T values]} of ONE sample (only the types in use)."""
        self.cnt += 1
        if not self.with_metrics:
            return
        frames = len(next(iter(per_frame.values()))) if per_frame else 0
        for idx in range(frames):
            interp = self.m <= idx < self.m + self.n
            dst, opts = (self.interpo, self.opt_interpo) if interp else (self.deblur, self.opt_deblur)
            for name, o in opts.items():
                dst[name] += per_frame[o["type"]][idx]

    def finish(self):
        current = 0.
        if self.with_metrics:
            for k in self.deblur:
                self.deblur[k] /= (self.cnt * 2 * self.m)
                current = self.deblur[k]
            for k in self.interpo:
                self.interpo[k] /= (self.cnt * self.n)
                current = self.interpo[k]
            for k in self.total:
                if k not in self.interpo:                  # (the reference raises KeyError here; no shipped YAML does this)
                    self.total[k] = self.deblur[k]
                    continue
                self.total[k] = self.deblur[k] * 2 * self.m + self.interpo[k] * self.n
                self.total[k] /= 2 * self.m + self.n
        return current

    def log_lines(self, dataset_name):
        """The three strings the reference logs, [total] / [deblur] / [interpolation], after ``finish``."""
        out = []
        for tag, res in (("total", self.total), ("deblur", self.deblur), ("interpolation", self.interpo)):
            s = f"Validation {dataset_name} [{tag}],\t"
            for k, v in res.items():
                s += f"\t # {k}: {v:.4f}"
            out.append(s)
        return out


class InterpolationMetrics:
    """The sharp models' bookkeeping (Test_twoSharpImage_event_recurrent_model.py:364-370, :453-502), without any GPU
    dependency: every frame of an item is an interpolation frame; ``finish`` divides the sums by cnt * T (T: the frame
    count of the last item, the reference's `imgs_per_iter`) and returns the last metric in dict order (0. without
    metrics); one log line.  Same interface as ``ValidationMetrics``."""

    def __init__(self, metrics_interpo):
        self.opt_interpo = metrics_interpo
        self.with_metrics = metrics_interpo is not None
        self.cnt = 0
        self.frames = 0
        self.interpo = {k: 0 for k in (metrics_interpo or {})}

    def metric_types(self):
        return {o["type"] for o in self.opt_interpo.values()} if self.with_metrics else set()

    def add_item(self, per_frame):
        self.cnt += 1
        if not self.with_metrics:
            return
        self.frames = len(next(iter(per_frame.values()))) if per_frame else 0
        for idx in range(self.frames):
            for name, o in self.opt_interpo.items():
                self.interpo[name] += per_frame[o["type"]][idx]

    def finish(self):
        current = 0.
        if self.with_metrics:
            for k in self.interpo:
                self.interpo[k] /= (self.cnt * self.frames)
                current = self.interpo[k]
        return current

    def log_lines(self, dataset_name):
        s = f"Validation {dataset_name} [interpolation],\t"
        for k, v in self.interpo.items():
            s += f"\t # {k}: {v:.4f}"
        return [s]


class SingleImageMetrics:
    """The single-image model's bookkeeping (image_event_restoration_model.py:377-382, :457-484) and its one log line
    (_log_validation_metric_values, :487-496), without any GPU dependency: one ``val.metrics`` dict, one sum per metric
    name over the items (an item is one frame), ``finish`` divides by the item count and returns the last metric in dict
    order (0. without metrics).  Same interface as ``ValidationMetrics``."""

    def __init__(self, val_metrics):
        self.opt_metrics = val_metrics
        self.with_metrics = val_metrics is not None
        self.cnt = 0
        self.results = {k: 0 for k in (val_metrics or {})}

    def metric_types(self):
        return {o["type"] for o in self.opt_metrics.values()} if self.with_metrics else set()

    def add_item(self, per_frame):
        """per_frame: {'calculate_psnr': [value], 'calculate_ssim': [value]} of ONE sample (only the types in use)."""
        self.cnt += 1
        if not self.with_metrics:
            return
        for name, o in self.opt_metrics.items():
            for v in per_frame[o["type"]]:
                self.results[name] += v

    def finish(self):
        current = 0.
        if self.with_metrics:
            for k in self.results:
                self.results[k] /= self.cnt
                current = self.results[k]
        return current

    def log_lines(self, dataset_name):
        s = f"Validation {dataset_name},\t"
        for k, v in self.results.items():
            s += f"\t # {k}: {v:.4f}"
        return [s]
