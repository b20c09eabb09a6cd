"""The event-based double integral (EDI, Pan et al., CVPR 2019): deblurring and interpolation without a network, on the
GPU (csrc/edi.hip; the contract is "Double integral" in include/refid_hip.h, tests/edi_ref.py restates it).

A pixel's log level moves by ``+c_pos`` or ``-c_neg`` per event, so the latent frame at an instant is the blurry key frame
times ``exp(level)``, divided by the mean of ``exp(level)`` over the key's exposure: the model-based inverse of what
``event_sim`` and ``blur_synth`` compute.  It needs no weights, reads the same resident frames and events as the
network runners and writes the same uint8 frames into the same sinks (PNG, Motion-JPEG, NIQE, ``gt`` scores), so it is
the baseline row next to a network's, and a check of a stream's conventions -- polarity, x / y order, the time unit --
before a network is blamed: a stream that is flipped or shifted scores below its own blurry key frames.

Not modelled: per-pixel threshold maps, estimating the thresholds from the data, a camera response for coded frames,
joint solves over many keys, event denoising.  There is no host fallback."""
import collections
import os

import numpy as np
import torch

from . import _lib, sequence
from ._lib import RefidHipError
from .event_sim import to_fixed

EXPOSURES = ("samples", "continuous")
EdiPair = collections.namedtuple("EdiPair", "left right row0 row1 first_stamp last_stamp left_end right_start")


def gain_tables():
    """float64 [577]: exp(i), i = -32 .. 32 | exp(h / 256), h = 0 .. 255 | exp(l / 65536), l = 0 .. 255; the gain of a level
    e = 65536 i + 256 h + l (units of 2^-16) is the product of one entry of each; over every level inside +-32 it lies at most 3 ulp from ``numpy.exp(e / 65536)``
    (tests/test_edi_ref_host.py measures all 4 194 305 of them)."""
    c = _lib.EDI_CLAMP
    return np.concatenate([np.exp(np.arange(-c, c + 1, dtype=np.float64)), np.exp(np.arange(256, dtype=np.float64) / 256.0),
                           np.exp(np.arange(256, dtype=np.float64) / 65536.0)])


_TABLES = {}


def device_tables(device):
    """``gain_tables()`` on ``device``, uploaded once per device."""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(gain_tables()).to(device)
    return _TABLES[key]


def sample_instants(s, e, m):
    """float32 [m]: where the ``m`` frames averaged into a key frame with exposure [s, e] were taken, equally spaced:
    fl32(s + ((e - s) j) / (m - 1)) in float64 from the float32 bounds, held inside [s, e]; m = 1: s."""
    s, e = np.float32(s), np.float32(e)
    if m == 1:
        return np.array([s], dtype=np.float32)
    part = (np.float64(e) - np.float64(s)) * np.arange(m, dtype=np.float64) / np.float64(m - 1)
    return np.clip((np.float64(s) + part).astype(np.float32), s, e)


def output_instants(layout, bounds, m=1, n=None):
    """float32 (T,): the instants the network's outputs stand for, from bounds (s0, e0, s1, e1).  'sharp': s0 + (s1 - s0)
    (f + 1) / (n + 1), f < n; 'blur': s0 + (e1 - s0) f / (2m + n - 1), f < 2m + n; 'single': (s0 + e0) / 2.  float64 from the
    float32 bounds, rounded to float32 and held inside the bounds."""
    s0, e0, s1, e1 = (np.float64(np.float32(v)) for v in bounds)
    if layout == "single":
        return np.array([(s0 + e0) / 2.0], dtype=np.float64).astype(np.float32)
    if layout == "sharp":
        part = (s1 - s0) * np.arange(1, n + 1, dtype=np.float64) / np.float64(n + 1)
        return np.clip((s0 + part).astype(np.float32), np.float32(s0), np.float32(s1))
    if layout != "blur":
        raise RefidHipError(f"output_instants: unknown layout {layout!r} ('blur', 'sharp' or 'single')")
    part = (e1 - s0) * np.arange(2 * m + n, dtype=np.float64) / np.float64(2 * m + n - 1)
    return np.clip((s0 + part).astype(np.float32), np.float32(s0), np.float32(e1))


def exposure_pairs(starts, ends):
    """[EdiPair] of blurry key frames with exposures [starts[k], ends[k]]: pair k is (k, k + 1) with all four bounds.  The
    first six fields are those of ``sequence.make_pairs(..., stamps='bounds')`` (the event-row windows are not used here
    and stay 0)."""
    s, e = np.asarray(starts, dtype=np.float32).reshape(-1), np.asarray(ends, dtype=np.float32).reshape(-1)
    if s.shape != e.shape:
        raise RefidHipError(f"exposure_pairs: {s.size} exposure starts, {e.size} exposure ends")
    return [EdiPair(k, k + 1, 0, 0, float(s[k]), float(e[k + 1]), float(e[k]), float(s[k + 1])) for k in range(len(s) - 1)]


class EdiStream:
    """The resident stream of one sequence, sorted by pixel: what every ``ops.edi`` launch of the sequence reads.
    ``load`` packs it once with torch operations on the device (a stable sort of the time-sorted rows by pixel, the
    segment starts by ``searchsorted`` on the sorted pixels, the stamps and signs gathered) and does not synchronise;
    ``dropped`` and ``unsorted`` read their counters, one synchronisation each, when they are first asked for."""

    def __init__(self, device=None):
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise RefidHipError("EdiStream: a GPU device is required (csrc/edi.hip has no host fallback)")
        self.t = self.p = self.seg = self.height = self.width = None
        self.n_events = 0
        self._dropped = self._unsorted = None

    def load(self, events, height, width):
        """``events``: float32 (E, 4) rows [t, x, y, p] sorted by time, host or device; x and y are truncated toward zero,
        rows outside the (height, width) frame are dropped and counted, p > 0 is positive, anything else negative."""
        ev = torch.as_tensor(events) if not torch.is_tensor(events) else events
        if ev.dtype != torch.float32 or ev.dim() != 2 or ev.shape[1] != 4:
            raise RefidHipError(f"EdiStream.load: events must be float32 (E, 4) rows [t, x, y, p], got {ev.dtype} {tuple(ev.shape)}")
        height, width = int(height), int(width)
        if height < 1 or width < 1 or height * width > _lib.EDI_MAX_PIXELS:
            raise RefidHipError(f"EdiStream.load: height {height} * width {width} must be 1 .. {_lib.EDI_MAX_PIXELS} pixels")
        if ev.shape[0] >= 2 ** 31:
            raise RefidHipError(f"EdiStream.load: {ev.shape[0]} rows, 2^31 - 1 are the most of one stream")
        ev = ev.to(self.device, non_blocking=True)
        hw = height * width
        x, y = torch.trunc(ev[:, 1]), torch.trunc(ev[:, 2])
        inside = (x >= 0) & (x < width) & (y >= 0) & (y < height)                  # (a NaN coordinate compares false)
        zero = torch.zeros_like(x)
        pix = torch.where(inside, torch.where(inside, y, zero).long() * width + torch.where(inside, x, zero).long(),
                          torch.full((), hw, dtype=torch.int64, device=self.device))      # dropped rows: behind the last pixel
        pix, order = torch.sort(pix, stable=True)
        self.t = ev[:, 0][order].contiguous()
        self.p = torch.where(ev[:, 3][order] > 0, 1, -1).to(torch.int8)
        self.seg = torch.searchsorted(pix, torch.arange(hw + 1, dtype=torch.int64, device=self.device)).to(torch.int32)
        self.n_events, self.height, self.width = int(ev.shape[0]), height, width
        self._dropped = (~inside).sum()
        self._unsorted = (ev[1:, 0] < ev[:-1, 0]).sum()
        return self

    @property
    def dropped(self):
        """Rows outside the frame (synchronises)."""
        return int(self._dropped)

    @property
    def unsorted(self):
        """Rows whose stamp lies before their predecessor's; the stream must be sorted by time, so anything but 0 means the
        outputs are not the model's (synchronises)."""
        return int(self._unsorted)


class _Resident:
    """What the sinks of ``sequence`` read of a runner's ``assembler``."""

    def __init__(self, layout):
        self.layout, self.frames, self.bgr, self.height, self.width = layout, None, False, None, None


class _EdiRunner(sequence._SequenceRunner):
    """What ``EdiInterpolator`` and ``EdiDeblurrer`` share: ``_SequenceRunner.run`` with the network's minibatch replaced by
    one ``ops.edi`` launch.  ``clamped`` (pixels of items whose gain was held at exp(+-32): a hot pixel, or thresholds far
    too large) and ``dropped`` (event rows outside the frame) are set after ``run``.

    The stream must be sorted by time.  That is checked on the device and read, with the two counters, only after the last
    minibatch, so that the loop holds no synchronisation: a stream that is not sorted makes ``run`` raise RefidHipError AFTER
    every frame has been handed to the sinks -- the files of ``out_dir`` and ``video`` are then written and are not the model's,
    and ``scores`` / ``niqe_scores`` stay None.  Sort first (``events[np.argsort(events[:, 0], kind='stable')]``)."""

    clamped = dropped = None

    def __init__(self, m, n, layout, c_pos, c_neg, exposure, eps, max_minibatch, device):
        what = type(self).__name__
        if exposure not in EXPOSURES:
            raise RefidHipError(f"{what}: unknown exposure {exposure!r} ('samples' or 'continuous')")
        self.m, self.n, self.exposure, self.eps = int(m), (None if n is None else int(n)), exposure, float(eps)
        if not 1 <= self.m <= _lib.BLUR_MAX_COUNT:
            raise RefidHipError(f"{what}: m {m} must be 1 .. {_lib.BLUR_MAX_COUNT}")
        if layout != "single" and (self.n is None or self.n < (1 if layout == "sharp" else 0)):
            raise RefidHipError(f"{what}: n {n} must be at least {1 if layout == 'sharp' else 0} for layout {layout!r}")
        count = 1 if layout == "single" else self.n if layout == "sharp" else 2 * self.m + self.n
        if count > _lib.EDI_MAX_INSTANTS:
            raise RefidHipError(f"{what}: {count} output frames per item, {_lib.EDI_MAX_INSTANTS} are the most")
        self.c_pos, self.c_neg = (self._threshold(what, name, c) for name, c in (("c_pos", c_pos), ("c_neg", c_neg)))
        if not (np.isfinite(self.eps) and self.eps >= 0.0):
            raise RefidHipError(f"{what}: eps {eps} must be finite and not negative")
        self.max_minibatch = int(max_minibatch)
        if self.max_minibatch < 1:
            raise RefidHipError(f"{what}: max_minibatch {max_minibatch} must be >= 1")
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise RefidHipError(f"{what}: a GPU device is required (csrc/edi.hip has no host fallback)")
        self.assembler, self.events = _Resident(layout), EdiStream(self.device)

    @staticmethod
    def _threshold(what, name, c):
        c = float(c)
        if not np.isfinite(c) or not 1 <= to_fixed(c) <= _lib.EDI_MAX_THRESHOLD:
            raise RefidHipError(f"{what}: {name} {c} must be at least 2^-16 and at most {_lib.EDI_MAX_THRESHOLD >> 16}")
        return to_fixed(c)

    def _load(self, frames, events, bgr):
        what, res = type(self).__name__, self.assembler
        frames = torch.as_tensor(frames) if not torch.is_tensor(frames) else frames
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
            raise RefidHipError(f"{what}.run: frames must be uint8 (N, H, W, 3), got {frames.dtype} {tuple(frames.shape)}")
        frames = frames.to(self.device, non_blocking=True)
        res.frames = (frames.flip(-1) if bgr else frames).contiguous()          # (resident as RGB: the outputs are RGB)
        res.height, res.width = int(frames.shape[1]), int(frames.shape[2])
        self.events.load(events, res.height, res.width)

    def _bounds(self, p):
        """(s0, e0, s1, e1) of an item: an ``EdiPair`` carries all four; a ``Pair`` of ``make_pairs(..., stamps='bounds')``
        carries the outer two, which are all a sharp pair or a single frame has."""
        layout = self.assembler.layout
        if len(p) >= 8:
            return p[4], p[6], p[7], p[5]
        if layout == "single":
            return p[4], p[5], p[5], p[5]
        if layout == "sharp":
            return p[4], p[4], p[5], p[5]
        raise RefidHipError(f"{type(self).__name__}.run: blurry pairs need all four exposure bounds: build them with edi.exposure_pairs")

    def _outputs(self, chunks):
        from . import ops
        res, layout = self.assembler, self.assembler.layout
        self.clamped = self.dropped = None
        counts = []
        for chunk in chunks:
            bounds = np.array([self._bounds(p) for p in chunk], dtype=np.float32)
            items = np.array([[p[0], -1 if layout == "single" else p[1]] for p in chunk], dtype=np.int64)
            instants = np.stack([output_instants(layout, b, self.m, self.n) for b in bounds])
            u8, held = ops.edi(res.frames, self.events, items, bounds, instants, m=self.m, exposure=self.exposure, c_pos=self.c_pos,
                               c_neg=self.c_neg, eps=self.eps)
            counts.append(held.sum())
            yield u8[:, 0] if layout == "single" else u8
        self.clamped = int(torch.stack(counts).sum())           # read after the loop, with the stream's counters
        self.dropped = self.events.dropped
        if self.events.unsorted:
            raise RefidHipError(f"{type(self).__name__}.run: {self.events.unsorted} event rows lie before their predecessor in time: sort "
                                "the stream by time first")


class EdiInterpolator(_EdiRunner):
    """``SequenceInterpolator`` without a network: the frames between (sharp layout) or inside and between (blur layout) two
    key frames by the double integral, at the instants the network's outputs stand for (``output_instants``).  ``c_pos`` /
    ``c_neg``: the stream's contrast thresholds in natural-log units (what ``simulate`` was given); ``exposure``: 'samples'
    -- a blurry key frame is the mean of ``m`` frames, what ``simulate --blur m`` writes -- or 'continuous', a real
    shutter; ``eps``: the simulator's offset of the log.  ``run`` has ``SequenceInterpolator.run``'s arguments, file names
    and results; blurry pairs come from ``exposure_pairs``, sharp ones from ``make_pairs(..., stamps='bounds')``."""

    def __init__(self, m, n, layout="sharp", c_pos=0.2, c_neg=0.2, exposure="samples", eps=1e-3, max_minibatch=2, device=None):
        if layout not in ("blur", "sharp"):
            raise RefidHipError(f"EdiInterpolator: unknown layout {layout!r} ('blur' or 'sharp')")
        super().__init__(1 if layout == "sharp" else m, n, layout, c_pos, c_neg, exposure, eps, max_minibatch, device)

    def run(self, frames, events, pairs, out_dir=None, names=None, keep=False, bgr=False, niqe=None, png_filter="none",
            png_deflate="host", gt=None, score=None, video=None, video_fps=30, video_quality=90, video_subsampling="420",
            video_keys=None, jpeg_pitch=None):
        """As ``SequenceInterpolator.run``: the same arguments, file names, ``niqe_scores``, ``scores`` and ``video_paths``.  An
        unsorted stream raises only after the frames were written (see ``_EdiRunner``)."""
        return sequence._SequenceRunner.run(self, frames, events, pairs, out_dir=out_dir, names=names, keep=keep, bgr=bgr, niqe=niqe,
                                            png_filter=png_filter, png_deflate=png_deflate, gt=gt, score=score, video=video,
                                            video_fps=video_fps, video_quality=video_quality, video_subsampling=video_subsampling,
                                            video_keys=video_keys, jpeg_pitch=jpeg_pitch)

    _paths = sequence.SequenceInterpolator._paths


class EdiDeblurrer(_EdiRunner):
    """``SequenceDeblurrer`` without a network: every blurry frame at the middle of its exposure.  ``m``: the frames averaged
    into a blurry frame ('samples' exposure).  ``run`` has ``SequenceDeblurrer.run``'s arguments, file names and results;
    items come from ``make_pairs(t, *frame_windows(starts, ends), stamps='bounds')``."""

    def __init__(self, m=1, c_pos=0.2, c_neg=0.2, exposure="samples", eps=1e-3, max_minibatch=1, device=None):
        super().__init__(m, None, "single", c_pos, c_neg, exposure, eps, max_minibatch, device)

    def run(self, frames, events, items, out_dir=None, names=None, keep=False, bgr=False, niqe=None, png_filter="none",
            png_deflate="host", gt=None, score=None, video=None, video_fps=30, video_quality=90, video_subsampling="420",
            jpeg_pitch=None):
        """As ``SequenceDeblurrer.run``: the same arguments, file names, ``niqe_scores``, ``scores`` and ``video_paths``.  An
        unsorted stream raises only after the frames were written (see ``_EdiRunner``)."""
        return sequence._SequenceRunner.run(self, frames, events, items, out_dir=out_dir, names=names, keep=keep, bgr=bgr, niqe=niqe,
                                            png_filter=png_filter, png_deflate=png_deflate, gt=gt, score=score, video=video,
                                            video_fps=video_fps, video_quality=video_quality, video_subsampling=video_subsampling,
                                            jpeg_pitch=jpeg_pitch)

    _paths = sequence.SequenceDeblurrer._paths
