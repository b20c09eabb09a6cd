"""Events from high-frame-rate video: the ESIM contrast-threshold model on the GPU (csrc/event_sim.hip; the contract is
"Simulated events" in include/refid_hip.h, tests/event_sim_ref.py restates it).

Every pixel keeps a reference level in log intensity; between two frames its level moves linearly, and each time it
passes the reference by a threshold an event leaves with an interpolated time stamp.  The arithmetic is integer (levels
and thresholds in units of 2^-16 from a 256-entry table), so the rows are reproducible to the bit.  The result is the
resident, time-sorted float32 (E, 4) tensor [t, x, y, p] that ``SequenceAssembler.load`` takes, and, through
``save_event_npz``, the reference's per-interval ``.npz`` files.

Not modelled: a refractory period, leak and shot noise, hot pixels, frame upsampling before simulation, colour or Bayer
events (blurry key frames are ``refid_amd.blur_synth``'s).  There is no host fallback."""
import os

import numpy as np
import torch

from . import _lib
from ._lib import RefidHipError

FIXED_ONE = 1 << 16          # a threshold of 1.0 (natural-log units) in fixed point
DEFAULT_FLOOR = 0.03         # the least per-pixel threshold threshold_maps draws: just above the cap's bound for the default table


def default_lut(eps=1e-3):
    """int32 [256]: rint(65536 ln(v / 255 + eps)) in float64, v = 0 .. 255 (span 452773 for eps = 1e-3)."""
    eps = float(eps)
    if not eps > 0.0:
        raise RefidHipError(f"default_lut: eps {eps} must be positive")
    v = np.arange(256, dtype=np.float64)
    return np.rint(65536.0 * np.log(v / 255.0 + eps)).astype(np.int32)


def to_fixed(c):
    """A threshold in natural-log units -> units of 2^-16."""
    return int(np.rint(float(c) * FIXED_ONE))


def min_threshold(lut):
    """The least threshold (units of 2^-16) that keeps a pixel at or below 255 events per interval on this table:
    (lut.max - lut.min) // c + 1 <= 255.  1776 for the default table."""
    lut = np.asarray(lut, dtype=np.int64).reshape(-1)
    return int((lut.max() - lut.min()) // _lib.EVENT_SIM_CAP + 1)


def check_cap(lut, c_min):
    """RefidHipError when a threshold of ``c_min`` (units of 2^-16) could give more than 255 events per pixel and interval."""
    lut = np.asarray(lut, dtype=np.int64).reshape(-1)
    c_min = int(c_min)
    if c_min < 1:
        raise RefidHipError(f"event_sim: the smallest threshold {c_min} must be at least 1 (units of 2^-16)")
    span, bound = int(lut.max() - lut.min()), min_threshold(lut)
    if span // c_min + 1 > _lib.EVENT_SIM_CAP:
        raise RefidHipError(f"event_sim: the smallest threshold {c_min} (units of 2^-16, {c_min / FIXED_ONE:.4f}) allows {span // c_min + 1} "
                            f"events per pixel and interval over the table's span {span}, the cap is {_lib.EVENT_SIM_CAP}: thresholds must "
                            f"be at least {bound} ({bound / FIXED_ONE:.4f})")


def threshold_maps(h, w, c_pos, c_neg, sigma=0.0, seed=0, floor=DEFAULT_FLOOR):
    """The thresholds in units of 2^-16: ``(c_pos, c_neg)`` as two ints for ``sigma = 0``, else two int32 (h, w) arrays drawn
    per pixel from N(c, sigma) with a seeded CPU generator (PCG64; positive map first, row-major), clamped below at ``floor``."""
    c_pos, c_neg, sigma, floor = float(c_pos), float(c_neg), float(sigma), float(floor)
    if sigma < 0.0 or not np.isfinite(sigma):
        raise RefidHipError(f"threshold_maps: sigma {sigma} must be finite and not negative")
    for name, c in (("c_pos", c_pos), ("c_neg", c_neg)):
        if not np.isfinite(c) or to_fixed(c) < 1 or to_fixed(c) >= 2 ** 31:
            raise RefidHipError(f"threshold_maps: {name} {c} must be at least 2^-16 and below 32768")
    if sigma == 0.0:
        return to_fixed(c_pos), to_fixed(c_neg)
    if not floor > 0.0 or to_fixed(floor) < 1:
        raise RefidHipError(f"threshold_maps: floor {floor} must be at least 2^-16")
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    out = []
    for c in (c_pos, c_neg):
        draw = rng.normal(c, sigma, size=(int(h), int(w)))
        out.append(np.rint(np.clip(draw, floor, 32767.0) * FIXED_ONE).astype(np.int32))
    return out[0], out[1]


def save_event_npz(out_dir, events, offsets, first=0):
    """The reference's per-interval event files: ``{out_dir}/{first + k:06d}.npz`` for interval k with the keys ``x``, ``y``
    (uint16), ``timestamp`` (float32) and ``polarity`` (int8, 1 or -1).  ``sequence.load_event_npz`` on the sorted files gives
    back exactly ``events``.  Returns the paths."""
    rows = events.detach().cpu().numpy() if torch.is_tensor(events) else np.asarray(events)
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if rows.dtype != np.float32 or rows.ndim != 2 or rows.shape[1] != 4:
        raise RefidHipError(f"save_event_npz: events must be float32 (E, 4) rows [t, x, y, p], got {rows.dtype} {rows.shape}")
    if len(offsets) < 1 or offsets[0] != 0 or offsets[-1] != len(rows) or np.any(np.diff(offsets) < 0):
        raise RefidHipError(f"save_event_npz: offsets must rise from 0 to E={len(rows)}")
    if len(rows) and (rows[:, 1:3].min() < 0 or rows[:, 1:3].max() > 65535):
        raise RefidHipError("save_event_npz: x and y must fit uint16")
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for k in range(len(offsets) - 1):
        part = rows[offsets[k]:offsets[k + 1]]
        path = os.path.join(out_dir, f"{first + k:06d}.npz")
        np.savez(path, x=part[:, 1].astype(np.uint16), y=part[:, 2].astype(np.uint16), timestamp=part[:, 0].astype(np.float32),
                 polarity=np.where(part[:, 3] > 0, 1, -1).astype(np.int8))
        paths.append(path)
    return paths


class EventSimulator:
    """The simulator of one (height, width) stream.  ``c_pos`` / ``c_neg``: thresholds in natural-log units;
    ``sigma`` > 0 draws per-pixel thresholds (``threshold_maps``).  ``lut``: another
    int32 [256] table in place of ``default_lut(eps)``.  ``reset(frame0)`` starts a clip, ``step(frames, stamps)`` takes a chunk
    whose first frame is the previous chunk's last (the state carries over, so long clips run in bounded memory),
    ``simulate`` does both over a whole clip.  Thresholds that could give a pixel more than 255 events in one interval are
    refused here, before anything is launched."""

    def __init__(self, height, width, c_pos=0.2, c_neg=0.2, sigma=0.0, seed=0, eps=1e-3, lut=None, device=None, floor=DEFAULT_FLOOR):
        self.height, self.width = int(height), int(width)
        if self.height < 1 or self.width < 1 or self.height * self.width > _lib.EVENT_SIM_MAX_PIXELS:
            raise RefidHipError(f"EventSimulator: height {height} * width {width} must be 1 .. {_lib.EVENT_SIM_MAX_PIXELS} pixels")
        lut = default_lut(eps) if lut is None else np.asarray(lut)
        if lut.shape != (256,) or not np.issubdtype(lut.dtype, np.integer) or np.abs(lut.astype(np.int64)).max() >= 2 ** 31:
            raise RefidHipError(f"EventSimulator: lut must hold 256 int32 levels, got {lut.dtype} {lut.shape}")
        self.lut_host = np.ascontiguousarray(lut, dtype=np.int32)
        self.lut_range = (int(self.lut_host.min()), int(self.lut_host.max()))
        cp, cn = threshold_maps(self.height, self.width, c_pos, c_neg, sigma, seed, floor)
        check_cap(self.lut_host, min(int(np.min(cp)), int(np.min(cn))))    # (scalars, or the bound the clamp gives the maps)
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise RefidHipError("EventSimulator: a GPU device is required (csrc/event_sim.hip has no host fallback)")
        self.lut = torch.from_numpy(self.lut_host).to(self.device)
        if isinstance(cp, np.ndarray):
            self.c_pos, self.c_neg = torch.from_numpy(cp).to(self.device), torch.from_numpy(cn).to(self.device)
            self.c_min = int(torch.minimum(self.c_pos.min(), self.c_neg.min()))        # one device reduction, here only
            check_cap(self.lut_host, self.c_min)
        else:
            self.c_pos, self.c_neg, self.c_min = cp, cn, None
        self.state = self.last_stamp = None

    def _frames(self, frames, what):
        frames = frames if torch.is_tensor(frames) else torch.as_tensor(np.asarray(frames))
        if frames.dtype != torch.uint8 or frames.dim() != 4 or tuple(frames.shape[1:]) != (self.height, self.width, 3):
            raise RefidHipError(f"EventSimulator.{what}: frames must be uint8 (N, {self.height}, {self.width}, 3), got {frames.dtype} "
                                f"{tuple(frames.shape)}")
        return frames.to(self.device).contiguous()

    def reset(self, frame0, bgr=False):
        """Starts a clip: the reference levels become those of ``frame0`` uint8 (H, W, 3)."""
        from . import ops
        frame0 = frame0 if torch.is_tensor(frame0) else torch.as_tensor(np.asarray(frame0))
        frame = self._frames(frame0[None] if frame0.dim() == 3 else frame0, "reset")[0]
        self.state = ops.event_sim_reset(frame, self.lut, bgr=bgr)
        self.last_stamp = None
        return self

    def step(self, frames, stamps, bgr=False):
        """The events of a chunk uint8 (N, H, W, 3), N >= 2, whose first frame is the frame ``reset`` got or the previous
        chunk's last -> ``(rows, offsets)`` as ``ops.event_sim`` returns them."""
        from . import ops
        if self.state is None:
            raise RefidHipError("EventSimulator.step: reset() on the clip's first frame first")
        stamps = np.asarray(stamps, dtype=np.float64).reshape(-1)
        if self.last_stamp is not None and len(stamps) and stamps[0] != self.last_stamp:
            raise RefidHipError(f"EventSimulator.step: stamps[0] = {stamps[0]!r} is not the previous chunk's last stamp {self.last_stamp!r} "
                                f"(chunks share their boundary frame)")
        rows, offsets = ops.event_sim(self._frames(frames, "step"), stamps, self.state, self.lut, self.c_pos, self.c_neg, bgr=bgr,
                                      lut_range=self.lut_range, c_min=self.c_min)
        self.last_stamp = float(stamps[-1])
        return rows, offsets

    def simulate(self, frames, stamps, chunk=64, bgr=False):
        """A whole clip: ``frames`` uint8 (N, H, W, 3) on the host or the device, ``stamps`` (N,) -> ``(events, offsets)``:
        float32 (E, 4) on the device, int64 (N,) on the host.  ``chunk`` frames go through one call (2 .. 512); a host clip
        is uploaded chunk by chunk."""
        chunk, n = int(chunk), len(frames)
        if not 2 <= chunk <= _lib.EVENT_SIM_MAX_FRAMES:
            raise RefidHipError(f"EventSimulator.simulate: chunk {chunk} must be 2 .. {_lib.EVENT_SIM_MAX_FRAMES} frames")
        stamps = np.asarray(stamps, dtype=np.float64).reshape(-1)
        if n < 2 or len(stamps) != n:
            raise RefidHipError(f"EventSimulator.simulate: {n} frames (at least 2) with {len(stamps)} stamps")
        self.reset(frames[0], bgr=bgr)
        rows, offsets = [], [np.zeros((1,), dtype=np.int64)]
        for at in range(0, n - 1, chunk - 1):
            r, o = self.step(frames[at:at + chunk], stamps[at:at + chunk], bgr=bgr)
            rows.append(r)
            offsets.append(o[1:] + offsets[-1][-1])
        return torch.cat(rows), np.concatenate(offsets)
