"""Host -> device hand-over of a batch and event voxelisation on the GPU (the steps immediately before the hot path).

``CUDAPrefetcher`` mirrors the reference's class of that name (basicsr/data/prefetch_dataloader.py:84-125, selected by
``prefetch_mode: cuda`` + ``pin_memory: true`` in the dataset options, train.py:197-205): batch k+1 travels host -> HBM on a
side stream while step k computes; ``next()`` makes the compute stream wait for the copy and starts the following one.

Event voxelisation:

Mirrors ``events_to_voxel_grid(events, num_bins, width, height)`` of the reference
(basicsr/data/event_util.py:6-66; events = [N x 4] rows of [timestamp, x, y, polarity], sorted by
time) and the recurrent datasets' slicing of a (2m+n+1)- or (n+1)-bin grid into sliding two-bin
pairs (image_npy_dataset.py:226-232).

Batch assembly: ``DeviceBatchAssembler`` is the device counterpart of the rest of those datasets' ``__getitem__``
(image_npy_dataset.py:188-232, image_sharp_npy_dataset.py:180-225): from u8 frames and float32 event rows it builds
``lq`` / ``voxel`` / ``gt`` with the kernels of csrc/sample.hip, voxelising only the crop; ``draw_augmentation`` draws
the crop origin and the flips in the reference's order, and ``CUDAPrefetcher(..., assemble=...)`` runs the assembler
on its side stream."""
import ctypes as C

import torch

from . import _lib
from ._lib import RefidHipError, check, lib


def events_to_voxel_grid(events, num_bins, width, height, return_format="CHW"):
    """events: (N,4) float64 CUDA/CPU tensor [t, x, y, p]; returns a (num_bins,H,W) float32 CUDA tensor."""
    if events.dim() != 2 or events.shape[1] != 4:
        raise AssertionError("events must be [N x 4]")
    assert num_bins > 0 and width > 0 and height > 0
    if not events.is_cuda:
        events = events.cuda()
    ev = events.to(torch.float64)
    ts = ev[:, 0].contiguous()
    xs = ev[:, 1].to(torch.int32).contiguous()          # .astype(int): truncation
    ys = ev[:, 2].to(torch.int32).contiguous()
    ps = ev[:, 3].to(torch.float32).contiguous()
    first, last = float(ev[0, 0]), float(ev[-1, 0])
    vox = torch.empty((num_bins, height, width), dtype=torch.float32, device=ev.device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib().refid_events_to_voxel(ts.data_ptr(), xs.data_ptr(), ys.data_ptr(), ps.data_ptr(), ev.shape[0],
                                      num_bins, width, height, first, last, vox.data_ptr(), st),
          "refid_events_to_voxel")
    if return_format == "CHW":
        return vox
    if return_format == "HWC":
        return vox.permute(1, 2, 0)
    raise RefidHipError(f"unknown return_format {return_format}")


def sliding_bin_pairs(voxel):
    """(bins,H,W) -> (bins-1, 2, H, W): adjacent-bin pairs fed to the network as `event`
    (image_npy_dataset.py:226-232)."""
    return torch.stack([voxel[:-1], voxel[1:]], dim=1)


def draw_augmentation(rng, frame_h, frame_w, gt_size, use_hflip, use_rot):
    """(top, left, hflip, vflip, rot90) drawn from ``rng`` (a ``random.Random``, or the ``random`` module) in the
    reference's order with its short-circuits: triple_random_crop's two ``randint`` (transforms.py:212-213; skipped when
    ``gt_size`` is None, image_npy_dataset.py:188), then augment's ``random() < 0.5`` for hflip only if ``use_hflip``,
    for vflip and for rot90 only if ``use_rot`` (transforms.py:110-112)."""
    top = left = 0
    if gt_size is not None:
        if frame_h < gt_size or frame_w < gt_size:
            raise ValueError(f"frame ({frame_h}, {frame_w}) is smaller than the patch size {gt_size}")
        top = rng.randint(0, frame_h - gt_size)
        left = rng.randint(0, frame_w - gt_size)
    hflip = bool(use_hflip and rng.random() < 0.5)
    vflip = bool(use_rot and rng.random() < 0.5)
    rot90 = bool(use_rot and rng.random() < 0.5)
    return top, left, hflip, vflip, rot90


def layout_shapes(layout, count, bins, m, h, w):
    """The shapes of (lq, voxel, gt) for ``count`` samples of (h, w) in a layout of both assemblers: 'blur', 'sharp'
    (sliding bin pairs in voxel, bins-1 ground-truth frames) or 'single' (plain bins, one ground-truth frame)."""
    if layout == "single":
        return (count, 3, h, w), (count, bins, h, w), (count, 3, h, w)
    lq = (count, 6 + 2 * (m - 1), h, w) if layout == "blur" else (count, 2, 3, h, w)
    return lq, (count, bins - 1, 2, h, w), (count, bins - 1, 3, h, w)


class GeometryCache(dict):
    """What both assemblers keep per geometry: (count, h, w) -> {'scratch': int64 (count, bins, h, w), 'table_dev' /
    'table_pin': the descriptor table on the device / in pinned memory, 'uploaded': the event behind the last copy out of
    the pinned buffer, and with ``parts`` voxel_norm's 'parts'}."""

    def __init__(self, device, bins, parts):
        super().__init__()
        self.device, self.bins, self.parts = device, bins, parts

    def upload(self, key, table):
        """The entry of ``key`` (made at its first use) with the ctypes array ``table`` copied to its device table: through
        the pinned buffer and without blocking, once the previous copy has left that buffer."""
        c = self.get(key)
        if c is None:
            count, h, w = key
            c = {"scratch": torch.empty((count, self.bins, h, w), dtype=torch.int64, device=self.device),
                 "table_dev": torch.empty(C.sizeof(table), dtype=torch.uint8, device=self.device),
                 "table_pin": torch.empty(C.sizeof(table), dtype=torch.uint8).pin_memory(),
                 "uploaded": None}
            if self.parts:
                from . import ops
                c["parts"] = ops.voxel_norm_parts(count, self.bins * h * w, self.device)
            self[key] = c
        if c["uploaded"] is not None:
            c["uploaded"].synchronize()
        C.memmove(c["table_pin"].data_ptr(), C.addressof(table), C.sizeof(table))
        c["table_dev"].copy_(c["table_pin"], non_blocking=True)
        c["uploaded"] = torch.cuda.Event()
        c["uploaded"].record()
        return c


_RAW_KEYS = ("frames", "events", "first_stamp", "last_stamp", "frame_hw", "origin", "top", "left", "hflip", "vflip", "rot90")


class DeviceBatchAssembler:
    """Builds ``{'lq', 'voxel', 'gt'}`` on the device from raw samples, one launch set per batch (csrc/sample.hip).

    ``layout='blur'``: 2m+n+1 voxel bins, lq (B, 6+2(m-1), h, w) = blur0 | bins 1..m-1 | blur1 | bins m+2+n.. (the blur
    datasets with ``return_deblur_voxel``); ``layout='sharp'``: n+1 bins, lq (B, 2, 3, h, w).  voxel is (B, bins-1, 2, h, w),
    gt (B, bins-1, 3, h, w).  ``gt_size=None`` keeps the whole frame (all samples of a batch then share one frame size, and
    rot90 needs a square frame).

    ``layout='single'`` (GoProSingleImageEventDataset, data/Single_image_npy_dataset.py:136-201; ``m`` and ``n`` are not
    used): ``num_bins`` bins, frames u8 (2, Hwin, Wwin, 3) = blur, sharp; lq (B, 3, h, w), gt (B, 3, h, w) and voxel
    (B, num_bins, h, w), the plain bins after ``voxel_norm`` (event_util.py:141-160, kept at :187) unless
    ``norm_voxel=False``.  A sample whose non-zero voxel elements have no spread comes out all zeros, where the reference
    returns NaN.

    ``__call__(raw_batch)``: a list of per-sample dicts, or a dict of per-sample lists.  Per sample:
      frames       u8 tensor (2 + bins-1, Hwin, Wwin, 3), BGR: blur0, blur1, then the ground-truth frames; host or device
      events       float32 tensor (N, 4) rows [t, x, y, p] as the datasets build them (N may be 0); host or device
      first_stamp, last_stamp   optional; default events[0,0] / events[-1,0] (event_util.py:25-31).  Give them when the
                   events were pre-filtered (e.g. to the crop window) so that the normalisation does not change
      frame_hw     optional (H, W) of the full frame; default: the frames' own size
      origin       optional (y0, x0) of the uploaded window inside the frame; default (0, 0)
      top, left, hflip, vflip, rot90   from ``draw_augmentation``; default 0
    Every other key is passed through as a per-sample list.  Everything runs on the current stream; host tensors are
    uploaded there (pin them for an asynchronous copy).  The cached scratch is ordered by that stream only: use one
    assembler per stream (``CUDAPrefetcher`` runs its own on its side stream)."""

    def __init__(self, m=1, n=1, layout="blur", gt_size=None, use_hflip=False, use_rot=False, device=None, num_bins=6,
                 norm_voxel=True):
        if layout not in ("blur", "sharp", "single"):
            raise RefidHipError(f"DeviceBatchAssembler: unknown layout {layout!r} ('blur', 'sharp' or 'single')")
        from . import ops
        self.m, self.n = int(m), int(n)
        self.layout = layout
        self.norm_voxel = bool(norm_voxel)
        if layout == "single":
            self._layout = None
            self.bins = ops.single_bins(num_bins)
            self.n_frames = 2
        else:
            self._layout = _lib.LAYOUT_BLUR if layout == "blur" else _lib.LAYOUT_SHARP
            self.bins = ops.assemble_bins(self.m, self.n, self._layout)
            self.n_frames = self.bins + 1
        self.gt_size = None if gt_size is None else int(gt_size)
        self.use_hflip, self.use_rot = bool(use_hflip), bool(use_rot)
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise RefidHipError("DeviceBatchAssembler: a GPU device is required (the HIP path has no CPU fallback)")
        self._last = None
        self._cache = GeometryCache(self.device, self.bins, layout == "single" and self.norm_voxel)     # keys (B, h, w)

    def draw(self, rng, frame_h, frame_w):
        """``draw_augmentation`` with this assembler's gt_size / use_hflip / use_rot, as a dict for a raw sample."""
        keys = ("top", "left", "hflip", "vflip", "rot90")
        return dict(zip(keys, draw_augmentation(rng, frame_h, frame_w, self.gt_size, self.use_hflip, self.use_rot)))

    def rerun(self, stages):
        """Launches ``stages`` (``_lib.ASSEMBLE_*``) again for the batch of the last call, into its outputs: lets a
        benchmark put device events around a single kernel (tools/bench_assemble.py)."""
        self._run(self._last[0], stages)

    def _run(self, desc, stages):
        from . import ops
        if self.layout == "single":
            ops.assemble_single(desc, stages)
        else:
            ops.assemble_batch(desc, stages & _lib.ASSEMBLE_ALL)

    @staticmethod
    def _samples(raw_batch):
        if isinstance(raw_batch, dict):
            keys = list(raw_batch)
            count = len(raw_batch["frames"])
            return [{k: raw_batch[k][i] for k in keys} for i in range(count)]
        return list(raw_batch)

    def __call__(self, raw_batch, stages=_lib.ASSEMBLE_ALL | _lib.ASSEMBLE_STATS):
        samples = self._samples(raw_batch)
        if not samples:
            raise RefidHipError("DeviceBatchAssembler: empty batch")
        B = len(samples)
        table = (_lib.SampleDesc * B)()
        keep = []                             # device tensors the kernels read
        crop = None
        for b, s in enumerate(samples):
            fr, ev = s["frames"], s["events"]
            if fr.dtype != torch.uint8 or fr.dim() != 4 or fr.shape[3] != 3 or fr.shape[0] != self.n_frames:
                what = "blur, sharp" if self.layout == "single" else f"blur0, blur1, {self.bins - 1} ground-truth frames"
                raise RefidHipError(f"DeviceBatchAssembler: sample {b}: frames must be uint8 ({self.n_frames}, H, W, 3) "
                                    f"({what}), got {fr.dtype} {tuple(fr.shape)}")
            if ev.dtype != torch.float32 or ev.dim() != 2 or ev.shape[1] != 4:
                raise RefidHipError(f"DeviceBatchAssembler: sample {b}: events must be float32 (N, 4) rows [t, x, y, p], "
                                    f"got {ev.dtype} {tuple(ev.shape)}")
            n_ev = ev.shape[0]
            first, last = s.get("first_stamp"), s.get("last_stamp")
            if first is None or last is None:
                first, last = (float(ev[0, 0]), float(ev[-1, 0])) if n_ev else (0.0, 0.0)
            fr = fr.contiguous().to(self.device, non_blocking=True)
            ev = ev.contiguous().to(self.device, non_blocking=True)
            keep += [fr, ev]
            win_h, win_w = fr.shape[1], fr.shape[2]
            y0, x0 = s.get("origin", (0, 0))
            H, W = s.get("frame_hw", (y0 + win_h, x0 + win_w))
            h, w = (H, W) if self.gt_size is None else (self.gt_size, self.gt_size)
            if crop is None:
                crop = (int(h), int(w))
            elif crop != (int(h), int(w)):
                raise RefidHipError(f"DeviceBatchAssembler: sample {b}: output {h}x{w} differs from sample 0's "
                                    f"{crop[0]}x{crop[1]} (gt_size=None needs equal frame sizes)")
            top, left = int(s.get("top", 0)), int(s.get("left", 0))
            if top < y0 or left < x0 or top + h > y0 + win_h or left + w > x0 + win_w:
                raise RefidHipError(f"DeviceBatchAssembler: sample {b}: crop {h}x{w} at ({top},{left}) does not fit inside "
                                    f"the uploaded {win_h}x{win_w} window at ({y0},{x0})")
            d = table[b]
            d.events, d.n_events = (ev.data_ptr() if n_ev else None), n_ev
            d.first_stamp, d.last_stamp = float(first), float(last)
            d.height, d.width = int(H), int(W)
            d.frames, d.frame_stride, d.row_pitch = fr.data_ptr(), win_h * win_w * 3, win_w * 3
            d.y0, d.x0, d.top, d.left = int(y0), int(x0), top, left
            d.hflip, d.vflip, d.rot90 = int(bool(s.get("hflip", 0))), int(bool(s.get("vflip", 0))), int(bool(s.get("rot90", 0)))
        h, w = crop
        c = self._cache.upload((B, h, w), table)
        lq, voxel, gt = (torch.empty(shape, dtype=torch.float32, device=self.device)
                         for shape in layout_shapes(self.layout, B, self.bins, self.m, h, w))
        single = self.layout == "single"
        desc = _lib.SingleDesc() if single else _lib.AssembleDesc()
        desc.samples_host, desc.samples_dev, desc.batch = C.addressof(table), c["table_dev"].data_ptr(), B
        desc.crop_h, desc.crop_w = h, w
        desc.scratch, desc.lq, desc.voxel, desc.gt = c["scratch"].data_ptr(), lq.data_ptr(), voxel.data_ptr(), gt.data_ptr()
        if single:
            desc.bins, desc.norm = self.bins, int(self.norm_voxel)
            desc.parts = c["parts"].data_ptr() if self.norm_voxel else None
        else:
            desc.m, desc.n, desc.layout = self.m, self.n, self._layout
        self._run(desc, stages)
        self._last = (desc, table, keep)      # rerun() launches again from these
        cur = torch.cuda.current_stream(self.device)
        for t in keep:                        # (tensors the caller allocated on another stream stay valid until the kernels ran)
            t.record_stream(cur)
        out = {"lq": lq, "voxel": voxel, "gt": gt}
        for k in samples[0]:
            if k not in _RAW_KEYS:
                out[k] = [s[k] for s in samples]
        return out


class CUDAPrefetcher:
    """prefetch_dataloader.py:84-125.  ``loader`` is any re-iterable of dict batches whose tensors live in (preferably
    pinned) host memory; ``next()`` returns the batch on the device, or None at the end of an epoch; ``reset()`` starts
    the next epoch.  Additions over the reference: the returned tensors are tied to the consumer stream
    (``record_stream``: the caching allocator must not hand their memory to the NEXT copy while the step still reads
    them), and -- only with ``time_waits=True`` (bench.py) -- the time the compute stream actually had to wait for a copy
    is measured with events (``exposed_ms()``); a training loop keeps no per-iteration state, like the reference class.
    ``assemble`` (a ``DeviceBatchAssembler``): the loader yields RAW batches, and ``preload()`` uploads them and runs the
    assembler on the side stream, so that assembling batch k+1 overlaps step k."""

    def __init__(self, loader, opt=None, device=None, time_waits=False, assemble=None):
        self.ori_loader = loader
        self.assemble = assemble
        self.loader = iter(loader)
        self.opt = opt
        if device is None:
            device = torch.device("cuda" if (opt or {}).get("num_gpu", 1) != 0 else "cpu")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RefidHipError("CUDAPrefetcher: a GPU device is required (the HIP path has no CPU fallback)")
        self.stream = torch.cuda.Stream(device=self.device)
        self.time_waits = bool(time_waits)
        self._waits = []                     # (event before the wait, event after it) on the consumer stream; time_waits only
        self._waited_ms = 0.0                # completed pairs are folded in here, so the list stays bounded
        self.preload()

    def preload(self):
        try:
            self.batch = next(self.loader)
        except StopIteration:
            self.batch = None
            return None
        with torch.cuda.stream(self.stream):
            if self.assemble is not None:
                self.batch = self.assemble(self.batch)
                return None
            self.batch = {k: (v.to(device=self.device, non_blocking=True) if torch.is_tensor(v) else v)
                          for k, v in self.batch.items()}

    def next(self):
        cur = torch.cuda.current_stream(self.device)
        if self.time_waits:
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record(cur)
            cur.wait_stream(self.stream)
            e1.record(cur)
            self._waits.append((e0, e1))
            while len(self._waits) > 64 and self._waits[0][1].query():        # fold finished pairs: no unbounded event list
                a, b = self._waits.pop(0)
                self._waited_ms += a.elapsed_time(b)
        else:
            cur.wait_stream(self.stream)
        batch = self.batch
        if batch is not None:
            for v in batch.values():
                if torch.is_tensor(v):
                    v.record_stream(cur)
        self.preload()
        return batch

    def reset(self):
        self.loader = iter(self.ori_loader)
        self.preload()

    def exposed_ms(self, clear=True):
        """Total time (ms) the consumer stream spent waiting for host -> device copies since the last call
        (synchronises the device).  Needs ``time_waits=True``."""
        if not self.time_waits:
            raise RefidHipError("CUDAPrefetcher.exposed_ms: construct with time_waits=True")
        torch.cuda.synchronize(self.device)
        t = self._waited_ms + sum(a.elapsed_time(b) for a, b in self._waits)
        if clear:
            self._waits = []
            self._waited_ms = 0.0
        return t
