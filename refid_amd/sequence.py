"""Test-time entry: interpolate the frame pairs of a whole sequence, without ground truth and at any frame size.

The key frames and ONE event stream of a sequence are uploaded once (``SequenceAssembler.load``); every pair -- two
key-frame indices and a row window of the stream -- becomes one sample of ``lq`` / ``voxel`` through the kernels of
csrc/sequence.hip, padded up to the multiple the network takes.  ``SequenceInterpolator`` runs the network over the
pairs in minibatches, assembling minibatch k+1 on a side stream while minibatch k computes (the way ``CUDAPrefetcher``
does it), crops the result back, quantises it with ``metrics.val_tail`` and hands the uint8 frames to
``validation.FrameWriter``.  ``SequenceDeblurrer`` does the same for the single-image deblurring network: one blurry frame
and the events of its exposure per item (``frame_windows``, ``SequenceAssembler(layout='single')``).

Window search stays on the host: the host loaded the events, so ``np.searchsorted`` over the same float32 timestamp
column the kernel reads costs nothing and needs no synchronisation."""
import collections
import contextlib
import ctypes as C
import os

import numpy as np
import torch

from . import _lib, metrics, niqe, score, validation
from ._lib import RefidHipError
from .data import GeometryCache, layout_shapes

Pair = collections.namedtuple("Pair", "left right row0 row1 first_stamp last_stamp")


def pair_windows(t, begins, ends):
    """Event rows of the half-open time windows [begins[k], ends[k]) of a stream: an int64 (K, 2) array of
    ``[searchsorted(t, begins[k], 'left'), searchsorted(t, ends[k], 'left'))``.  ``t`` is the float32 timestamp column
    (non-decreasing, else RefidHipError); the bounds are cast to float32, the type the events carry.  An event exactly at
    ``ends[k]`` belongs to the next window."""
    t = np.ascontiguousarray(np.asarray(t, dtype=np.float32).reshape(-1))
    if t.size > 1 and bool(np.any(t[1:] < t[:-1])):
        raise RefidHipError("pair_windows: the event timestamps are not non-decreasing (sort the stream by time first)")
    b = np.asarray(begins, dtype=np.float32).reshape(-1)
    e = np.asarray(ends, dtype=np.float32).reshape(-1)
    if b.shape != e.shape:
        raise RefidHipError(f"pair_windows: {b.size} window begins, {e.size} window ends")
    r0 = np.searchsorted(t, b, "left").astype(np.int64)
    r1 = np.maximum(np.searchsorted(t, e, "left").astype(np.int64), r0)        # ends[k] < begins[k]: an empty window
    return np.stack([r0, r1], axis=1)


def sharp_windows(frame_stamps):
    """Sharp key frames: pairs (k, k+1) with the window [stamp_k, stamp_{k+1}).  Returns (lefts, rights, begins, ends)."""
    s = np.asarray(frame_stamps).reshape(-1)
    k = np.arange(max(len(s) - 1, 0))
    return k, k + 1, s[:-1], s[1:]


def exposure_windows(starts, ends):
    """Blurry key frames with exposures [starts[k], ends[k]]: pairs (k, k+1) with the window [start_k, end_{k+1}), which
    covers both exposures (consecutive windows overlap).  Returns (lefts, rights, begins, ends)."""
    s, e = np.asarray(starts).reshape(-1), np.asarray(ends).reshape(-1)
    if s.shape != e.shape:
        raise RefidHipError(f"exposure_windows: {s.size} exposure starts, {e.size} exposure ends")
    k = np.arange(max(len(s) - 1, 0))
    return k, k + 1, s[:-1], e[1:]


def frame_windows(starts, ends):
    """Single blurry frames with exposures [starts[k], ends[k]): item k is frame k with the window [start_k, end_k).
    Returns (k, k, starts, ends) for ``make_pairs`` (the single layout reads ``left`` only)."""
    s, e = np.asarray(starts).reshape(-1), np.asarray(ends).reshape(-1)
    if s.shape != e.shape:
        raise RefidHipError(f"frame_windows: {s.size} exposure starts, {e.size} exposure ends")
    k = np.arange(len(s))
    return k, k, s, e


def make_pairs(t, lefts, rights, begins, ends, stamps="events"):
    """[Pair] for ``SequenceAssembler.assemble``.  ``stamps='events'`` (what the reference datasets do, event_util.py:25-31):
    the normalisation runs from the stamp of the first row of the window to that of its last row; an empty window gives
    (0, 0) and an all-zero voxel.  ``stamps='bounds'``: from ``begins[k]`` to ``ends[k]`` (as float32)."""
    if stamps not in ("events", "bounds"):
        raise RefidHipError(f"make_pairs: unknown stamps {stamps!r} ('events' or 'bounds')")
    t = np.asarray(t, dtype=np.float32).reshape(-1)
    rows = pair_windows(t, begins, ends)
    lefts, rights = np.asarray(lefts).reshape(-1), np.asarray(rights).reshape(-1)
    if not len(lefts) == len(rights) == len(rows):
        raise RefidHipError(f"make_pairs: {len(lefts)} lefts, {len(rights)} rights, {len(rows)} windows")
    b32, e32 = np.asarray(begins, dtype=np.float32).reshape(-1), np.asarray(ends, dtype=np.float32).reshape(-1)
    out = []
    for k, (r0, r1) in enumerate(rows.tolist()):
        if stamps == "bounds":
            first, last = float(b32[k]), float(e32[k])
        else:
            first, last = (float(t[r0]), float(t[r1 - 1])) if r1 > r0 else (0.0, 0.0)
        out.append(Pair(int(lefts[k]), int(rights[k]), r0, r1, first, last))
    return out


def load_event_npz(paths, swap_xy=False):
    """The reference's per-frame event files (``.npz`` with keys ``x``, ``y``, ``timestamp``, ``polarity``) concatenated to
    float32 rows [t, x, y, p], exactly as image_sharp_npy_dataset.py:145-163 builds them.  ``swap_xy``: the HighREV
    files carry x and y in each other's column (image_sharp_Ruisi_dataset.py:145-157).

    float32 timestamps are the reference's choice, and they are kept because the voxel grid is defined on them.  What it
    costs: float32 has 24 significant bits, so the spacing of representable stamps is t * 2^-23 -- 1 us near t = 8 s of a
    microsecond clock, 8 us near a minute, and at epoch-sized stamps (1.6e15 us) 1.3e8 us, where every event of a window
    collapses onto a few values.  Subtract a per-sequence origin before saving such streams."""
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    out = np.zeros((0, 4), dtype=np.float32)
    for path in paths:
        z = np.load(path)
        x = z["x"].astype(np.float32).reshape(-1, 1)
        y = z["y"].astype(np.float32).reshape(-1, 1)
        t = z["timestamp"].astype(np.float32).reshape(-1, 1)
        p = z["polarity"].astype(np.float32).reshape(-1, 1)
        if swap_xy:
            x, y = y, x
        out = np.concatenate((out, np.concatenate((t, x, y, p), axis=1)), axis=0)
    return out


PNG_WORKERS_MAX = 16      # the inflate pool never grows with the machine: a shared box shows more CPUs than a job may use


def _load_staged(what, items, device, workers, frames_per_launch, plan):
    """The pipeline under ``load_png_frames`` and ``load_jpeg_frames`` (``what``: the name in the messages).  After the
    argument checks ``plan(device)`` gives ``(out, shapes, fill, launch)``: the result tensor; per frame the ``(shape,
    dtype)`` of every staging array; ``fill(item, *views)``, which runs in a worker thread and writes one frame's slices of a
    pinned staging set (numpy views); ``launch(first, n, host, dev)``, which queues the decode of frames first .. first+n-1
    on the current stream from the chunk's staging tensors ``host`` and their uploaded copies ``dev``.

    ``workers`` threads (at most ``PNG_WORKERS_MAX``) fill the chunks of ``frames_per_launch`` frames, two chunks ahead of
    the launches: the one in hand and the next, each in its own staging set (one set when there is one chunk).  A chunk whose
    workers are done is uploaded without blocking and launched; its set is handed to the workers again only after the
    event behind that upload has completed.  A worker's exception cancels what has not started and is raised again, the
    first failing frame's in frame order.  Returns ``out`` without synchronising."""
    from concurrent.futures import ThreadPoolExecutor
    workers, per = int(workers), int(frames_per_launch)
    if not items:
        raise RefidHipError(f"{what}: no files")
    if not 1 <= workers <= PNG_WORKERS_MAX or per < 1:
        raise RefidHipError(f"{what}: workers {workers} must be 1..{PNG_WORKERS_MAX} and frames_per_launch {per} >= 1")
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RefidHipError(f"{what}: a GPU device is required (the HIP path has no CPU fallback)")
    out, shapes, fill, launch = plan(device)
    per = min(per, len(items))
    chunks = [items[i:i + per] for i in range(0, len(items), per)]
    with ThreadPoolExecutor(max_workers=workers) as pool, torch.cuda.device(device):
        staging = [[torch.empty((per, *shape), dtype=dtype).pin_memory() for shape, dtype in shapes]
                   for _ in range(min(2, len(chunks)))]
        copied = [None] * len(staging)                     # the event after the upload that last read each set
        ahead = collections.deque(maxlen=2)                # the chunks being filled: the one in hand and the next

        def submit(k):
            if k < len(chunks):
                if copied[k % 2] is not None:
                    copied[k % 2].synchronize()
                views = [t.numpy() for t in staging[k % 2]]
                ahead.append([pool.submit(fill, item, *(v[i] for v in views)) for i, item in enumerate(chunks[k])])

        submit(0)
        submit(1)
        for k, chunk in enumerate(chunks):
            futures = ahead.popleft()
            try:
                for fut in futures:
                    fut.result()
            except BaseException:
                for later in list(ahead) + [futures]:
                    for f in later:
                        f.cancel()
                raise
            n = len(chunk)
            host = [t[:n] for t in staging[k % 2]]
            dev = [torch.empty(t.shape, dtype=t.dtype, device=device) for t in host]
            for d, t in zip(dev, host):
                d.copy_(t, non_blocking=True)
            copied[k % 2] = torch.cuda.Event()
            copied[k % 2].record()
            launch(k * per, n, host, dev)
            submit(k + 2)
    return out


def load_png_frames(paths, device=None, workers=8, frames_per_launch=8):
    """8-bit RGB / grey PNG key frames of one size -> uint8 (N, H, W, 3) on the device, a grey file replicated to three
    channels: what ``SequenceAssembler.load`` takes.  ``paths``: the files in order, or a directory (its ``*.png`` sorted
    by name).  The files are read and inflated by ``workers`` threads (``zlib`` releases the GIL; at most
    ``PNG_WORKERS_MAX``), which check their filter bytes on the host and copy the rows straight into one of two pinned
    staging buffers; every chunk of ``frames_per_launch`` frames is uploaded without blocking and unfiltered by one
    ``refid_png_unfilter`` launch (csrc/png.hip) on the current stream, while the pool inflates the next chunk.  A staging
    buffer is written again only after the event behind its last upload has completed.  Files that differ in (H, W,
    channels): RefidHipError naming the first one; a broken file: ``png.read_png``'s ValueError.  Rows wider than the
    kernel's line (``_lib.PNG_MAX_ROW_BYTES``) are decoded on the host by ``png.read_png``, in the same workers, and only
    uploaded.  Does not synchronise at the end."""
    import glob
    from . import ops, png
    if isinstance(paths, (str, os.PathLike)):
        paths = sorted(glob.glob(os.path.join(paths, "*.png"))) if os.path.isdir(paths) else [paths]
    paths = [os.fspath(p) for p in paths]

    def plan(device):
        w, h, ch = png.read_header(paths[0])               # (the header alone: no worker waits for a whole file)
        out = torch.empty((len(paths), h, w, 3), dtype=torch.uint8, device=device)
        if w * ch > _lib.PNG_MAX_ROW_BYTES:                # the host route for this file set
            def fill(path, pixels):
                img = png.read_png(path)
                if img.shape != ((h, w, 3) if ch == 3 else (h, w)):
                    raise RefidHipError(f"load_png_frames: {path} differs in size from {paths[0]}")
                pixels[...] = img if ch == 3 else img[:, :, None]

            def launch(first, n, host, dev):
                out[first:first + n].copy_(dev[0])

            return out, [((h, w, 3), torch.uint8)], fill, launch

        def fill(path, rows):
            wi, hi, ci, filtered = png.read_filtered(path)
            if (wi, hi, ci) != (w, h, ch):
                raise RefidHipError(f"load_png_frames: {path} is {hi}x{wi}x{ci}, {paths[0]} is {h}x{w}x{ch}: the files of a "
                                    "sequence must share (H, W, channels)")
            rows[...] = filtered

        def launch(first, n, host, dev):
            bands = png.find_bands(host[0][:, :, 0].numpy())
            ops.png_unfilter(dev[0], n, h, w, ch, out=out[first:first + n], bands=bands)

        return out, [((h, 1 + w * ch), torch.uint8)], fill, launch

    return _load_staged("load_png_frames", paths, device, workers, frames_per_launch, plan)


def _jpeg_sources(sources):
    """[(name, path or bytes)] of ``load_jpeg_frames``'s ``sources``."""
    import glob
    if isinstance(sources, (str, os.PathLike)):
        if os.path.isdir(sources):
            sources = sorted(glob.glob(os.path.join(sources, "*.jpg")) + glob.glob(os.path.join(sources, "*.jpeg")))
        else:
            sources = [sources]
    out = []
    for k, s in enumerate(sources):
        if isinstance(s, (bytes, bytearray, memoryview)):
            out.append((f"frame {k} ({len(s)} bytes)", bytes(s)))
        else:
            out.append((os.fspath(s), os.fspath(s)))
    return out


def load_jpeg_frames(sources, device=None, workers=8, frames_per_launch=8):
    """Baseline JPEG key frames of one size -> uint8 (N, H, W, 3) RGB on the device, a grey file replicated to three channels:
    what ``SequenceAssembler.load`` takes, and byte for byte what libjpeg (PIL) decodes.  ``sources``: paths in order, byte
    strings in order (the frames of ``video.read_mjpeg_avi``), or a directory (its ``*.jpg`` / ``*.jpeg`` sorted by name).
    ``workers`` threads (at most ``PNG_WORKERS_MAX``) read the files and undo their Huffman coding (``jpeg.entropy_decode``:
    the library call releases the GIL) straight into one of two pinned staging buffers of coefficients and tables; every
    chunk of ``frames_per_launch`` frames is uploaded without blocking and decoded by one ``refid_jpeg_decode``
    (csrc/jpeg_decode.hip) on the current stream while the pool works on the next chunk.  A staging buffer is written again
    only after the event behind its last upload has completed.  Files that differ in (H, W, components, sampling):
    RefidHipError naming the first one; a file the decoder refuses (include/refid_hip.h lists what): RefidHipError with its
    name and the library's message.  Does not synchronise at the end."""
    from . import jpeg, ops
    items = _jpeg_sources(sources)

    def read(item):
        name, src = item
        if isinstance(src, bytes):
            return src
        with open(src, "rb") as f:
            return f.read()

    def probe(item, data):
        try:
            return jpeg.probe(data)
        except RefidHipError as e:
            raise RefidHipError(f"load_jpeg_frames: {item[0]}: {e}") from None

    def plan(device):
        first = probe(items[0], read(items[0]))
        h, w, comps, sampling, total = first.height, first.width, first.components, first.sampling, first.total_blocks
        out = torch.empty((len(items), h, w, 3), dtype=torch.uint8, device=device)

        def fill(item, coefs, quant):
            data = read(item)
            info = probe(item, data)
            if info[:4] != first[:4]:
                raise RefidHipError(f"load_jpeg_frames: {item[0]} is {info.height}x{info.width}, {info.components} components, sampling "
                                    f"{info.sampling}; {items[0][0]} is {h}x{w}, {comps}, {sampling}: the files of a sequence must share "
                                    "(H, W, components, sampling)")
            try:
                jpeg.entropy_decode(data, info, coefs, quant.view(np.uint16))
            except RefidHipError as e:
                raise RefidHipError(f"load_jpeg_frames: {item[0]}: {e}") from None

        def launch(first_frame, n, host, dev):
            ops.jpeg_decode(dev[0], dev[1], n, h, w, sampling, out=out[first_frame:first_frame + n])

        return out, [((total, 64), torch.int16), ((comps, 64), torch.int16)], fill, launch

    return _load_staged("load_jpeg_frames", items, device, workers, frames_per_launch, plan)


def load_key_frames(path, device=None, workers=8, frames_per_launch=8):
    """The key frames of ``path`` -> uint8 (N, H, W, 3) RGB on the device: a directory of PNGs (``load_png_frames``), a
    directory of JPEGs (``load_jpeg_frames``), or a Motion-JPEG ``*.avi`` (``video.read_mjpeg_avi``, then ``load_jpeg_frames``
    on its frames; the parts ``stem.part002.avi`` ... of a split video follow in order).  A directory that holds both kinds
    of file, or neither: RefidHipError."""
    import glob
    from . import video
    path = os.fspath(path)
    kw = dict(device=device, workers=workers, frames_per_launch=frames_per_launch)
    if os.path.isdir(path):
        pngs = sorted(glob.glob(os.path.join(path, "*.png")))
        jpgs = [name for name, _ in _jpeg_sources(path)]
        if pngs and jpgs:
            raise RefidHipError(f"load_key_frames: {path} holds both PNG ({len(pngs)}) and JPEG ({len(jpgs)}) files: keep one kind")
        if not pngs and not jpgs:
            raise RefidHipError(f"load_key_frames: no *.png, *.jpg or *.jpeg under {path}")
        return load_png_frames(pngs, **kw) if pngs else load_jpeg_frames(jpgs, **kw)
    if path.lower().endswith(".avi"):
        frames, part = [], 1
        while part == 1 or os.path.exists(video.part_path(path, part)):
            try:
                frames += video.read_mjpeg_avi(video.part_path(path, part))[1]
            except (OSError, ValueError) as e:
                raise RefidHipError(f"load_key_frames: {e}") from None
            part += 1
        if not frames:
            raise RefidHipError(f"load_key_frames: {path} holds no frames")
        return load_jpeg_frames(frames, **kw)
    raise RefidHipError(f"load_key_frames: {path} is neither a directory of PNG or JPEG files nor an .avi file")


def _round_up(v, multiple):
    return (v + multiple - 1) // multiple * multiple


class SequenceAssembler:
    """``{'lq', 'voxel'}`` for frame pairs of one resident sequence (csrc/sequence.hip), in the layouts of
    ``DeviceBatchAssembler``: ``layout='sharp'``: n+1 bins, lq (P, 2, 3, h, w); ``layout='blur'``: 2m+n+1 bins, lq
    (P, 6+2(m-1), h, w) = frame[left] | bins 1..m-1 | frame[right] | bins m+2+n..; voxel (P, bins-1, 2, h, w).
    ``layout='single'`` (``m`` and ``n`` are not used): ``num_bins`` bins, one blurry frame per item (``left``; ``right`` is
    not read): lq (P, 3, h, w), voxel (P, num_bins, h, w) = the plain bins after ``voxel_norm`` unless ``norm_voxel=False``;
    the statistics are taken over the unpadded frame, and an item without spread comes out all zeros.  (h, w) is the frame
    size rounded up to ``multiple`` (default 8, single layout 4): image channels replicate the last row / column there,
    voxel channels are zero.  Everything runs on the current stream; the cached scratch and pair table are ordered by that
    stream only: use one assembler per stream."""

    def __init__(self, m=None, n=None, layout="sharp", multiple=None, device=None, num_bins=6, norm_voxel=True):
        if layout not in ("blur", "sharp", "single"):
            raise RefidHipError(f"SequenceAssembler: unknown layout {layout!r} ('blur', 'sharp' or 'single')")
        from . import ops
        self.layout = layout
        self.norm_voxel = bool(norm_voxel)
        if layout == "single":
            self.m = self.n = self._layout = None
            self.bins = ops.single_bins(num_bins)
        else:
            if m is None or n is None:
                raise RefidHipError(f"SequenceAssembler: layout {layout!r} needs m and n")
            self.m, self.n = int(m), int(n)
            self._layout = _lib.LAYOUT_BLUR if layout == "blur" else _lib.LAYOUT_SHARP
            self.bins = ops.assemble_bins(self.m, self.n, self._layout)
        self.multiple = int((4 if layout == "single" else 8) if multiple is None else multiple)
        if self.multiple < 1:
            raise RefidHipError(f"SequenceAssembler: multiple {multiple} must be >= 1")
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise RefidHipError("SequenceAssembler: a GPU device is required (the HIP path has no CPU fallback)")
        self.frames = self.events = None
        self._cache = GeometryCache(self.device, self.bins, layout == "single" and self.norm_voxel)    # keys (P, H, W)
        self._last = None                     # descriptor and host table of the last call: lets a test or benchmark relaunch it

    def load(self, frames, events, bgr=False):
        """Uploads the sequence once: ``frames`` uint8 (N, H, W, 3), ``events`` float32 (E, 4) rows [t, x, y, p] (E may be
        0); numpy arrays or tensors, host or device.  ``bgr``: the frames are BGR as cv2 decodes them."""
        frames = torch.as_tensor(frames) if not torch.is_tensor(frames) else frames
        events = torch.as_tensor(events) if not torch.is_tensor(events) else events
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
            raise RefidHipError(f"SequenceAssembler.load: frames must be uint8 (N, H, W, 3), got {frames.dtype} "
                                f"{tuple(frames.shape)}")
        if events.dtype != torch.float32 or events.dim() != 2 or events.shape[1] != 4:
            raise RefidHipError(f"SequenceAssembler.load: events must be float32 (E, 4) rows [t, x, y, p], got "
                                f"{events.dtype} {tuple(events.shape)}")
        self.frames = frames.contiguous().to(self.device, non_blocking=True)
        self.events = events.contiguous().to(self.device, non_blocking=True)
        self.bgr = bool(bgr)
        self.height, self.width = int(frames.shape[1]), int(frames.shape[2])
        self.out_h, self.out_w = _round_up(self.height, self.multiple), _round_up(self.width, self.multiple)
        return self

    def assemble(self, pairs, stages=_lib.ASSEMBLE_ALL | _lib.ASSEMBLE_STATS):
        from . import ops
        if self.frames is None:
            raise RefidHipError("SequenceAssembler.assemble: load() a sequence first")
        pairs = list(pairs)
        if not pairs:
            raise RefidHipError("SequenceAssembler.assemble: no pairs")
        count = len(pairs)
        table = (_lib.SeqPair * count)()
        for k, p in enumerate(pairs):
            d = table[k]
            d.left, d.right, d.row0, d.row1 = int(p[0]), int(p[1]), int(p[2]), int(p[3])
            d.first_stamp, d.last_stamp = float(p[4]), float(p[5])
        c = self._cache.upload((count, self.height, self.width), table)
        h, w = self.out_h, self.out_w
        single = self.layout == "single"
        lq, voxel = (torch.empty(shape, dtype=torch.float32, device=self.device)
                     for shape in layout_shapes(self.layout, count, self.bins, self.m, h, w)[:2])
        desc = _lib.SeqSingleDesc() if single else _lib.SeqDesc()
        n_ev = int(self.events.shape[0])
        desc.events, desc.n_events = (self.events.data_ptr() if n_ev else None), n_ev
        desc.frames, desc.n_frames = self.frames.data_ptr(), int(self.frames.shape[0])
        desc.frame_stride, desc.row_pitch = self.height * self.width * 3, self.width * 3
        desc.height, desc.width, desc.bgr = self.height, self.width, int(self.bgr)
        desc.out_h, desc.out_w = h, w
        desc.scratch, desc.lq, desc.voxel = c["scratch"].data_ptr(), lq.data_ptr(), voxel.data_ptr()
        if single:
            desc.items_host, desc.items_dev, desc.n_items = C.addressof(table), c["table_dev"].data_ptr(), count
            desc.bins, desc.norm = self.bins, int(self.norm_voxel)
            desc.parts = c["parts"].data_ptr() if self.norm_voxel else None
            ops.seq_assemble_single(desc, stages)
        else:
            desc.pairs_host, desc.pairs_dev, desc.n_pairs = C.addressof(table), c["table_dev"].data_ptr(), count
            desc.m, desc.n, desc.layout = self.m, self.n, self._layout
            ops.seq_assemble(desc, stages & _lib.ASSEMBLE_ALL)
        self._last = (desc, table)
        cur = torch.cuda.current_stream(self.device)
        for t in (self.frames, self.events):  # (uploaded on another stream: they stay valid until the kernels ran)
            t.record_stream(cur)
        return {"lq": lq, "voxel": voxel}


class _Sink:
    """One output of a runner's uint8 frames (``_SequenceRunner.run`` lists them).  ``add(u8, base, count)``: once per minibatch,
    the frames (count, [T,] H, W, 3) of items base .. base + count - 1; it only queues work on the current stream.  ``close()``:
    in the ``finally`` behind the loop.  ``finish()``: after a loop that did not fail; it may synchronise and sets the result."""

    def __init__(self, runner, names):
        self.runner, self.names, self.what = runner, names, type(runner).__name__

    def paths(self, root, u8, base, count):
        return [p for i in range(count) for p in self.runner._paths(root, self.names[base + i], u8[i])]

    def close(self):
        pass

    def finish(self):
        pass


def _flat(u8):
    return u8.view(-1, *u8.shape[-3:])


class _PngSink(_Sink):
    def __init__(self, runner, names, out_dir, png_filter, png_deflate):
        super().__init__(runner, names)
        self.out_dir, self.writer = out_dir, validation.FrameWriter(runner.device, png_filter=png_filter, png_deflate=png_deflate)

    def add(self, u8, base, count):
        self.writer.dump([(_flat(u8), self.paths(self.out_dir, u8, base, count))])

    def close(self):
        self.writer.close()


class _VideoSink(_Sink):
    def __init__(self, runner, names, pairs, keys, path, fps, quality, subsampling, jpeg_pitch):
        super().__init__(runner, names)
        self.pairs, self.keys = pairs, keys
        self.writer = validation.VideoWriter(runner.device, path, fps, quality, subsampling, jpeg_pitch)

    def add(self, u8, base, count):
        """The frames of a minibatch as they enter the video: the outputs in order; with ``keys`` pair k's left key frame
        (resident, RGB) in front of its outputs, and its right key frame behind them unless the next pair starts on it."""
        if self.keys:
            asm, pairs, parts = self.runner.assembler, self.pairs, []
            key = lambda i: asm.frames[i:i + 1].flip(-1) if asm.bgr else asm.frames[i:i + 1]      # noqa: E731
            for i in range(count):
                p = pairs[base + i]
                parts += [key(p[0]), u8[i].reshape(-1, *u8.shape[-3:])]
                if base + i + 1 >= len(pairs) or pairs[base + i + 1][0] != p[1]:
                    parts.append(key(p[1]))
            u8 = torch.cat(parts, dim=0)
        self.writer.add(_flat(u8))

    def close(self):
        self.writer.close()
        self.runner.video_paths = self.writer.paths


class _NiqeSink(_Sink):
    def __init__(self, runner, names, model):
        super().__init__(runner, names)
        niqe.cropped_size(runner.assembler.height, runner.assembler.width)        # a frame without one 96x96 block raises here
        self.model, self.sums_pin, self.per_item = model, None, 0                 # pinned, sized at the first minibatch

    def add(self, u8, base, count):
        sums = niqe.moments(_flat(u8), self.model)
        if self.sums_pin is None:
            self.per_item = sums.shape[0] // count
            self.sums_pin = torch.empty((len(self.names) * self.per_item,) + tuple(sums.shape[1:]), dtype=sums.dtype).pin_memory()
        self.sums_pin[base * self.per_item:][:sums.shape[0]].copy_(sums, non_blocking=True)

    def finish(self):
        torch.cuda.current_stream(self.runner.device).synchronize()               # the last sums have arrived
        scores = niqe.finish(self.sums_pin.numpy(), self.model)
        self.runner.niqe_scores = [(self.names[i // self.per_item], i % self.per_item, sc) for i, sc in enumerate(scores)]


class _ScoreSink(_Sink):
    def __init__(self, runner, names, gt, scorer):
        super().__init__(runner, names)
        self.scorer, self.scored = score.FrameScorer() if scorer is None else scorer, 0
        self.gt_dir = os.fspath(gt) if isinstance(gt, (str, os.PathLike)) else None
        self.gt_all = None
        if self.gt_dir is None:                # the frames themselves, uploaded once; a directory's PNGs are decoded per minibatch
            H, W = runner.assembler.height, runner.assembler.width
            gt = torch.as_tensor(gt) if not torch.is_tensor(gt) else gt
            if gt.dtype != torch.uint8 or gt.dim() != 4 or tuple(gt.shape[1:]) != (H, W, 3):
                raise RefidHipError(f"{self.what}.run: gt must be a directory or uint8 (frames, {H}, {W}, 3), got {gt.dtype} "
                                    f"{tuple(gt.shape)}")
            self.gt_all = gt.contiguous().to(runner.device, non_blocking=True)

    def add(self, u8, base, count):
        flat = _flat(u8)
        if self.gt_dir is not None:
            gpaths = self.paths(self.gt_dir, u8, base, count)
            for p in gpaths:
                if not os.path.isfile(p):
                    raise RefidHipError(f"{self.what}.run: no ground truth {p}")
            g = load_png_frames(gpaths, device=self.runner.device, frames_per_launch=len(gpaths))
            if g.shape != flat.shape:
                raise RefidHipError(f"{self.what}.run: the ground truth {gpaths[0]} is {g.shape[1]}x{g.shape[2]}, the "
                                    f"output {flat.shape[1]}x{flat.shape[2]}")
        else:
            g = self.gt_all[self.scored:self.scored + flat.shape[0]]
            if g.shape[0] != flat.shape[0]:
                raise RefidHipError(f"{self.what}.run: gt holds {self.gt_all.shape[0]} frames, fewer than the outputs")
        self.scorer.add(flat, g)
        self.scored += flat.shape[0]

    def finish(self):
        if self.gt_all is not None and self.scored != self.gt_all.shape[0]:
            raise RefidHipError(f"{self.what}.run: gt holds {self.gt_all.shape[0]} frames for {self.scored} outputs")
        sc = self.scorer.finish()               # the one synchronisation, after the loop
        each = self.scored // len(self.names)
        self.runner.scores = [(self.names[i // each], i % each, score.Scores(*(None if col is None else col[i] for col in sc)))
                              for i in range(self.scored)]


class _SequenceRunner:
    """What ``SequenceInterpolator`` and ``SequenceDeblurrer`` share: upload the sequence once, assemble minibatch k+1 on a
    side stream while minibatch k runs, crop back to (H, W), quantise with ``metrics.val_tail`` and hand the uint8 frames to
    ``validation.FrameWriter``.  A subclass sets ``net``, ``assembler``, ``max_minibatch``, ``device`` and ``stream`` and
    gives ``_forward(batch)`` -> (P, ..., 3, h, w) and ``_paths(out_dir, name, u8_item)`` -> one path per frame of an item.

    ``niqe``: a ``niqe.NiqeModel``.  Every minibatch's uint8 frames then also go through the NIQE moments kernel
    (csrc/niqe.hip) on the current stream and the few sums per block are copied, non-blocking, into one pinned buffer; the
    host finish of all frames runs after the loop, which gains no synchronisation.  ``niqe_scores`` then holds
    ``(name, frame index, score)`` per frame, in output order (None when ``niqe`` was not given).

    ``gt``: ground truth for the output frames, which are then scored against it while they are resident
    (``score.FrameScorer``, csrc/score.hip), again without a synchronisation in the loop: a directory that holds a PNG of
    the name of every output frame (decoded on the GPU per minibatch), or uint8 (all output frames, H, W, 3) RGB in output
    order (uploaded once).  ``score``: the ``FrameScorer`` to use -- its ``crop_border`` and which scores it takes; default
    ``FrameScorer()``: PSNR and the 3-D SSIM, uncropped.  ``scores`` then holds ``(name, frame index, score.Scores)`` per
    frame, a ``Scores`` field being None for what was not asked for (``scores`` is None without ``gt``)."""

    niqe_scores = scores = video_paths = None

    def run(self, frames, events, pairs, out_dir=None, names=None, keep=False, bgr=False, niqe=None, png_filter="none",
            png_deflate="host", gt=None, score=None, video=None, video_fps=30, video_quality=90, video_subsampling="420",
            video_keys=None, jpeg_pitch=None):
        what = type(self).__name__
        self.niqe_scores = self.scores = self.video_paths = None
        png_filter = validation.check_png_filter(png_filter, f"{what}.run: png_filter")
        png_deflate = validation.check_png_deflate(png_deflate, f"{what}.run: png_deflate")
        if video is not None:
            validation.check_video_options(video_fps, video_quality, video_subsampling, jpeg_pitch, f"{what}.run")
            sharp = self.assembler.layout == "sharp"
            if video_keys and not sharp:
                raise RefidHipError(f"{what}.run: video_keys needs sharp key frames (layout 'sharp'), not {self.assembler.layout!r}")
            video_keys = sharp if video_keys is None else bool(video_keys)
        pairs = list(pairs)
        if not pairs:
            raise RefidHipError(f"{what}.run: no pairs")
        if names is None:
            names = [f"{p[0]:06d}" for p in pairs]
        if len(names) != len(pairs):
            raise RefidHipError(f"{what}.run: {len(names)} names for {len(pairs)} pairs")
        self._load(frames, events, bgr)
        sinks = [None if out_dir is None else _PngSink(self, names, out_dir, png_filter, png_deflate),
                 None if video is None else _VideoSink(self, names, pairs, video_keys, video, video_fps, video_quality,
                                                       video_subsampling, jpeg_pitch),
                 None if niqe is None else _NiqeSink(self, names, niqe),
                 None if gt is None else _ScoreSink(self, names, gt, score)]
        sinks = [s for s in sinks if s is not None]         # those asked for, in the order their work is queued per minibatch
        if gt is None and score is not None:
            raise RefidHipError(f"{what}.run: score= needs gt=")
        chunks = [pairs[i:i + self.max_minibatch] for i in range(0, len(pairs), self.max_minibatch)]
        kept = []
        outputs = self._outputs(chunks)
        try:
            with torch.no_grad():
                for k, u8 in enumerate(outputs):
                    for sink in sinks:
                        sink.add(u8, k * self.max_minibatch, len(chunks[k]))
                    if keep:
                        kept.append(u8)
        finally:
            outputs.close()                                # (the generator's own ``finally`` runs now, if it had started)
            with contextlib.ExitStack() as closing:        # (last in, first out) in the sinks' order, each even if another raises
                for sink in reversed(sinks):
                    closing.callback(sink.close)
        for sink in sinks:
            sink.finish()
        return torch.cat(kept, dim=0).cpu().numpy() if keep else None

    def _load(self, frames, events, bgr):
        """Makes the sequence resident; after it ``assembler`` has ``frames`` (device), ``bgr``, ``height``, ``width``, ``layout``."""
        self.assembler.load(frames, events, bgr=bgr)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))       # the upload was issued on the current stream

    def _outputs(self, chunks):
        """Yields the uint8 RGB frames (P, [T,] H, W, 3) of one chunk of items after the other, on the current stream."""
        asm, side = self.assembler, self.stream
        cur = torch.cuda.current_stream(self.device)

        def preload(k):
            if k >= len(chunks):
                return None
            with torch.cuda.stream(side):
                return asm.assemble(chunks[k])

        was_training = self.net.training
        self.net.eval()
        try:
            nxt = preload(0)
            for k, chunk in enumerate(chunks):
                cur.wait_stream(side)
                batch = nxt
                for v in batch.values():
                    v.record_stream(cur)
                nxt = preload(k + 1)
                out = self._forward(batch)
                yield metrics.val_tail(out[..., :asm.height, :asm.width], bgr=False).pred_u8       # (P, [T,] H, W, 3)
        finally:
            self.net.train(was_training)
            cur.wait_stream(side)


class SequenceInterpolator(_SequenceRunner):
    """Runs ``net`` over the frame pairs of a sequence.  ``run`` uploads the sequence once, assembles minibatch k+1 on a
    side stream while minibatch k runs, and turns every output into uint8 RGB frames of the original (H, W).  The
    minibatch composition is part of the contract: pairs [0, max_minibatch), [max_minibatch, 2 max_minibatch), ... go
    through ``net(x=lq, event=voxel)`` together, under ``eval()`` / ``no_grad()``."""

    def __init__(self, net, m, n, layout="sharp", max_minibatch=2):
        self.net = net
        self.max_minibatch = int(max_minibatch)
        if self.max_minibatch < 1:
            raise RefidHipError(f"SequenceInterpolator: max_minibatch {max_minibatch} must be >= 1")
        if not hasattr(net, "num_encoders"):
            raise RefidHipError("SequenceInterpolator: the network has no num_encoders (the padding multiple is taken from it)")
        self.device = next(net.parameters()).device
        self.assembler = SequenceAssembler(m, n, layout, multiple=1 << int(net.num_encoders), device=self.device)
        self.stream = torch.cuda.Stream(device=self.device)

    def run(self, frames, events, pairs, out_dir=None, names=None, keep=False, bgr=False, niqe=None, png_filter="none",
            png_deflate="host", gt=None, score=None, video=None, video_fps=30, video_quality=90, video_subsampling="420",
            video_keys=None, jpeg_pitch=None):
        """``frames`` uint8 (N, H, W, 3), ``events`` float32 (E, 4), ``pairs`` from ``make_pairs``.  With ``out_dir`` frame f
        of pair k goes to ``{out_dir}/{names[k]}_{f:02d}.png`` (default name: the left key frame's index, six digits, as
        the validation dumps are named).  ``keep=True`` returns the uint8 frames (P, T, H, W, 3) on the host, else None.
        ``niqe``: a ``NiqeModel``; ``niqe_scores`` then holds (name, f, score) per output frame.  ``png_filter``: 'none' or
        'adaptive' (``validation.FrameWriter``): the same pixels in smaller files.  ``png_deflate``: 'host' or 'device'
        (the PNGs' zlib streams come from the GPU, ``ops.png_deflate``): the same pixels again.  ``gt`` / ``score``: ground
        truth to score the outputs against (``_SequenceRunner``): a directory of ``{names[k]}_{f:02d}.png`` or the uint8
        frames; ``scores`` then holds (name, f, ``score.Scores``) per output frame.
        ``video``: a path; the output frames then also go, in output order, into one Motion-JPEG AVI file there
        (``validation.VideoWriter``: baseline JPEG frames from the GPU, csrc/jpeg.hip; ``video_paths`` lists the file and
        its parts) -- independent of ``out_dir``: either, both or neither.  ``video_fps``, ``video_quality`` 1 .. 100,
        ``video_subsampling`` '420' or '444', ``jpeg_pitch`` as ``VideoWriter`` takes it.  ``video_keys``: the resident key
        frames enter the video too (default: yes for layout 'sharp', no otherwise; True elsewhere raises) -- pair k's left
        key frame in front of its outputs, its right key frame behind them when the next pair does not start on it or
        there is none -- so that a run of consecutive pairs is a gap-free slow-motion clip."""
        return super().run(frames, events, pairs, out_dir=out_dir, names=names, keep=keep, bgr=bgr, niqe=niqe,
                           png_filter=png_filter, png_deflate=png_deflate, gt=gt, score=score, video=video, video_fps=video_fps,
                           video_quality=video_quality, video_subsampling=video_subsampling, video_keys=video_keys,
                           jpeg_pitch=jpeg_pitch)

    def _forward(self, batch):
        return self.net(x=batch["lq"], event=batch["voxel"])

    def _paths(self, out_dir, name, u8_item):
        return [os.path.join(out_dir, f"{name}_{f:02d}.png") for f in range(u8_item.shape[0])]


class SequenceDeblurrer(_SequenceRunner):
    """Runs a single-image deblurring ``net`` (``SingleMultiConnectEVHINet``: ``net(x, event)`` returns a list whose last
    element is the output) over the blurry frames of a sequence, as ``SequenceInterpolator`` does for pairs: one upload,
    assembly of minibatch k+1 (``SequenceAssembler(layout='single')``, padded to ``net.size_multiple``) on a side stream
    while minibatch k runs, ``eval()`` / ``no_grad()``, the minibatch composition [0, mb), [mb, 2mb), ... as part of the
    contract.  ``crop_size``: every item goes through ``tiling.tiled_forward`` on the padded frame instead (tiles in
    minibatches of ``max_minibatch``); half-instance-norm statistics are then per tile, so the output differs from the
    whole-frame one by design."""

    def __init__(self, net, num_bins, max_minibatch=1, crop_size=None, norm_voxel=True):
        self.net = net
        self.max_minibatch = int(max_minibatch)
        if self.max_minibatch < 1:
            raise RefidHipError(f"SequenceDeblurrer: max_minibatch {max_minibatch} must be >= 1")
        if not hasattr(net, "size_multiple"):
            raise RefidHipError("SequenceDeblurrer: the network has no size_multiple (the padding multiple is taken from it)")
        self.crop_size = None if crop_size is None else int(crop_size)
        if self.crop_size is not None and (self.crop_size < 1 or self.crop_size % int(net.size_multiple)):
            raise RefidHipError(f"SequenceDeblurrer: crop_size {crop_size} must be a positive multiple of "
                                f"net.size_multiple ({net.size_multiple})")
        self.device = next(net.parameters()).device
        self.assembler = SequenceAssembler(layout="single", num_bins=num_bins, norm_voxel=norm_voxel,
                                           multiple=int(net.size_multiple), device=self.device)
        self.stream = torch.cuda.Stream(device=self.device)

    def run(self, frames, events, items, out_dir=None, names=None, keep=False, bgr=False, niqe=None, png_filter="none",
            png_deflate="host", gt=None, score=None, video=None, video_fps=30, video_quality=90, video_subsampling="420",
            jpeg_pitch=None):
        """``frames`` uint8 (N, H, W, 3), ``events`` float32 (E, 4), ``items`` from ``make_pairs(t, *frame_windows(...))``.
        With ``out_dir`` item k goes to ``{out_dir}/{names[k]}.png`` (default name: the frame index, six digits).
        ``keep=True`` returns the uint8 frames (P, H, W, 3) on the host, else None.
        ``niqe``: a ``NiqeModel``; ``niqe_scores`` then holds (name, 0, score) per output frame.  ``png_filter``: as for
        ``SequenceInterpolator.run``.  ``gt`` / ``score``: as there, the directory holding ``{names[k]}.png``.  ``video`` and
        its options: as there, the deblurred frames in order (no key frames)."""
        return super().run(frames, events, items, out_dir=out_dir, names=names, keep=keep, bgr=bgr, niqe=niqe,
                           png_filter=png_filter, png_deflate=png_deflate, gt=gt, score=score, video=video, video_fps=video_fps,
                           video_quality=video_quality, video_subsampling=video_subsampling, jpeg_pitch=jpeg_pitch)

    def _forward(self, batch):
        if self.crop_size is None:
            return self.net(x=batch["lq"], event=batch["voxel"])[-1]
        from . import tiling
        return torch.cat([tiling.tiled_forward(self.net, batch["lq"][i:i + 1], batch["voxel"][i:i + 1], self.crop_size,
                                               self.max_minibatch) for i in range(batch["lq"].shape[0])], dim=0)

    def _paths(self, out_dir, name, u8_item):
        return [os.path.join(out_dir, f"{name}.png")]


