"""Image dumps of the validation loop (twoImage_event_recurrent_model.py:435-458) without stalling the GPU.

The uint8 frames that ``metrics.val_tail`` leaves on the device go to one of two pinned host buffers on a side stream;
a small thread pool encodes and writes the PNGs.  The buffers alternate, so the copy and the encoding of item k overlap
the forward pass of item k+1.  A worker reads a pinned buffer only after the copy's event has completed, and a buffer
is reused only after every job that reads it has finished.  No fp32 frame leaves the device.

``png_filter='adaptive'``: the frames are first filtered on the device (``ops.png_filter``, csrc/png_filter.hip: per row the
PNG filter type libpng's heuristic picks) on the current stream; the filtered rows -- one byte per row more than the
frames -- take the frames' place in the pinned buffers and the workers only deflate them (``png.write_png_rows``).  The
files hold the same pixels; they are smaller and cheaper to deflate on anything but flat frames.

``png_deflate='device'``: the rows (filter 0 with ``png_filter='none'``, adaptive otherwise) are also deflated on the device
(``ops.png_deflate``, csrc/png_deflate.hip: Huffman codes per block, no matches) on the current stream; the finished zlib
streams and their lengths take the rows' place in the pinned buffers -- the whole pitch is copied, so nothing waits for a
length -- and the workers only take the CRC and write the file (``png.write_png_stream``).  The files hold the same
pixels as the host route's; their bytes differ (another block structure).

``VideoWriter`` is the same machinery for one Motion-JPEG AVI file instead of a PNG per frame: ``add(frames)`` encodes the
uint8 frames to baseline JPEG files on the device (``ops.jpeg_encode``, csrc/jpeg.hip) on the current stream, the files and
their lengths travel together into one of two pinned buffers on the side stream -- the whole pitch is copied, so nothing
waits for a length -- and one worker appends them to the container (``video.MjpegAviWriter``) in submission order."""
import threading
from concurrent.futures import ThreadPoolExecutor

import torch

from . import _lib
from .png import write_png, write_png_rows, write_png_stream

PNG_FILTERS = ("none", "adaptive")
PNG_DEFLATES = ("host", "device")


def _check_choice(value, choices, where):
    """``value`` (None, an absent key: the first choice) if it is one of ``choices``; anything else raises, naming ``where``."""
    value = choices[0] if value is None else value
    if value not in choices:
        raise _lib.RefidHipError(f"{where}: {value!r} is not one of {', '.join(choices)}")
    return value


def check_png_filter(value, where="png_filter"):
    """'none' (or None: an absent key) / 'adaptive'; anything else raises, naming ``where``."""
    return _check_choice(value, PNG_FILTERS, where)


def check_png_deflate(value, where="png_deflate"):
    """'host' (or None: an absent key) / 'device'; anything else raises, naming ``where``."""
    return _check_choice(value, PNG_DEFLATES, where)


JPEG_SUBSAMPLINGS = ("420", "444")


def check_video_options(fps=30, quality=90, subsampling="420", jpeg_pitch=None, where="VideoWriter"):
    """(fps, quality, subsampling, jpeg_pitch) as given, or raises naming ``where`` and the option."""
    from .video import fps_fraction
    try:
        fps_fraction(fps)
    except ValueError as ex:
        raise _lib.RefidHipError(f"{where}: video_fps: {ex}") from None
    if type(quality) is not int or not 1 <= quality <= 100:
        raise _lib.RefidHipError(f"{where}: video_quality {quality!r} is not an integer 1 .. 100")
    if subsampling not in JPEG_SUBSAMPLINGS:
        raise _lib.RefidHipError(f"{where}: video_subsampling {subsampling!r} is not one of {', '.join(JPEG_SUBSAMPLINGS)}")
    least = _lib.JPEG_HEADER_BYTES + 2
    if jpeg_pitch is not None and jpeg_pitch != "bound" and (type(jpeg_pitch) is not int or not least <= jpeg_pitch < 2 ** 31):
        raise _lib.RefidHipError(f"{where}: jpeg_pitch {jpeg_pitch!r} is not None, 'bound' or an integer {least} .. 2^31 - 1")
    return fps, quality, subsampling, jpeg_pitch


class _PinnedRelay:
    """What ``FrameWriter`` and ``VideoWriter`` share: a side stream, two pinned host buffers ("slots") that take turns, the
    event behind a slot's copies, and a thread pool whose jobs read a slot once that event has completed.  Per transfer the
    owner calls ``claim()``, launches its device work on the current stream, ``send()``s the results and ``submit()``s the jobs
    that read them, in this order: the overlap rests on it ("Frame outputs")."""

    def __init__(self, device, workers, queue, thread_name_prefix):
        self.stream = torch.cuda.Stream(device)
        self.slots = [dict(buf=None, jobs=[]), dict(buf=None, jobs=[])]
        self.turn = 0
        self.pool = ThreadPoolExecutor(max_workers=workers, thread_name_prefix=thread_name_prefix)
        self.room = threading.BoundedSemaphore(queue)   # jobs submitted and not finished; `submit` blocks beyond that

    def claim(self):
        """Takes the next slot and waits for the jobs of its previous transfer: its buffer may then be overwritten."""
        self.slot = self.slots[self.turn]
        self.turn ^= 1
        self._drain(self.slot)

    def send(self, groups):
        """groups: [[device tensor, ...], ...], all of them one transfer into the claimed slot.  Every tensor is copied,
        non-blocking, on the side stream -- which first waits for the current stream -- to the next multiple of its element
        size (int32 lengths behind uint8 payload: the next multiple of 4); one event is recorded behind the copies.  Returns
        the pinned views in the same nesting; only a job given to ``submit`` may read them."""
        slot, off, views = self.slot, 0, []
        total = sum((t.numel() + 1) * t.element_size() for group in groups for t in group)       # with room to align each
        if slot["buf"] is None or slot["buf"].numel() < total:
            slot["buf"] = torch.empty(total, dtype=torch.uint8).pin_memory()
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            for group in groups:
                views.append([])
                for t in group:
                    size = t.element_size()
                    off = -(-off // size) * size
                    dst = slot["buf"][off:off + t.numel() * size].view(t.dtype).view(t.shape)
                    dst.copy_(t, non_blocking=True)
                    t.record_stream(self.stream)            # the allocator must not hand t's block out before the copy ran
                    views[-1].append(dst)
                    off += t.numel() * size
            self.done = torch.cuda.Event()
            self.done.record(self.stream)
        return views

    def submit(self, job, *args):
        """Runs ``job(*args)`` on the pool once the copies of the last ``send`` have completed; blocks while the queue is full."""
        self.room.acquire()
        self.slot["jobs"].append(self.pool.submit(self._run, self.done, job, args))

    def _run(self, done, job, args):
        try:
            done.synchronize()                              # nothing reads the pinned buffer before its copy has completed
            job(*args)
        finally:
            self.room.release()

    @staticmethod
    def _drain(slot):
        jobs, slot["jobs"] = slot["jobs"], []
        err = None
        for j in jobs:                                      # wait for ALL of them, then re-raise the first failure
            try:
                j.result()
            except BaseException as ex:                     # noqa: BLE001
                err = err or ex
        if err is not None:
            raise err

    def close(self):
        """Joins the pool: every job has run when this returns; the first job's exception is raised here."""
        try:
            for slot in self.slots:
                self._drain(slot)
        finally:
            self.pool.shutdown(wait=True, cancel_futures=True)


class FrameWriter:
    WORKERS = 4              # encoding is zlib (releases the GIL); never sized from the machine's core count
    QUEUE = 32               # jobs submitted and not finished; `dump` blocks beyond that

    def __init__(self, device, level=1, png_filter="none", png_deflate="host"):
        self.level = level
        self.png_filter = check_png_filter(png_filter, "FrameWriter: png_filter")
        self.png_deflate = check_png_deflate(png_deflate, "FrameWriter: png_deflate")
        self.relay = _PinnedRelay(device, self.WORKERS, self.QUEUE, "refid-png")

    def dump(self, batches):
        """batches: [(uint8 device tensor (N, H, W, 3), [N paths])] of ONE item; returns at once."""
        self.relay.claim()                                  # the slot's previous item is written
        routed = [self._route(t, paths) for t, paths in batches]        # the device's share, launched on the current stream
        for (_, paths, width, height), (payload, *lens) in zip(routed, self.relay.send([r[0] for r in routed])):
            payload, lens = payload.numpy(), lens[0].numpy() if lens else None
            for i, path in enumerate(paths):
                self.relay.submit(self._write, payload[i], path, width, None if lens is None else lens[i:i + 1], height)

    def _route(self, t, paths):
        """([what travels], paths, W, H): the frames themselves (W and H None: the host does everything); with
        ``png_filter='adaptive'`` their filtered rows (N, H, 1 + 3W) (H None); with ``png_deflate='device'`` the zlib streams
        (N, pitch) of the rows -- filter 0 or adaptive -- and their lengths (N,).  Frames the filter kernel does not take keep
        the host route."""
        from . import ops
        deflate, fits = self.png_deflate == "device", t.dim() == 4 and t.shape[-1] == 3 and t.shape[2] <= _lib.PNG_FILTER_MAX_WIDTH
        if not fits or not (deflate or self.png_filter == "adaptive"):
            return [t], paths, None, None
        rows = ops.png_filter(t.contiguous(), "adaptive" if self.png_filter == "adaptive" else 0)
        if not deflate:
            return [rows], paths, int(t.shape[2]), None
        return list(ops.png_deflate(rows)), paths, int(t.shape[2]), int(t.shape[1])

    def _write(self, frame, path, width, length, height):
        if length is not None:                              # a zlib stream of the device: its length came with the copy
            write_png_stream(path, frame[:int(length[0])], width, height)
        elif width is None:
            write_png(path, frame, self.level)
        else:                                               # rows the device has filtered
            write_png_rows(path, frame, width, frame.shape[0], self.level)

    def close(self):
        """Joins the pool: every file exists when this returns; a worker's exception is raised here."""
        self.relay.close()


class VideoWriter:
    """One Motion-JPEG AVI file (and ``stem.part002.avi`` ... beyond ``max_bytes``) of the frames given to ``add`` in order.
    ``jpeg_pitch``: the bytes a frame's file may take -- None: the header and 3 bytes per pixel (every natural frame fits),
    'bound': ``refid_jpeg_bound`` (every frame fits), or an integer; a frame that does not fit fails the writer with an
    error that names it.  The file is created at the first ``add`` (the frame size comes with it); ``paths`` lists the
    files once ``close`` has returned."""
    QUEUE = 8                # batches submitted and not appended; `add` blocks beyond that

    def __init__(self, device, path, fps, quality=90, subsampling="420", jpeg_pitch=None, max_bytes=None):
        self.fps, self.quality, self.subsampling, self.jpeg_pitch = check_video_options(fps, quality, subsampling, jpeg_pitch)
        self.path, self.max_bytes = str(path), max_bytes
        self.relay = _PinnedRelay(device, 1, self.QUEUE, "refid-avi")                       # one worker: submission order
        self.avi, self.frames, self.paths, self.failed = None, 0, [], None

    def add(self, frames_u8):
        """frames_u8: uint8 device tensor (N, H, W, 3), RGB; returns at once."""
        from . import ops
        from .video import MjpegAviWriter
        if self.failed is not None:
            raise self.failed
        t = frames_u8.contiguous()
        if self.avi is None:
            if t.dim() != 4:
                raise _lib.RefidHipError(f"VideoWriter: frames must be uint8 (N, H, W, 3), got {tuple(t.shape)}")
            kw = {} if self.max_bytes is None else dict(max_bytes=self.max_bytes)
            self.avi = MjpegAviWriter(self.path, int(t.shape[2]), int(t.shape[1]), self.fps, **kw)
            self.size = tuple(t.shape[1:])
        elif tuple(t.shape[1:]) != self.size:
            raise _lib.RefidHipError(f"VideoWriter: frames of {tuple(t.shape[1:])} in a video of {self.size}")
        self.relay.claim()                                  # the slot's previous batch is appended
        out, lens = ops.jpeg_encode(t, self.quality, self.subsampling, pitch=self.jpeg_pitch)      # on the current stream
        (files, sizes), = self.relay.send([[out, lens]])    # the whole pitch and the lengths: nothing waits for a length
        self.relay.submit(self._append, files.numpy(), sizes.numpy(), self.frames, int(out.shape[1]))
        self.frames += int(out.shape[0])

    def _append(self, files, sizes, first, pitch):
        if self.failed is not None:                         # an earlier batch failed: the order is lost, append nothing more
            return
        try:
            for i in range(files.shape[0]):
                size = int(sizes[i])
                if size < 0:
                    raise _lib.RefidHipError(f"VideoWriter: frame {first + i} needs {-size} bytes, the pitch is {pitch}: "
                                             f"pass jpeg_pitch='bound'")
                self.avi.add(files[i, :size].tobytes())
        except BaseException as ex:                         # noqa: BLE001
            self.failed = ex
            raise

    def close(self):
        """Joins the worker and finishes the container: the files are complete when this returns; a worker's exception is
        raised here (the container is still closed, with the frames in front of the failure)."""
        try:
            self.relay.close()
        finally:
            if self.avi is not None:
                self.paths = self.avi.close()
