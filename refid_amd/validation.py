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


def check_png_filter(value, where="png_filter"):
    """'none' (or None: an absent key) / 'adaptive'; anything else raises, naming ``where``."""
    value = "none" if value is None else value
    if value not in PNG_FILTERS:
        raise _lib.RefidHipError(f"{where}: {value!r} is not one of {', '.join(PNG_FILTERS)}")
    return value


def check_png_deflate(value, where="png_deflate"):
    """'host' (or None: an absent key) / 'device'; anything else raises, naming ``where``."""
    value = "host" if value is None else value
    if value not in PNG_DEFLATES:
        raise _lib.RefidHipError(f"{where}: {value!r} is not one of {', '.join(PNG_DEFLATES)}")
    return value


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


class FrameWriter:
    WORKERS = 4              # encoding is zlib (releases the GIL); never sized from the machine's core count
    QUEUE = 32               # jobs submitted and not finished; `dump` blocks beyond that

    def __init__(self, device, level=1, png_filter="none", png_deflate="host"):
        self.level = level
        self.png_filter = check_png_filter(png_filter, "FrameWriter: png_filter")
        self.png_deflate = check_png_deflate(png_deflate, "FrameWriter: png_deflate")
        self.stream = torch.cuda.Stream(device)
        self.slots = [dict(buf=None, jobs=[]), dict(buf=None, jobs=[])]
        self.turn = 0
        self.pool = ThreadPoolExecutor(max_workers=self.WORKERS, thread_name_prefix="refid-png")
        self.room = threading.BoundedSemaphore(self.QUEUE)

    def dump(self, batches):
        """batches: [(uint8 device tensor (N, H, W, 3), [N paths])] of ONE item; returns at once."""
        slot = self.slots[self.turn]
        self.turn ^= 1
        self._drain(slot)                                   # its previous item is written: the buffer may be overwritten
        # (tensor, paths, width, (lens, height)): the width marks rows the device has filtered, the last entry zlib streams it
        # has deflated as well; both launched here on the current stream
        if self.png_deflate == "device":
            batches = [self._deflated(t, paths, self.png_filter) for t, paths in batches]
        else:
            batches = [self._filtered(t, paths) if self.png_filter == "adaptive" else (t, paths, None, None) for t, paths in batches]
        total = sum(t.numel() + (0 if deflated is None else 4 * deflated[0].numel() + 4) for t, _, _, deflated in batches)
        if slot["buf"] is None or slot["buf"].numel() < total:
            slot["buf"] = torch.empty(total, dtype=torch.uint8).pin_memory()
        self.stream.wait_stream(torch.cuda.current_stream())
        views, off = [], 0
        with torch.cuda.stream(self.stream):
            for t, paths, width, deflated in batches:
                dst = slot["buf"][off:off + t.numel()].view(t.shape)
                dst.copy_(t, non_blocking=True)
                t.record_stream(self.stream)                # the allocator must not hand t's block out before the copy ran
                off += t.numel()
                sizes = None
                if deflated is not None:                    # the streams' lengths, behind them at the next multiple of 4
                    lens, height = deflated
                    off = (off + 3) & ~3
                    pinned = slot["buf"][off:off + 4 * lens.numel()].view(torch.int32)
                    pinned.copy_(lens, non_blocking=True)
                    lens.record_stream(self.stream)
                    off += 4 * lens.numel()
                    sizes = (pinned.numpy(), height)
                views.append((dst.numpy(), paths, width, sizes))
            done = torch.cuda.Event()
            done.record(self.stream)
        for frames, paths, width, sizes in views:
            for i, path in enumerate(paths):
                self.room.acquire()
                stream = None if sizes is None else (sizes[0][i:i + 1], sizes[1])
                slot["jobs"].append(self.pool.submit(self._job, done, frames[i], path, width, stream))

    @staticmethod
    def _filtered(t, paths):
        """(filtered rows (N, H, 1 + 3W) of t, paths, W), launched on the current stream; frames wider than the kernel
        takes stay as they are (filter 0 on the host)."""
        from . import ops
        if t.dim() != 4 or t.shape[-1] != 3 or t.shape[2] > _lib.PNG_FILTER_MAX_WIDTH:
            return t, paths, None, None
        return ops.png_filter(t.contiguous(), "adaptive"), paths, int(t.shape[2]), None

    @staticmethod
    def _deflated(t, paths, png_filter):
        """(zlib streams (N, pitch) of t's rows, paths, W, (lens (N,), H)), launched on the current stream: the rows are
        filter 0 or adaptive.  Frames the filter kernel does not take keep the host route."""
        from . import ops
        if t.dim() != 4 or t.shape[-1] != 3 or t.shape[2] > _lib.PNG_FILTER_MAX_WIDTH:
            return t, paths, None, None
        rows = ops.png_filter(t.contiguous(), "adaptive" if png_filter == "adaptive" else 0)
        out, lens = ops.png_deflate(rows)
        return out, paths, int(t.shape[2]), (lens, int(t.shape[1]))

    def _job(self, done, frame, path, width=None, stream=None):
        try:
            done.synchronize()                              # nothing reads the pinned buffer before its copy has completed
            if stream is not None:                          # a zlib stream of the device: its length came with the copy
                write_png_stream(path, frame[:int(stream[0][0])], width, stream[1])
            elif width is None:
                write_png(path, frame, self.level)
            else:                                           # rows the device has filtered
                write_png_rows(path, frame, width, frame.shape[0], self.level)
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
        """Joins the pool: every file exists when this returns; a worker's exception is raised here."""
        try:
            for slot in self.slots:
                self._drain(slot)
        finally:
            self.pool.shutdown(wait=True, cancel_futures=True)


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
        self.stream = torch.cuda.Stream(device)
        self.slots = [dict(buf=None, jobs=[]), dict(buf=None, jobs=[])]
        self.turn = 0
        self.pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="refid-avi")      # one worker: submission order
        self.room = threading.BoundedSemaphore(self.QUEUE)
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
        slot = self.slots[self.turn]
        self.turn ^= 1
        self._drain(slot)                                   # its previous batch is appended: the buffer may be overwritten
        out, lens = ops.jpeg_encode(t, self.quality, self.subsampling, pitch=self.jpeg_pitch)      # on the current stream
        n, pitch = int(out.shape[0]), int(out.shape[1])
        at = (out.numel() + 3) & ~3                         # the lengths, behind the files at the next multiple of 4
        total = at + 4 * n
        if slot["buf"] is None or slot["buf"].numel() < total:
            slot["buf"] = torch.empty(total, dtype=torch.uint8).pin_memory()
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            files = slot["buf"][:out.numel()].view(n, pitch)
            files.copy_(out, non_blocking=True)
            out.record_stream(self.stream)                  # the allocator must not hand the block out before the copy ran
            sizes = slot["buf"][at:total].view(torch.int32)
            sizes.copy_(lens, non_blocking=True)
            lens.record_stream(self.stream)
            done = torch.cuda.Event()
            done.record(self.stream)
        self.room.acquire()
        slot["jobs"].append(self.pool.submit(self._job, done, files.numpy(), sizes.numpy(), self.frames, pitch))
        self.frames += n

    def _job(self, done, files, sizes, first, pitch):
        try:
            if self.failed is not None:                     # an earlier batch failed: the order is lost, append nothing more
                return
            done.synchronize()                              # nothing reads the pinned buffer before its copy has completed
            for i in range(files.shape[0]):
                size = int(sizes[i])
                if size < 0:
                    raise _lib.RefidHipError(f"VideoWriter: frame {first + i} needs {-size} bytes, the pitch is {pitch}: "
                                             f"pass jpeg_pitch='bound'")
                self.avi.add(files[i, :size].tobytes())
        except BaseException as ex:                         # noqa: BLE001
            self.failed = ex
            raise
        finally:
            self.room.release()

    _drain = staticmethod(FrameWriter._drain)

    def close(self):
        """Joins the worker and finishes the container: the files are complete when this returns; a worker's exception is
        raised here (the container is still closed, with the frames in front of the failure)."""
        try:
            for slot in self.slots:
                self._drain(slot)
        finally:
            self.pool.shutdown(wait=True, cancel_futures=True)
            if self.avi is not None:
                self.paths = self.avi.close()
