"""The host stage of JPEG decode: ``probe`` reads a baseline JPEG file's header, ``entropy_decode`` undoes its Huffman coding
into quantised coefficients (csrc/jpeg_entropy.h, through the library: ctypes calls that release the GIL, touch no GPU API
and work on a machine without one).  ``ops.jpeg_decode`` (csrc/jpeg_decode.hip) turns the coefficients into pixels;
``sequence.load_jpeg_frames`` runs both for a sequence of files.  What is accepted and refused: include/refid_hip.h."""
import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import RefidHipError

GREY, S444, S422, S420 = _lib.JPEG_DEC_GREY, _lib.JPEG_DEC_444, _lib.JPEG_DEC_422, _lib.JPEG_DEC_420
SAMPLINGS = {"grey": GREY, "444": S444, "422": S422, "420": S420}
SAMPLING_NAMES = {v: k for k, v in SAMPLINGS.items()}

Info = collections.namedtuple("Info", "height width components sampling blocks total_blocks restart_interval")


def _buffer(data):
    """(address, length, keep-alive) of bytes-like ``data`` without a copy where it can be had."""
    if isinstance(data, np.ndarray):
        a = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        return a.ctypes.data, a.size, a
    if isinstance(data, bytes):
        return C.cast(C.c_char_p(data), C.c_void_p).value, len(data), data
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    return a.ctypes.data, a.size, a


def _error(what):
    return RefidHipError(f"{what}: {_lib.lib().refid_last_error().decode('utf-8', 'replace')}")


def _c_info(info):
    c = _lib.JpegInfo(height=info.height, width=info.width, components=info.components, sampling=SAMPLINGS[info.sampling],
                      total_blocks=info.total_blocks, restart_interval=info.restart_interval)
    for k in range(3):
        c.blocks[k] = info.blocks[k]
    return c


def probe(data):
    """``Info`` of a JPEG byte string: height, width, components (1 or 3), sampling ('grey', '444', '422', '420'), blocks per
    component (3 entries), their sum, the restart interval in MCUs (0: none).  A file the decoder refuses: RefidHipError
    with the library's message, which begins ``jpeg_decode:``."""
    addr, n, keep = _buffer(data)
    c = _lib.JpegInfo()
    if _lib.lib().refid_jpeg_probe(addr, n, C.byref(c)) != 0:
        raise _error("jpeg.probe")
    return Info(c.height, c.width, c.components, SAMPLING_NAMES[c.sampling], tuple(c.blocks), c.total_blocks, c.restart_interval)


def entropy_decode(data, info, coefs_out, quant_out):
    """Decodes one file whose header gives exactly ``info`` (a ``probe`` result) into ``coefs_out`` -- a C-contiguous int16
    numpy array of info.total_blocks * 64 elements: the components back to back, blocks in raster order of the plane padded
    to whole MCUs, natural coefficient order -- and ``quant_out``, uint16, info.components * 64 elements in natural order.
    The library writes straight into the arrays' memory (pinned staging buffers, in ``load_jpeg_frames``).  Safe from several
    threads at once.  A refused file: RefidHipError with the library's message; the arrays' contents are then unspecified."""
    for a, dtype, size, name in ((coefs_out, np.int16, info.total_blocks * 64, "coefs_out"), (quant_out, np.uint16, info.components * 64, "quant_out")):
        if not isinstance(a, np.ndarray) or a.dtype != dtype or a.size != size or not a.flags.c_contiguous or not a.flags.writeable:
            raise RefidHipError(f"jpeg.entropy_decode: {name} must be a writeable C-contiguous {np.dtype(dtype).name} array of {size} elements")
    addr, n, keep = _buffer(data)
    c = _c_info(info)
    if _lib.lib().refid_jpeg_entropy_decode(addr, n, C.byref(c), coefs_out.ctypes.data, quant_out.ctypes.data) != 0:
        raise _error("jpeg.entropy_decode")
