"""CPU-only: the JPEG entry points of include/refid_hip.h -- the library exports refid_jpeg_encode and its three size
functions, the ctypes mirror of refid_jpeg_desc has the header's field order and types, the constants agree with the header
and with tests/jpeg_ref.py, the size functions are the restatement's formulas, the ABI version stays 9 (additive), a bad
descriptor is turned down on the host with a message that names the field, before anything is launched, and the options of
ops.jpeg_encode, validation.VideoWriter and both command lines are checked by name."""
import ctypes
import os
import re

import pytest

import jpeg_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {"int32_t": ctypes.c_int32, "uint8_t": ctypes.c_uint8, "uint32_t": ctypes.c_uint32}


def _header():
    with open(os.path.join(ROOT, "include", "refid_hip.h")) as f:
        return f.read()


def _fields(struct_name):
    """[(name, ctypes type)] of a struct of the header, parsed as test_abi_symbols_png_deflate.py does: pointers are c_void_p."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct_name, struct_name), _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        mt = re.match(r"^(const\s+)?(uint8_t|uint32_t|int32_t)\s*(.*)$", stmt)
        assert mt, stmt
        for name in mt.group(3).split(","):
            name = name.strip()
            out.append((name.lstrip("*").strip(), ctypes.c_void_p if name.startswith("*") else C_TYPES[mt.group(2)]))
    return out


def test_jpeg_desc_matches_the_header():
    from refid_amd import _lib
    assert _fields("refid_jpeg_desc") == list(_lib.JpegDesc._fields_)
    assert [f[0] for f in _lib.JpegDesc._fields_] == ["frames", "out", "lens", "work", "n_frames", "height", "width", "quality",
                                                     "subsampling", "restart_mcus", "out_pitch"]
    assert ctypes.sizeof(_lib.JpegDesc) == 4 * 8 + 8 * 4                          # four pointers, seven int32 and the padding
    src = _header()
    const = lambda name: int(re.search(r"#define %s (\d+)" % name, src).group(1))       # noqa: E731
    assert const("REFID_JPEG_444") == _lib.JPEG_444 == J.J444 == 0 and const("REFID_JPEG_420") == _lib.JPEG_420 == J.J420 == 1
    assert const("REFID_JPEG_HEADER_BYTES") == _lib.JPEG_HEADER_BYTES == J.HEADER_BYTES == len(J.header(37, 50, 90, J.J420))
    assert const("REFID_JPEG_BLOCK_BITS") == _lib.JPEG_BLOCK_BITS == J.BLOCK_BITS
    longest = lambda codes: max(length for _, length in codes.values())                # noqa: E731
    assert J.BLOCK_BITS == max(map(longest, J.DC_CODES)) + 11 + 63 * (max(map(longest, J.AC_CODES)) + 10)
    decl = re.search(r"int refid_jpeg_encode\((.*?)\);", src, re.S).group(1)
    assert [a.strip() for a in decl.split(",")] == ["const refid_jpeg_desc* d", "void* stream"]
    assert re.search(r"size_t refid_jpeg_header_bytes\(void\);", src)
    assert re.search(r"size_t refid_jpeg_bound\(int32_t height, int32_t width, int32_t subsampling, int32_t restart_mcus\);", src)
    assert re.search(r"size_t refid_jpeg_work_bytes\(int32_t n_frames, int32_t height, int32_t width, int32_t subsampling, "
                     r"int32_t restart_mcus\);", src)
    assert const("REFID_ABI_VERSION") == 9 == _lib.ABI_VERSION


def test_library_exports_the_jpeg_entry_points():
    from refid_amd import _lib, ops, validation, video
    from refid_amd.build import build
    L = ctypes.CDLL(build())
    for name in ("refid_jpeg_encode", "refid_jpeg_header_bytes", "refid_jpeg_bound", "refid_jpeg_work_bytes"):
        assert hasattr(L, name), name
    bound = _lib.lib()
    assert bound.refid_jpeg_encode.argtypes[0]._type_ is _lib.JpegDesc and bound.refid_jpeg_encode.argtypes[1] is ctypes.c_void_p
    for f in (bound.refid_jpeg_header_bytes, bound.refid_jpeg_bound, bound.refid_jpeg_work_bytes):
        assert f.restype is ctypes.c_size_t
    assert bound.refid_abi_version() == 9                                          # additive: the ABI version stays
    assert bound.refid_jpeg_header_bytes() == J.header_bytes() == 625
    assert callable(ops.jpeg_encode) and callable(video.MjpegAviWriter) and callable(video.read_mjpeg_avi)
    assert callable(validation.VideoWriter) and validation.JPEG_SUBSAMPLINGS == ("420", "444")
    assert ops.jpeg_default_pitch(33, 65) == J.default_pitch(33, 65) and ops.JPEG_SUBSAMPLINGS == J.SUBSAMPLINGS


def test_bound_and_work_bytes_are_the_restatements_formulas():
    from refid_amd import _lib
    L = _lib.lib()
    sizes = [(1, 1), (8, 8), (16, 16), (7, 9), (17, 35), (33, 65), (5, 131), (720, 1280), (1080, 1920), (65535, 1), (1, 65535), (4096, 4096)]
    for h, w in sizes:
        for ss in (J.J444, J.J420):
            for restart in (0, 1, 2, 3, 80, 65535):
                want = J.bound(h, w, ss, restart)
                assert L.refid_jpeg_bound(h, w, ss, restart) == want, (h, w, ss, restart)
                assert want >= J.HEADER_BYTES + 2 * (-(-J.BLOCK_BITS * J.geometry(h, w, ss, restart)[3] // 8)) + 2
                for n in (1, 3, 9):
                    assert L.refid_jpeg_work_bytes(n, h, w, ss, restart) == J.work_bytes(n, h, w, ss, restart), (n, h, w, ss, restart)
    assert J.bound(65535, 65535, J.J444, 0) > 2 ** 31 - 1 and L.refid_jpeg_bound(65535, 65535, J.J444, 0) == 0
    assert L.refid_jpeg_work_bytes(1, 65535, 65535, J.J444, 0) == 0
    for h, w, ss, restart in ((0, 8, 0, 0), (8, 0, 0, 0), (-1, 8, 1, 0), (65536, 8, 0, 0), (8, 65536, 1, 0), (8, 8, 2, 0), (8, 8, -1, 0),
                              (8, 8, 0, -1), (8, 8, 1, 65536)):
        assert L.refid_jpeg_bound(h, w, ss, restart) == 0, (h, w, ss, restart)
        assert L.refid_jpeg_work_bytes(1, h, w, ss, restart) == 0, (h, w, ss, restart)
    assert L.refid_jpeg_work_bytes(0, 8, 8, 0, 0) == 0 and L.refid_jpeg_work_bytes(-2, 8, 8, 0, 0) == 0
    assert L.refid_jpeg_work_bytes(2 ** 31 - 1, 64, 64, 0, 1) == 0                  # more workgroups than a grid takes


def test_the_entry_rejects_bad_descriptors_before_any_launch():
    """The argument checks run on the host and launch nothing, so they hold without a GPU (a launch without one would
    return 2, 'launch failed')."""
    from refid_amd import _lib
    L = _lib.lib()
    ok = dict(frames=16, out=4096, lens=64, work=8192, n_frames=2, height=17, width=35, quality=90, subsampling=J.J420, restart_mcus=0,
              out_pitch=J.bound(17, 35, J.J420))
    assert L.refid_jpeg_encode(None, None) == 1 and "descriptor" in L.refid_last_error().decode()
    for change, word in ((dict(frames=None), "frames is null"), (dict(out=None), "out is null"), (dict(lens=None), "lens is null"),
                         (dict(work=None), "work is null"), (dict(n_frames=0), "n_frames 0"), (dict(n_frames=-1), "n_frames -1"),
                         (dict(height=0), "height 0"), (dict(height=65536), "height 65536"), (dict(width=0), "width 0"),
                         (dict(width=-4), "width -4"), (dict(width=65536), "width 65536"), (dict(quality=0), "quality 0"),
                         (dict(quality=101), "quality 101"), (dict(subsampling=2), "subsampling 2"), (dict(subsampling=-1), "subsampling -1"),
                         (dict(restart_mcus=-1), "restart_mcus -1"), (dict(restart_mcus=65536), "restart_mcus 65536"),
                         (dict(out_pitch=626), "out_pitch 626"), (dict(out_pitch=0), "out_pitch 0"), (dict(out_pitch=-8), "out_pitch -8"),
                         (dict(lens=66), "lens is not aligned"), (dict(work=8193), "work is not aligned"),
                         (dict(height=65535, width=65535, subsampling=J.J444), "height 65535 x width 65535"),
                         (dict(n_frames=2 ** 31 - 1, height=64, width=64, restart_mcus=1), "n_frames 2147483647")):
        desc = _lib.JpegDesc(**dict(ok, **change))
        assert L.refid_jpeg_encode(ctypes.byref(desc), None) == 1, change
        message = L.refid_last_error().decode()
        assert message.startswith("jpeg:") and word in message, (change, message)


def test_the_option_values_are_checked():
    from fractions import Fraction
    from refid_amd import deblur, interpolate
    from refid_amd._lib import RefidHipError
    from refid_amd.validation import check_video_options
    assert check_video_options() == (30, 90, "420", None)
    assert check_video_options(Fraction(30000, 1001), 1, "444", "bound") == (Fraction(30000, 1001), 1, "444", "bound")
    assert check_video_options(12.5, 100, "420", 627)[3] == 627
    for kw, word in ((dict(fps=0), "video_fps"), (dict(fps="x"), "video_fps"), (dict(quality=0), "video_quality 0"),
                     (dict(quality=90.0), "video_quality 90.0"), (dict(subsampling="422"), "video_subsampling '422'"),
                     (dict(subsampling=420), "video_subsampling 420"), (dict(jpeg_pitch=626), "jpeg_pitch 626"),
                     (dict(jpeg_pitch="all"), "jpeg_pitch 'all'")):
        with pytest.raises(RefidHipError, match="SequenceInterpolator.run: " + word):
            check_video_options(**dict(kw, where="SequenceInterpolator.run"))
    import torch
    from refid_amd import ops
    from refid_amd.validation import VideoWriter
    for kw, word in ((dict(fps=0), "VideoWriter: video_fps"), (dict(quality=101), "VideoWriter: video_quality 101"),
                     (dict(subsampling="411"), "VideoWriter: video_subsampling '411'"), (dict(jpeg_pitch=-1), "VideoWriter: jpeg_pitch -1")):
        with pytest.raises(RefidHipError, match=word):                 # checked before a stream or a file is made
            VideoWriter(**dict(dict(device=None, path="v.avi", fps=30), **kw))
    with pytest.raises(RefidHipError, match="jpeg_encode: a non-empty contiguous uint8 CUDA tensor .* on cpu"):
        ops.jpeg_encode(torch.zeros((1, 8, 8, 3), dtype=torch.uint8))   # no CPU fallback
    inputs = ["--frames", "f", "--events", "e", "--stamps", "s"]
    for main in (interpolate.main, deblur.main):                       # the flags are checked before anything is loaded
        for flags, word in ((["--video-quality", "0"], "--video-quality 0"), (["--video-quality", "high"], "--video-quality: 'high'"),
                            (["--video-fps", "0"], "--video-fps"), (["--video-fps", "1/0"], "--video-fps: '1/0'"),
                            (["--video-subsampling", "422"], "--video-subsampling '422'")):
            with pytest.raises(SystemExit, match=word):
                main([*inputs, "--video", "v.avi", *flags])
        with pytest.raises(SystemExit, match="--out, --video or both"):
            main(inputs)
        with pytest.raises(SystemExit, match="give --out"):
            main([*inputs, "--video", "v.avi", "--niqe", "p.npz"])
    with pytest.raises(SystemExit):
        deblur.main([*inputs, "--video", "v.avi", "--video-no-keys"])
