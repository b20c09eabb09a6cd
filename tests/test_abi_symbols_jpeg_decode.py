"""CPU-only: the JPEG decode entry points of include/refid_hip.h -- the ctypes mirrors of refid_jpeg_info and
refid_jpeg_decode_desc have the header's field order and types, the constants agree with the header and with
tests/jpeg_decode_ref.py, the library exports the entry points, the ABI version stays 9 (additive), a bad descriptor is
turned down on the host with a message that names the field, before anything is launched, sequence.load_key_frames
dispatches by what the path holds, and both command lines end in a plain message when JPEG input meets a machine without
a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import jpeg_decode_cases as K
import jpeg_decode_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {"int32_t": ctypes.c_int32, "uint8_t": ctypes.c_uint8, "uint16_t": ctypes.c_uint16, "int16_t": ctypes.c_int16}


def _header():
    with open(os.path.join(ROOT, "include", "refid_hip.h")) as f:
        return f.read()


def _fields(struct_name):
    """[(name, ctypes type)] of a struct of the header, parsed as test_abi_symbols_jpeg.py does: pointers are c_void_p,
    ``name[n]`` an array."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct_name, struct_name), _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        mt = re.match(r"^(const\s+)?(uint8_t|uint16_t|int16_t|int32_t)\s*(.*)$", stmt)
        assert mt, stmt
        for name in mt.group(3).split(","):
            name = name.strip()
            array = re.match(r"^(\w+)\[(\d+)\]$", name)
            if array:
                out.append((array.group(1), C_TYPES[mt.group(2)] * int(array.group(2))))
            else:
                out.append((name.lstrip("*").strip(), ctypes.c_void_p if name.startswith("*") else C_TYPES[mt.group(2)]))
    return out


def test_the_structs_and_constants_match_the_header():
    from refid_amd import _lib, jpeg, ops
    assert _fields("refid_jpeg_info") == list(_lib.JpegInfo._fields_)
    assert _fields("refid_jpeg_decode_desc") == list(_lib.JpegDecodeDesc._fields_)
    assert [f[0] for f in _lib.JpegDecodeDesc._fields_] == ["coefs", "quant", "frames", "work", "n_frames", "height", "width", "sampling"]
    assert ctypes.sizeof(_lib.JpegInfo) == 9 * 4 and ctypes.sizeof(_lib.JpegDecodeDesc) == 4 * 8 + 4 * 4
    src = _header()
    const = lambda name: int(re.search(r"#define %s (\d+)" % name, src).group(1))       # noqa: E731
    assert const("REFID_JPEG_DEC_GREY") == _lib.JPEG_DEC_GREY == R.GREY == jpeg.GREY == 0
    assert const("REFID_JPEG_DEC_444") == _lib.JPEG_DEC_444 == R.S444 == jpeg.S444 == 1
    assert const("REFID_JPEG_DEC_422") == _lib.JPEG_DEC_422 == R.S422 == jpeg.S422 == 2
    assert const("REFID_JPEG_DEC_420") == _lib.JPEG_DEC_420 == R.S420 == jpeg.S420 == 3
    assert jpeg.SAMPLINGS == K.CODES == ops.JPEG_DECODE_SAMPLINGS and jpeg.SAMPLING_NAMES == R.SAMPLING_NAMES
    assert const("REFID_JPEG_444") == 0 and const("REFID_JPEG_420") == 1           # the encoder's constants are untouched
    for decl in (r"int refid_jpeg_probe\(const uint8_t\* file, size_t len, refid_jpeg_info\* info\);",
                 r"int refid_jpeg_entropy_decode\(const uint8_t\* file, size_t len, const refid_jpeg_info\* expect, int16_t\* coefs, "
                 r"uint16_t\* quant\);",
                 r"int refid_jpeg_decode\(const refid_jpeg_decode_desc\* d, void\* stream\);",
                 r"size_t refid_jpeg_decode_work_bytes\(int32_t n_frames, int32_t height, int32_t width, int32_t sampling\);"):
        assert re.search(decl, src), decl
    assert const("REFID_ABI_VERSION") == 9 == _lib.ABI_VERSION


def test_the_library_exports_the_entry_points_and_the_size_functions_agree():
    from refid_amd import _lib, ops, sequence, validation
    from refid_amd.build import build
    L = ctypes.CDLL(build())
    for name in ("refid_jpeg_probe", "refid_jpeg_entropy_decode", "refid_jpeg_decode", "refid_jpeg_decode_work_bytes", "refid_jpeg_decode_blocks"):
        assert hasattr(L, name), name
    bound = _lib.lib()
    assert bound.refid_abi_version() == 9                                          # additive: the ABI version stays
    assert bound.refid_jpeg_decode.argtypes[0]._type_ is _lib.JpegDecodeDesc and bound.refid_jpeg_decode_work_bytes.restype is ctypes.c_size_t
    assert validation.JPEG_SUBSAMPLINGS == ("420", "444") and ops.JPEG_SUBSAMPLINGS == {"444": 0, "420": 1}
    assert callable(ops.jpeg_decode) and callable(sequence.load_jpeg_frames) and callable(sequence.load_key_frames)
    for h, w in ((1, 1), (8, 8), (17, 35), (33, 65), (720, 1280), (1080, 1920), (65535, 65535), (1, 65535)):
        for name, code in K.CODES.items():
            blocks, total = R.blocks_of(h, w, code)
            assert ops.jpeg_decode_blocks(h, w, name) == (blocks, total), (h, w, name)
            for n in (1, 3):
                want = n * total * 64 if (n * total + 255) // 256 <= 2 ** 31 - 1 else 0      # the planes: one byte per sample
                assert bound.refid_jpeg_decode_work_bytes(n, h, w, code) == want, (n, h, w, name)
    for args in ((0, 8, 8, 1), (-1, 8, 8, 1), (65536, 8, 8, 1), (1, 0, 8, 1), (1, 8, 0, 1), (1, 65536, 8, 1), (1, 8, 65536, 1), (1, 8, 8, 4),
                 (1, 8, 8, -1), (65535, 65535, 65535, 1)):
        assert bound.refid_jpeg_decode_work_bytes(*args) == 0, args
    assert bound.refid_jpeg_decode_blocks(0, 8, 1, None) == 0 and bound.refid_jpeg_decode_blocks(8, 8, 7, None) == 0


def test_the_entry_rejects_bad_descriptors_before_any_launch():
    """The argument checks run on the host and launch nothing, so they hold without a GPU (a launch without one would
    return 2, 'launch failed')."""
    from refid_amd import _lib
    L = _lib.lib()
    ok = dict(coefs=4096, quant=256, frames=17, work=8192, n_frames=2, height=17, width=35, sampling=R.S420)
    assert L.refid_jpeg_decode(None, None) == 1 and "descriptor" in L.refid_last_error().decode()
    for change, word in ((dict(coefs=None), "coefs is null"), (dict(quant=None), "quant is null"), (dict(frames=None), "frames is null"),
                         (dict(work=None), "work is null"), (dict(n_frames=0), "n_frames 0"), (dict(n_frames=-3), "n_frames -3"),
                         (dict(height=0), "height 0"), (dict(height=65536), "height 65536"), (dict(height=-1), "height -1"),
                         (dict(width=0), "width 0"), (dict(width=65536), "width 65536"), (dict(sampling=4), "sampling 4"),
                         (dict(sampling=-1), "sampling -1"), (dict(coefs=4098), "coefs is not aligned"), (dict(coefs=4104), "coefs is not aligned"),
                         (dict(quant=257), "quant is not aligned"), (dict(work=8200), "work is not aligned"),
                         (dict(n_frames=65536), "n_frames 65536"), (dict(n_frames=65535, height=65535, width=65535, sampling=R.S444), "exceed the grid")):
        desc = _lib.JpegDecodeDesc(**dict(ok, **change))
        assert L.refid_jpeg_decode(ctypes.byref(desc), None) == 1, change
        message = L.refid_last_error().decode()
        assert message.startswith("jpeg_decode:") and word in message, (change, message)


def test_ops_jpeg_decode_checks_its_arguments_on_the_host():
    import torch
    from refid_amd import ops
    from refid_amd._lib import RefidHipError
    coefs, quant = torch.zeros((1, 3, 64), dtype=torch.int16), torch.zeros((1, 3, 64), dtype=torch.int16)
    with pytest.raises(RefidHipError, match="coefs must be a contiguous int16 CUDA tensor of 1\\*3\\*64 elements .* on cpu"):
        ops.jpeg_decode(coefs, quant, 1, 8, 8, "444")                  # no CPU fallback
    with pytest.raises(RefidHipError, match="sampling '411'"):
        ops.jpeg_decode(coefs, quant, 1, 8, 8, "411")
    with pytest.raises(RefidHipError, match="n=0"):
        ops.jpeg_decode(coefs, quant, 0, 8, 8, "444")
    with pytest.raises(RefidHipError, match="height 0 and width 8"):
        ops.jpeg_decode(coefs, quant, 1, 0, 8, "444")


def _write(path, data):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)


def test_load_key_frames_dispatches_by_what_the_path_holds(tmp_path, monkeypatch):
    """The loaders behind it are replaced by recorders: the dispatch is host logic."""
    from refid_amd import png, sequence, video
    from refid_amd._lib import RefidHipError
    calls = []
    monkeypatch.setattr(sequence, "load_png_frames", lambda paths, **kw: calls.append(("png", list(paths), kw)) or "P")
    monkeypatch.setattr(sequence, "load_jpeg_frames", lambda sources, **kw: calls.append(("jpeg", list(sources), kw)) or "J")
    jpg = K.golden()["s420_17x35_q90"][0]
    for name in ("b.jpg", "a.jpeg", "c.jpg"):
        _write(str(tmp_path / "jpegs" / name), jpg)
    (tmp_path / "jpegs" / "notes.txt").write_text("not a frame")
    for name in ("1.png", "0.png"):
        png.write_png(str(tmp_path / "pngs" / name), np.zeros((4, 4, 3), dtype=np.uint8))
    kw = dict(device=None, workers=8, frames_per_launch=8)
    assert sequence.load_key_frames(str(tmp_path / "jpegs")) == "J"
    assert calls.pop() == ("jpeg", [str(tmp_path / "jpegs" / n) for n in ("a.jpeg", "b.jpg", "c.jpg")], kw)     # sorted by name
    assert sequence.load_key_frames(tmp_path / "pngs", workers=2) == "P"
    assert calls.pop() == ("png", [str(tmp_path / "pngs" / n) for n in ("0.png", "1.png")], dict(kw, workers=2))
    # a video in three parts: the parts follow in order
    frames = [jpg + bytes([k]) for k in range(5)]
    with video.MjpegAviWriter(str(tmp_path / "clip.avi"), 35, 17, 30, max_bytes=video._FIRST_CHUNK + 2 * (len(jpg) + 40)) as wr:
        for f in frames:
            wr.add(f)
    assert len(wr.paths) == 3 and wr.paths[1] == video.part_path(str(tmp_path / "clip.avi"), 2)
    assert sequence.load_key_frames(str(tmp_path / "clip.avi"), frames_per_launch=3) == "J"
    assert calls.pop() == ("jpeg", frames, dict(kw, frames_per_launch=3))
    os.rename(str(tmp_path / "clip.avi"), str(tmp_path / "CLIP2.AVI"))
    assert sequence.load_key_frames(str(tmp_path / "CLIP2.AVI")) == "J" and calls.pop()[1] == frames[:2]     # its parts have another stem
    # errors
    _write(str(tmp_path / "both" / "0.jpg"), jpg)
    png.write_png(str(tmp_path / "both" / "1.png"), np.zeros((4, 4, 3), dtype=np.uint8))
    with pytest.raises(RefidHipError, match="holds both PNG \\(1\\) and JPEG \\(1\\) files"):
        sequence.load_key_frames(str(tmp_path / "both"))
    os.makedirs(tmp_path / "empty")
    with pytest.raises(RefidHipError, match="no \\*.png, \\*.jpg or \\*.jpeg under"):
        sequence.load_key_frames(str(tmp_path / "empty"))
    with pytest.raises(RefidHipError, match="neither a directory"):
        sequence.load_key_frames(str(tmp_path / "frames.npy"))
    _write(str(tmp_path / "bad.avi"), b"RIFF\0\0\0\0nope")
    with pytest.raises(RefidHipError, match="bad.avi: not a RIFF AVI file"):
        sequence.load_key_frames(str(tmp_path / "bad.avi"))
    with pytest.raises(RefidHipError, match="load_key_frames: .*missing.avi"):
        sequence.load_key_frames(str(tmp_path / "missing.avi"))
    assert not calls


def test_load_jpeg_frames_checks_its_arguments_without_a_gpu(tmp_path):
    from refid_amd import sequence
    from refid_amd._lib import RefidHipError
    os.makedirs(tmp_path / "empty")
    with pytest.raises(RefidHipError, match="load_jpeg_frames: no files"):
        sequence.load_jpeg_frames(str(tmp_path / "empty"))
    jpg = K.golden()["s420_17x35_q90"][0]
    for kw in (dict(workers=0), dict(workers=sequence.PNG_WORKERS_MAX + 1), dict(frames_per_launch=0)):
        with pytest.raises(RefidHipError, match="workers .* must be 1..16 and frames_per_launch"):
            sequence.load_jpeg_frames([jpg], **kw)
    with pytest.raises(RefidHipError, match="a GPU device is required"):
        sequence.load_jpeg_frames([jpg], device="cpu")


def test_jpeg_input_without_a_gpu_ends_in_a_plain_message(tmp_path, monkeypatch):
    """--frames DIR_OF_JPEGS and --frames clip.avi of both command lines on a machine without a GPU; PNG and .npy input keep
    their host route and messages."""
    import torch
    from refid_amd import deblur, interpolate
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    jpg = K.golden()["s420_17x35_q90"][0]
    _write(str(tmp_path / "jpegs" / "0.jpg"), jpg)
    _write(str(tmp_path / "clip.avi"), b"RIFF")
    os.makedirs(tmp_path / "empty")
    common = ["--events", "e.npz", "--stamps", "s.txt", "--out", str(tmp_path / "out")]
    for main, extra in ((interpolate.main, ["--n", "1"]), (deblur.main, ["--num-bins", "6"])):
        for frames in (str(tmp_path / "jpegs"), str(tmp_path / "clip.avi")):
            with pytest.raises(SystemExit, match="--frames: JPEG key frames need the GPU"):
                main([*common, *extra, "--frames", frames])
        with pytest.raises(SystemExit, match="--frames: no \\*.png under"):
            main([*common, *extra, "--frames", str(tmp_path / "empty")])
    assert "JPEG" in interpolate.__doc__ and ".avi" in interpolate.__doc__ and "JPEG" in deblur.__doc__
