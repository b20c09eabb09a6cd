"""CPU-only: the PNG deflate entry points of include/refid_hip.h -- the library exports refid_png_deflate and its two size
functions, the ctypes mirror of refid_png_deflate_desc has the header's field order and types, the constants agree with the
header and with tests/deflate_ref.py, the ABI version stays 9 (additive), and a bad descriptor is turned down on the host
with a message that names the field, before anything is launched."""
import ctypes
import os
import re

import deflate_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {"int32_t": ctypes.c_int32, "uint8_t": ctypes.c_uint8, "uint32_t": ctypes.c_uint32}


def _header():
    with open(os.path.join(ROOT, "include", "refid_hip.h")) as f:
        return f.read()


def _fields(struct_name):
    """[(name, ctypes type)] of a struct of the header, parsed as test_abi_symbols_png_filter.py does: pointers are c_void_p."""
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


def test_png_deflate_desc_matches_the_header():
    from refid_amd import _lib
    assert _fields("refid_png_deflate_desc") == list(_lib.PngDeflateDesc._fields_)
    assert [f[0] for f in _lib.PngDeflateDesc._fields_] == ["src", "out", "lens", "work", "n_streams", "stream_bytes", "block_bytes",
                                                           "out_pitch"]
    assert ctypes.sizeof(_lib.PngDeflateDesc) == 4 * 8 + 4 * 4                      # four pointers, four int32
    src = _header()
    const = lambda name: int(re.search(r"#define %s (\d+)" % name, src).group(1))       # noqa: E731
    assert const("REFID_PNG_DEFLATE_BLOCK") == _lib.PNG_DEFLATE_BLOCK == D.DEFAULT_BLOCK_BYTES
    assert const("REFID_PNG_DEFLATE_MAX_BLOCK") == _lib.PNG_DEFLATE_MAX_BLOCK == D.MAX_BLOCK == 65535
    assert const("REFID_PNG_DEFLATE_RECORD") == _lib.PNG_DEFLATE_RECORD == D.RECORD_BYTES
    assert D.RECORD_BYTES % 4 == 0 and D.RECORD_BYTES >= 4 * (8 + 257)              # a header of 8 words and the 257 codes
    decl = re.search(r"int refid_png_deflate\((.*?)\);", src, re.S).group(1)
    assert [a.strip() for a in decl.split(",")] == ["const refid_png_deflate_desc* d", "void* stream"]
    assert re.search(r"size_t refid_png_deflate_bound\(int32_t stream_bytes, int32_t block_bytes\);", src)
    assert re.search(r"size_t refid_png_deflate_work_bytes\(int32_t n_streams, int32_t stream_bytes, int32_t block_bytes\);", src)
    assert const("REFID_ABI_VERSION") == 9 == _lib.ABI_VERSION


def test_library_exports_the_png_deflate_entry_points():
    from refid_amd import _lib, ops, png, validation
    from refid_amd.build import build
    L = ctypes.CDLL(build())
    for name in ("refid_png_deflate", "refid_png_deflate_bound", "refid_png_deflate_work_bytes", "refid_png_filter"):
        assert hasattr(L, name), name
    bound = _lib.lib()
    assert bound.refid_png_deflate.argtypes[0]._type_ is _lib.PngDeflateDesc
    assert bound.refid_png_deflate.argtypes[1] is ctypes.c_void_p
    assert bound.refid_png_deflate_bound.restype is ctypes.c_size_t and bound.refid_png_deflate_work_bytes.restype is ctypes.c_size_t
    assert bound.refid_abi_version() == 9                                          # additive: the ABI version stays
    assert callable(ops.png_deflate) and callable(png.wrap_zlib_stream) and callable(png.write_png_stream)
    assert validation.PNG_DEFLATES == ("host", "device") and validation.PNG_FILTERS == ("none", "adaptive")


def test_bound_and_work_bytes_are_the_restatements_formulas():
    from refid_amd import _lib
    L = _lib.lib()
    for size in (1, 2, 4, 63, 64, 65, 257, 4101, 65535, 65536, 2764800, 5992704, 2 ** 31 - 1 - 11 - 5 * 32768):
        for block in (1, 2, 64, 257, 4096, 32768, 65535):
            want = D.bound(size, block)
            if want > 2 ** 31 - 1:
                assert L.refid_png_deflate_bound(size, block) == 0, (size, block)
                continue
            assert L.refid_png_deflate_bound(size, block) == want == 2 + size + 5 * (-(-size // block)) + 9, (size, block)
            for n in (1, 3, 9):
                want_work = D.work_bytes(n, size, block) if n * D.n_blocks(size, block) <= 2 ** 31 - 1 else 0
                assert L.refid_png_deflate_work_bytes(n, size, block) == want_work, (n, size, block)
    for size, block in ((0, 64), (-1, 64), (100, 0), (100, -3), (100, 65536), (2 ** 31 - 1, 65535)):
        assert L.refid_png_deflate_bound(size, block) == 0, (size, block)
        assert L.refid_png_deflate_work_bytes(1, size, block) == 0, (size, block)
    assert L.refid_png_deflate_work_bytes(0, 100, 64) == 0 and L.refid_png_deflate_work_bytes(-2, 100, 64) == 0
    assert L.refid_png_deflate_work_bytes(2 ** 31 - 1, 100, 1) == 0                  # more workgroups than a grid takes


def test_the_entry_rejects_bad_descriptors_before_any_launch():
    """The argument checks run on the host and launch nothing, so they hold without a GPU (a launch without one would
    return 2, 'launch failed')."""
    from refid_amd import _lib
    L = _lib.lib()
    ok = dict(src=16, out=4096, lens=64, work=8192, n_streams=2, stream_bytes=100, block_bytes=64, out_pitch=D.bound(100, 64))
    assert L.refid_png_deflate(None, None) == 1 and "descriptor" in L.refid_last_error().decode()
    for change, word in ((dict(src=None), "src is null"), (dict(out=None), "out is null"), (dict(lens=None), "lens is null"),
                         (dict(work=None), "work is null"), (dict(n_streams=0), "n_streams 0"), (dict(n_streams=-1), "n_streams -1"),
                         (dict(stream_bytes=0), "stream_bytes 0"), (dict(block_bytes=0), "block_bytes 0"),
                         (dict(block_bytes=-5), "block_bytes -5"), (dict(block_bytes=65536), "block_bytes 65536"),
                         (dict(out_pitch=D.bound(100, 64) - 1), f"out_pitch {D.bound(100, 64) - 1}"), (dict(out_pitch=0), "out_pitch 0"),
                         (dict(out_pitch=-8), "out_pitch -8"), (dict(lens=66), "lens is not aligned"), (dict(work=8193), "work is not aligned"),
                         (dict(stream_bytes=2 ** 31 - 1, out_pitch=2 ** 31 - 1), "stream_bytes 2147483647"),
                         (dict(n_streams=2 ** 31 - 1, block_bytes=1, out_pitch=2 ** 31 - 1), "n_streams 2147483647")):
        desc = _lib.PngDeflateDesc(**dict(ok, **change))
        assert L.refid_png_deflate(ctypes.byref(desc), None) == 1, change
        message = L.refid_last_error().decode()
        assert message.startswith("png_deflate:") and word in message, (change, message)


def test_the_option_value_is_checked():
    import pytest
    from refid_amd._lib import RefidHipError
    from refid_amd.validation import check_png_deflate
    assert check_png_deflate(None) == "host" and check_png_deflate("host") == "host" and check_png_deflate("device") == "device"
    with pytest.raises(RefidHipError, match="val.png_deflate: 'gpu'"):
        check_png_deflate("gpu", "val.png_deflate")
