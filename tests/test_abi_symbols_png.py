"""CPU-only: the PNG entry point of include/refid_hip.h -- the library exports refid_png_unfilter, the ctypes mirror of
refid_png_unfilter_desc has the header's field order and types, the line limit agrees, and the ABI version stays 9
(additive)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {"int32_t": ctypes.c_int32, "uint8_t": ctypes.c_uint8}


def _fields(struct_name):
    """[(name, ctypes type)] of a struct of the header: pointers are c_void_p."""
    src = open(os.path.join(ROOT, "include", "refid_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct_name, struct_name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        mt = re.match(r"^(const\s+)?(uint8_t|int32_t)\s*(.*)$", stmt)
        assert mt, stmt
        for name in mt.group(3).split(","):
            name = name.strip()
            out.append((name.lstrip("*").strip(), ctypes.c_void_p if name.startswith("*") else C_TYPES[mt.group(2)]))
    return out


def test_png_desc_matches_the_header():
    from refid_amd import _lib
    assert _fields("refid_png_unfilter_desc") == list(_lib.PngUnfilterDesc._fields_)
    assert [f[0] for f in _lib.PngUnfilterDesc._fields_] == ["rows", "frames", "bands", "n_bands", "n_frames", "height", "width",
                                                             "channels"]
    assert ctypes.sizeof(_lib.PngUnfilterDesc) == 3 * 8 + 5 * 4 + 4                 # three pointers, five int32, tail padding
    src = open(os.path.join(ROOT, "include", "refid_hip.h")).read()
    assert int(re.search(r"#define REFID_PNG_MAX_ROW_BYTES (\d+)", src).group(1)) == _lib.PNG_MAX_ROW_BYTES
    assert _lib.PNG_MAX_ROW_BYTES % 12 == 0                                         # whole 12-byte groups (csrc/png.hip)
    decl = re.search(r"int refid_png_unfilter\((.*?)\);", src, re.S).group(1)
    assert [a.strip() for a in decl.split(",")] == ["const refid_png_unfilter_desc* d", "void* stream"]
    assert int(re.search(r"#define REFID_ABI_VERSION (\d+)", src).group(1)) == 9


def test_library_exports_the_png_entry_point():
    from refid_amd import _lib, ops
    from refid_amd.build import build
    L = ctypes.CDLL(build())
    assert hasattr(L, "refid_png_unfilter") and hasattr(L, "refid_niqe_moments")
    bound = _lib.lib()
    assert bound.refid_png_unfilter.argtypes[0]._type_ is _lib.PngUnfilterDesc
    assert bound.refid_png_unfilter.argtypes[1] is ctypes.c_void_p
    assert bound.refid_abi_version() == 9                                          # additive: the ABI version stays
    assert callable(ops.png_unfilter)


def test_the_entry_rejects_bad_descriptors_before_any_launch():
    """The argument checks run on the host and launch nothing, so they hold without a GPU."""
    from refid_amd import _lib
    L = _lib.lib()
    ok = dict(rows=16, frames=16, bands=None, n_bands=0, n_frames=1, height=2, width=3, channels=3)
    for change, word in ((dict(rows=None), "null"), (dict(channels=2), "channels 2"), (dict(width=0), "positive"),
                         (dict(width=_lib.PNG_MAX_ROW_BYTES // 3 + 1), "LDS line"), (dict(n_bands=2), "n_bands 2"),
                         (dict(bands=16, n_bands=0), "n_bands 0")):
        desc = _lib.PngUnfilterDesc(**dict(ok, **change))
        assert L.refid_png_unfilter(ctypes.byref(desc), None) == 1, change
        assert word in L.refid_last_error().decode(), (change, L.refid_last_error())
