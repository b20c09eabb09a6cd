"""CPU-only: the PNG filter entry point of include/refid_hip.h -- the library exports refid_png_filter, the ctypes mirror of
refid_png_filter_desc has the header's field order and types, the constants agree, the ABI version stays 9 (additive), and
a bad descriptor is turned down on the host with a message that names the field, before anything is launched."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {"int32_t": ctypes.c_int32, "uint8_t": ctypes.c_uint8, "uint32_t": ctypes.c_uint32}


def _header():
    with open(os.path.join(ROOT, "include", "refid_hip.h")) as f:
        return f.read()


def _fields(struct_name):
    """[(name, ctypes type)] of a struct of the header, parsed as test_abi_symbols_png.py does: pointers are c_void_p."""
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


def test_png_filter_desc_matches_the_header():
    from refid_amd import _lib
    assert _fields("refid_png_filter_desc") == list(_lib.PngFilterDesc._fields_)
    assert [f[0] for f in _lib.PngFilterDesc._fields_] == ["frames", "rows", "costs", "n_frames", "height", "width", "mode"]
    assert ctypes.sizeof(_lib.PngFilterDesc) == 3 * 8 + 4 * 4                       # three pointers, four int32
    src = _header()
    assert int(re.search(r"#define REFID_PNG_FILTER_ADAPTIVE (\d+)", src).group(1)) == _lib.PNG_FILTER_ADAPTIVE == 5
    limit = int(re.search(r"#define REFID_PNG_FILTER_MAX_WIDTH (\d+)", src).group(1))
    assert limit == _lib.PNG_FILTER_MAX_WIDTH
    assert 128 * 3 * limit < 2 ** 32 <= 128 * 3 * (limit + 1)                       # the widest row whose cost sum fits uint32
    decl = re.search(r"int refid_png_filter\((.*?)\);", src, re.S).group(1)
    assert [a.strip() for a in decl.split(",")] == ["const refid_png_filter_desc* d", "void* stream"]
    assert int(re.search(r"#define REFID_ABI_VERSION (\d+)", src).group(1)) == 9 == _lib.ABI_VERSION


def test_library_exports_the_png_filter_entry_point():
    from refid_amd import _lib, ops, png, validation
    from refid_amd.build import build
    L = ctypes.CDLL(build())
    assert hasattr(L, "refid_png_filter") and hasattr(L, "refid_png_unfilter")
    bound = _lib.lib()
    assert bound.refid_png_filter.argtypes[0]._type_ is _lib.PngFilterDesc
    assert bound.refid_png_filter.argtypes[1] is ctypes.c_void_p
    assert bound.refid_abi_version() == 9                                          # additive: the ABI version stays
    assert callable(ops.png_filter) and callable(png.encode_png_rows) and callable(png.write_png_rows)
    assert validation.PNG_FILTERS == ("none", "adaptive")


def test_the_entry_rejects_bad_descriptors_before_any_launch():
    """The argument checks run on the host and launch nothing, so they hold without a GPU (a launch without one would
    return 2, 'launch failed')."""
    from refid_amd import _lib
    L = _lib.lib()
    ok = dict(frames=16, rows=64, costs=None, n_frames=1, height=2, width=3, mode=5)
    assert L.refid_png_filter(None, None) == 1 and "descriptor" in L.refid_last_error().decode()
    for change, word in ((dict(frames=None), "frames"), (dict(rows=None), "rows"), (dict(width=0), "width 0"),
                         (dict(height=0), "height 0"), (dict(n_frames=-1), "n_frames -1"), (dict(mode=6), "mode 6"),
                         (dict(mode=-1), "mode -1"), (dict(width=_lib.PNG_FILTER_MAX_WIDTH + 1), f"width {_lib.PNG_FILTER_MAX_WIDTH + 1}"),
                         (dict(costs=18), "costs")):
        desc = _lib.PngFilterDesc(**dict(ok, **change))
        assert L.refid_png_filter(ctypes.byref(desc), None) == 1, change
        message = L.refid_last_error().decode()
        assert message.startswith("png_filter:") and word in message, (change, message)


def test_the_option_value_is_checked():
    import pytest
    from refid_amd._lib import RefidHipError
    from refid_amd.validation import check_png_filter
    assert check_png_filter(None) == "none" and check_png_filter("none") == "none" and check_png_filter("adaptive") == "adaptive"
    with pytest.raises(RefidHipError, match="val.png_filter: 'paeth'"):
        check_png_filter("paeth", "val.png_filter")
