"""CPU-only: the NIQE entry points of include/refid_hip.h -- the library exports both symbols, the header declares them
with the argument list the ctypes binding uses, the flag constants agree, and the ABI version stays 9 (additive)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_niqe_entry_points():
    from refid_amd import _lib
    from refid_amd.build import build
    L = ctypes.CDLL(build())
    assert hasattr(L, "refid_niqe_moments") and hasattr(L, "refid_niqe_moments_parts") and hasattr(L, "refid_val_tail")
    bound = _lib.lib()
    assert bound.refid_abi_version() == 9
    assert bound.refid_niqe_moments_parts.restype is ctypes.c_longlong
    assert bound.refid_niqe_moments_parts(3, 1224, 1632) >= 0


def test_binding_matches_the_header():
    from refid_amd import _lib
    src = open(os.path.join(ROOT, "include", "refid_hip.h")).read()
    decl = re.search(r"int refid_niqe_moments\((.*?)\);", src, re.S).group(1)
    args = [a.strip() for a in decl.replace("\n", " ").split(",")]
    kinds = [ctypes.c_void_p if "*" in a else ctypes.c_int for a in args]
    assert [a.split()[-1].lstrip("*") for a in args] == ["frames_u8", "n_frames", "h", "w", "flags", "crop_border", "window49",
                                                         "sums", "parts", "y_out", "mscn1_out", "mscn2_out", "stream"]
    assert list(_lib.lib().refid_niqe_moments.argtypes) == kinds
    assert int(re.search(r"#define REFID_NIQE_BGR (\d+)", src).group(1)) == _lib.NIQE_BGR
    assert int(re.search(r"#define REFID_ABI_VERSION (\d+)", src).group(1)) == 9
