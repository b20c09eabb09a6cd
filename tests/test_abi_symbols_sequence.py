"""CPU-only: the sequence entry points of include/refid_hip.h -- the ctypes mirrors of refid_seq_pair / refid_seq_desc
have the header's field order and sizes, and the library exports the new symbol next to the existing ones."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float}


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
        mt = re.match(r"^(const\s+)?(unsigned char|long long|float|int|refid_seq_pair)\s*(.*)$", stmt)
        assert mt, stmt
        for name in mt.group(3).split(","):
            name = name.strip()
            pointer = name.startswith("*")
            out.append((name.lstrip("*").strip(), ctypes.c_void_p if pointer else C_TYPES[mt.group(2)]))
    return out


def test_seq_structs_match_the_header():
    from refid_amd._lib import SeqDesc, SeqPair
    assert _fields("refid_seq_pair") == list(SeqPair._fields_)
    assert _fields("refid_seq_desc") == list(SeqDesc._fields_)
    assert [f[0] for f in SeqPair._fields_] == ["left", "right", "row0", "row1", "first_stamp", "last_stamp"]
    assert ctypes.sizeof(SeqPair) == 32                                         # 2 int, 2 long long, 2 float: no padding


def test_library_exports_the_sequence_entry_point():
    from refid_amd import _lib
    from refid_amd.build import build
    L = ctypes.CDLL(build())
    assert hasattr(L, "refid_seq_assemble") and hasattr(L, "refid_assemble_batch")
    bound = _lib.lib()
    assert bound.refid_seq_assemble.argtypes[0]._type_ is _lib.SeqDesc
    assert bound.refid_abi_version() == 9                                       # additive: the ABI version stays
