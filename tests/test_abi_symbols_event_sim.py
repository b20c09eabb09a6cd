"""CPU-only: the event simulator's entry points of include/refid_hip.h -- the ctypes mirror of refid_event_sim_desc has the
header's field order and types, the constants agree with the header and with tests/event_sim_ref.py, the library exports
the entry points, the ABI version stays 9 (additive), a bad descriptor is turned down on the host with a message that
names the field, before anything is launched, ``ops.event_sim`` checks its arguments on the host, and the command line
names a bad flag and ends in a plain message on a machine without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import event_sim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint8_t": ctypes.c_uint8, "float": ctypes.c_float, "double": ctypes.c_double}


def _header():
    with open(os.path.join(ROOT, "include", "refid_hip.h")) as f:
        return f.read()


def _fields(struct_name):
    """[(name, ctypes type)] of a struct of the header, parsed as test_abi_symbols_jpeg_decode.py does: pointers are c_void_p."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct_name, struct_name), _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        mt = re.match(r"^(const\s+)?(uint8_t|int32_t|int64_t|float|double)\s*(.*)$", stmt)
        assert mt, stmt
        for name in mt.group(3).split(","):
            name = name.strip()
            out.append((name.lstrip("*").strip(), ctypes.c_void_p if name.startswith("*") else C_TYPES[mt.group(2)]))
    return out


def test_the_struct_and_constants_match_the_header():
    from refid_amd import _lib
    assert _fields("refid_event_sim_desc") == list(_lib.EventSimDesc._fields_)
    assert [f[0] for f in _lib.EventSimDesc._fields_] == [
        "frames", "stamps_host", "stamps_dev", "lut", "c_pos_map", "c_neg_map", "state", "counts", "totals", "ends", "rows", "keys", "perm",
        "sorted", "n_rows", "n_frames", "height", "width", "bgr", "c_pos", "c_neg", "c_min", "lut_min", "lut_max", "stage"]
    assert ctypes.sizeof(_lib.EventSimDesc) == 14 * 8 + 8 + 10 * 4
    src = _header()
    const = lambda name: int(re.search(r"#define %s (\d+)" % name, src).group(1))       # noqa: E731
    assert (const("REFID_EVENT_SIM_RESET"), const("REFID_EVENT_SIM_COUNT"), const("REFID_EVENT_SIM_EMIT"), const("REFID_EVENT_SIM_GATHER")) == \
        (_lib.EVENT_SIM_RESET, _lib.EVENT_SIM_COUNT, _lib.EVENT_SIM_EMIT, _lib.EVENT_SIM_GATHER) == (1, 2, 4, 8)
    assert const("REFID_EVENT_SIM_CAP") == _lib.EVENT_SIM_CAP == R.CAP == 255
    assert const("REFID_EVENT_SIM_MAX_FRAMES") == _lib.EVENT_SIM_MAX_FRAMES == 512            # 9 bits of k in a signed 64-bit key
    assert const("REFID_EVENT_SIM_MAX_PIXELS") == _lib.EVENT_SIM_MAX_PIXELS == 1 << 25        # 25 bits of pix; 21 of tick, 8 of j
    assert (const("REFID_EVENT_SIM_FLAG_OVERFLOW"), const("REFID_EVENT_SIM_FLAG_SLOTS")) == (_lib.EVENT_SIM_FLAG_OVERFLOW, _lib.EVENT_SIM_FLAG_SLOTS) == (1, 2)
    for decl in (r"int refid_event_sim\(const refid_event_sim_desc\* d, void\* stream\);",
                 r"int32_t refid_event_sim_min_threshold\(int32_t lut_min, int32_t lut_max\);"):
        assert re.search(decl, src), decl
    assert const("REFID_ABI_VERSION") == 9 == _lib.ABI_VERSION


def test_the_library_exports_the_entry_points():
    from refid_amd import _lib, event_sim, ops, simulate
    from refid_amd.build import build
    L = ctypes.CDLL(build())
    for name in ("refid_event_sim", "refid_event_sim_min_threshold"):
        assert hasattr(L, name), name
    bound = _lib.lib()
    assert bound.refid_abi_version() == 9                                          # additive: the ABI version stays
    assert bound.refid_event_sim.argtypes[0]._type_ is _lib.EventSimDesc
    assert callable(ops.event_sim) and callable(ops.event_sim_reset) and callable(event_sim.EventSimulator) and callable(simulate.main)
    lut = R.default_lut()
    assert bound.refid_event_sim_min_threshold(int(lut.min()), int(lut.max())) == 1776 == R.min_threshold(lut)
    for lo, hi in ((0, 0), (0, 254), (0, 255), (-5, 5000), (-2 ** 31, 2 ** 31 - 1)):
        assert bound.refid_event_sim_min_threshold(lo, hi) == (hi - lo) // 255 + 1, (lo, hi)
    assert bound.refid_event_sim_min_threshold(5, 4) == 0


def test_the_entry_rejects_bad_descriptors_before_any_launch():
    """The argument checks run on the host and launch nothing, so they hold without a GPU (a launch without one would
    return 2, 'launch failed').  The pointers are never followed, except stamps_host, which is real."""
    from refid_amd import _lib
    L = _lib.lib()
    lut = R.default_lut()
    stamps = np.array([0.0, 1.0, 2.5], dtype=np.float64)
    equal, back, nan = np.array([0.0, 1.0, 1.0]), np.array([0.0, 2.0, 1.0]), np.array([0.0, np.nan, 1.0])
    big = np.arange(513, dtype=np.float64)
    ok = dict(frames=4099, stamps_host=stamps.ctypes.data, stamps_dev=4096, lut=8192, state=12288, counts=16384, totals=20480, ends=24576,
              rows=28672, keys=32768, perm=36864, sorted=40960, n_rows=5, n_frames=3, height=17, width=35, bgr=0, c_pos=13107, c_neg=13107,
              lut_min=int(lut.min()), lut_max=int(lut.max()))
    assert L.refid_event_sim(None, None) == 1 and "descriptor" in L.refid_last_error().decode()
    count, emit, gather, reset = _lib.EVENT_SIM_COUNT, _lib.EVENT_SIM_EMIT, _lib.EVENT_SIM_GATHER, _lib.EVENT_SIM_RESET
    cases = [
        (count, dict(stage=0), "stage 0"), (count, dict(stage=3), "stage 3"),
        (count, dict(frames=None), "frames is null"), (count, dict(lut=None), "lut is null"), (count, dict(state=None), "state is null"),
        (reset, dict(state=None), "state is null"), (reset, dict(height=0), "height 0"),
        (count, dict(stamps_host=None), "stamps_host is null"), (count, dict(stamps_dev=None), "stamps_dev is null"),
        (count, dict(totals=None), "totals is null"), (count, dict(counts=None), "counts is null"),
        (count, dict(lut=8194), "lut is not aligned"), (count, dict(state=12289), "state is not aligned"),
        (count, dict(stamps_dev=4100), "stamps_dev is not aligned"), (count, dict(totals=20484), "totals is not aligned"),
        (count, dict(counts=16386), "counts is not aligned"), (count, dict(c_pos_map=4097), "c_pos_map is not aligned"),
        (count, dict(n_frames=1), "n_frames 1 must be at least 2"), (count, dict(n_frames=0), "n_frames 0"), (emit, dict(n_frames=-4), "n_frames -4"),
        (count, dict(n_frames=513, stamps_host=big.ctypes.data), "n_frames 513 exceeds 512"),
        (count, dict(height=0), "height 0"), (count, dict(width=-1), "width -1"),
        (count, dict(height=8192, width=4097), "33562624 pixels exceed 33554432, what the sort key holds"),
        (count, dict(c_pos=0), "c_pos 0 must be at least 1"), (count, dict(c_neg=-7), "c_neg -7 must be at least 1"),
        (count, dict(c_pos_map=4096, c_pos=0, c_min=0), "c_min 0"), (count, dict(c_neg_map=4096, c_min=-1), "c_min -1"),
        (count, dict(c_pos=1775), "thresholds must be at least 1776"), (emit, dict(c_neg=1775), "smallest threshold 1775 allows 256 events"),
        (count, dict(c_pos_map=4096, c_neg_map=4096, c_min=1775), "thresholds must be at least 1776"),
        (count, dict(c_pos_map=4096, c_min=5000, c_neg=1000), "smallest threshold 1000"),
        (count, dict(lut_min=5, lut_max=4), "lut_max 4 is below lut_min 5"),
        (count, dict(stamps_host=equal.ctypes.data), "stamps are not strictly increasing: stamps[2]"),
        (count, dict(stamps_host=back.ctypes.data), "stamps are not strictly increasing: stamps[2]"),
        (emit, dict(stamps_host=nan.ctypes.data), "stamps[1] is not finite"),
        (emit, dict(n_rows=2 ** 31), "n_rows 2147483648 is not 1 .. 2^31 - 1 (use a smaller chunk)"), (emit, dict(n_rows=0), "n_rows 0"),
        (emit, dict(n_rows=-1), "n_rows -1"),
        (emit, dict(ends=None), "ends is null"), (emit, dict(rows=None), "rows is null"), (emit, dict(keys=None), "keys is null"),
        (emit, dict(rows=28680), "rows is not aligned to 16"), (emit, dict(ends=24580), "ends is not aligned to 8"),
        (emit, dict(keys=32772), "keys is not aligned to 8"),
        (gather, dict(n_rows=2 ** 31), "use a smaller chunk"), (gather, dict(n_rows=0), "n_rows 0"), (gather, dict(rows=None), "rows is null"),
        (gather, dict(perm=None), "perm is null"), (gather, dict(sorted=None), "sorted is null"), (gather, dict(sorted=40968), "sorted is not aligned to 16"),
        (gather, dict(rows=28676), "rows is not aligned to 16"), (gather, dict(perm=36868), "perm is not aligned to 8"),
    ]
    for stage, change, word in cases:
        desc = _lib.EventSimDesc(**{**ok, "stage": stage, **change})
        assert L.refid_event_sim(ctypes.byref(desc), None) == 1, change
        message = L.refid_last_error().decode()
        assert message.startswith("event_sim:") and word in message, (change, message)
    del equal, back, nan, big                # (alive until here: the descriptors above held their addresses)


def test_ops_event_sim_checks_its_arguments_on_the_host():
    import torch
    from refid_amd import ops
    from refid_amd._lib import RefidHipError
    frames = torch.zeros((3, 4, 5, 3), dtype=torch.uint8)
    state, lut = torch.zeros((4, 5), dtype=torch.int32), torch.from_numpy(R.default_lut())
    with pytest.raises(RefidHipError, match="frames must be a contiguous uint8 \\(N, H, W, 3\\) CUDA tensor .* on cpu"):
        ops.event_sim(frames, [0.0, 1.0, 2.0], state, lut, 13107, 13107)          # no CPU fallback
    with pytest.raises(RefidHipError, match="frames must be .* got ndarray"):
        ops.event_sim(frames.numpy(), [0.0, 1.0, 2.0], state, lut, 13107, 13107)
    with pytest.raises(RefidHipError, match="event_sim_reset: the frame must be .* on cpu"):
        ops.event_sim_reset(frames[0], lut)
    for c, word in ((0, "c_pos 0 must be 1"), (0.2, "c_pos must be an int"), (True, "c_pos must be an int"), (2 ** 31, "c_pos 2147483648")):
        with pytest.raises(RefidHipError, match=word):
            ops._event_sim_threshold("c_pos", c, 4, 5, torch.device("cpu"))
    with pytest.raises(RefidHipError, match="a c_neg map must be a contiguous int32 \\(4, 5\\) tensor"):
        ops._event_sim_threshold("c_neg", torch.zeros((4, 5), dtype=torch.int64), 4, 5, torch.device("cpu"))


def test_the_command_line_names_bad_flags_and_needs_the_gpu(tmp_path, monkeypatch):
    import torch
    from refid_amd import simulate
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    np.save(str(tmp_path / "stack.npy"), np.zeros((3, 4, 4, 3), dtype=np.uint8))
    base = ["--frames", str(tmp_path / "stack.npy"), "--out", str(tmp_path / "out")]
    for extra, word in (([], "exactly one of --fps and --stamps"), (["--fps", "240", "--stamps", "s.txt"], "exactly one of --fps and --stamps"),
                        (["--fps", "fast"], "--fps: 'fast' is not a number"), (["--fps", "0"], "--fps: 0 must be positive"),
                        (["--fps", "240", "--chunk", "1"], "--chunk: 1 must be 2 .. 512"), (["--fps", "240", "--chunk", "513"], "--chunk: 513"),
                        (["--fps", "240", "--split", "1"], "--split: 1 must be"), (["--fps", "240", "--eps", "0"], "--eps: 0.0 must be positive"),
                        (["--fps", "240", "--sigma-c", "-1"], "--sigma-c: -1.0"),
                        (["--fps", "240", "--c-pos", "0.02"], "--c-pos: 0.02 must be at least 0.0271 \\(1776"),
                        (["--fps", "240", "--c-neg", "0"], "--c-neg: 0.0 must be at least"),
                        (["--fps", "240"], "refid_amd.simulate needs the GPU: .* no host fallback"),
                        (["--fps", "240000/1001", "--split", "8", "--c-pos", "0.0271", "--bgr"], "needs the GPU")):
        with pytest.raises(SystemExit, match=word):
            simulate.main(base + extra)
    assert not os.path.exists(tmp_path / "out")
    assert "--split" in simulate.__doc__ and "refid_amd.interpolate" in simulate.__doc__
