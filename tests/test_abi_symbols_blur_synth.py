"""CPU-only: the blur synthesis entry point of include/refid_hip.h -- the ctypes mirror of refid_blur_synth_desc has the
header's field order and types, the constant agrees with the header and with tests/blur_ref.py, the library exports the
entry point, the ABI version stays 9 (additive), a bad descriptor is turned down on the host with a message that names
the field, before anything is launched, ``ops.blur_synth`` checks its arguments on the host, and the command line names a
bad ``--blur`` / ``--gap`` / ``--blur-gamma`` while the messages it had before stay as they were."""
import ctypes
import os
import re

import numpy as np
import pytest

import blur_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "uint8_t": ctypes.c_uint8,
           "float": ctypes.c_float, "double": ctypes.c_double}


def _header():
    with open(os.path.join(ROOT, "include", "refid_hip.h")) as f:
        return f.read()


def _fields(struct_name):
    """[(name, ctypes type)] of a struct of the header, parsed as test_abi_symbols_event_sim.py does: pointers are c_void_p."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct_name, struct_name), _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        mt = re.match(r"^(const\s+)?(uint8_t|int32_t|uint32_t|int64_t|float|double)\s*(.*)$", stmt)
        assert mt, stmt
        for name in mt.group(3).split(","):
            name = name.strip()
            out.append((name.lstrip("*").strip(), ctypes.c_void_p if name.startswith("*") else C_TYPES[mt.group(2)]))
    return out


def test_the_struct_and_constants_match_the_header():
    from refid_amd import _lib
    assert _fields("refid_blur_synth_desc") == list(_lib.BlurSynthDesc._fields_)
    assert [f[0] for f in _lib.BlurSynthDesc._fields_] == [
        "frames", "windows_host", "windows", "to_linear_host", "to_linear", "out", "n_frames", "height", "width", "n_windows", "max_groups"]
    assert ctypes.sizeof(_lib.BlurSynthDesc) == 6 * 8 + 5 * 4 + 4                    # (tail padding to the pointers' 8)
    src = _header()
    const = lambda name: int(re.search(r"#define %s (\d+)" % name, src).group(1))       # noqa: E731
    assert const("REFID_BLUR_MAX_COUNT") == _lib.BLUR_MAX_COUNT == R.MAX_COUNT == 64
    assert re.search(r"int refid_blur_synth\(const refid_blur_synth_desc\* d, void\* stream\);", src)
    assert const("REFID_ABI_VERSION") == 9 == _lib.ABI_VERSION


def test_the_library_exports_the_entry_point():
    from refid_amd import _lib, blur_synth, ops, simulate
    from refid_amd.build import build
    L = ctypes.CDLL(build())
    assert hasattr(L, "refid_blur_synth")
    bound = _lib.lib()
    assert bound.refid_abi_version() == 9                                          # additive: the ABI version stays
    assert bound.refid_blur_synth.argtypes[0]._type_ is _lib.BlurSynthDesc
    assert callable(ops.blur_synth) and callable(blur_synth.synthesize) and callable(blur_synth.gamma_table) and callable(simulate.main)


def test_the_entry_rejects_bad_descriptors_before_any_launch():
    """The argument checks run on the host and launch nothing, so they hold without a GPU (a launch without one would
    return 2, 'launch failed').  The device pointers are never followed; the two host tables are real."""
    from refid_amd import _lib
    L = _lib.lib()
    windows = np.array([[0, 1], [2, 7], [8, 1]], dtype=np.int32)
    table = R.gamma_table(2.2)

    def changed(base, at, value):
        other = base.copy()
        other.reshape(-1)[at] = value
        return other

    zero, many, past, before = changed(windows, 3, 0), changed(windows, 3, 65), changed(windows, 4, 9), changed(windows, 0, -1)
    wide = changed(windows, 1, 10)
    flat, back, high = changed(table, 100, table[99]), changed(table, 7, 0), changed(table, 255, 2 ** 24 + 1)
    ok = dict(frames=4099, windows_host=windows.ctypes.data, windows=8192, to_linear_host=table.ctypes.data, to_linear=12288, out=16387,
              n_frames=9, height=17, width=35, n_windows=3, max_groups=0)
    assert L.refid_blur_synth(None, None) == 1 and "descriptor" in L.refid_last_error().decode()
    cases = [
        (dict(frames=None), "frames is null"), (dict(out=None), "out is null"), (dict(windows_host=None), "windows_host is null"),
        (dict(windows=None), "windows is null"), (dict(windows=8194), "windows is not aligned to 4"),
        (dict(windows_host=windows.ctypes.data + 2), "windows_host is not aligned to 4"),
        (dict(to_linear=12290), "to_linear is not aligned to 4"), (dict(to_linear_host=table.ctypes.data + 1), "to_linear_host is not aligned to 4"),
        (dict(to_linear=None), "to_linear is null but to_linear_host is not"), (dict(to_linear_host=None), "to_linear_host is null but to_linear is not"),
        (dict(n_windows=0), "n_windows 0 must be at least 1"), (dict(n_windows=-3), "n_windows -3"),
        (dict(height=0), "height 0"), (dict(width=0), "width 0"), (dict(width=-5), "width -5"), (dict(n_frames=0), "n_frames 0"),
        (dict(max_groups=-1), "max_groups -1"),
        (dict(windows_host=zero.ctypes.data), "windows[1]: count 0 is not 1 .. 64"),
        (dict(windows_host=many.ctypes.data, n_frames=100), "windows[1]: count 65 is not 1 .. 64"),
        (dict(windows_host=past.ctypes.data), "windows[2]: frames 9 .. 9 lie outside the n_frames 9"),
        (dict(windows_host=wide.ctypes.data), "windows[0]: frames 0 .. 9 lie outside the n_frames 9"),
        (dict(windows_host=before.ctypes.data), "windows[0]: frames -1 .. -1 lie outside"),
        (dict(n_frames=8), "windows[1]: frames 2 .. 8 lie outside the n_frames 8"),
        (dict(to_linear_host=flat.ctypes.data), "to_linear is not strictly increasing: to_linear[100]"),
        (dict(to_linear_host=back.ctypes.data), "to_linear is not strictly increasing: to_linear[7] = 0 after to_linear[6]"),
        (dict(to_linear_host=high.ctypes.data), "to_linear[255] = 16777217 exceeds 2^24"),
        (dict(height=2 ** 21, width=2 ** 20), "height 2097152 * width 1048576 exceed 2^40 pixels"),
        (dict(height=2 ** 20, width=2 ** 20), "make 2415919104 tiles, 2^31 - 1 are the most"),
    ]
    for change, word in cases:
        desc = _lib.BlurSynthDesc(**{**ok, **change})
        assert L.refid_blur_synth(ctypes.byref(desc), None) == 1, change
        message = L.refid_last_error().decode()
        assert message.startswith("blur_synth:") and word in message, (change, message)
    del zero, many, past, before, wide, flat, back, high     # (alive until here: the descriptors above held their addresses)


def test_ops_blur_synth_checks_its_arguments_on_the_host():
    import torch
    from refid_amd import blur_synth, ops
    from refid_amd._lib import RefidHipError
    frames = torch.zeros((3, 4, 5, 3), dtype=torch.uint8)
    with pytest.raises(RefidHipError, match="frames must be a non-empty contiguous uint8 \\(N, H, W, 3\\) CUDA tensor \\(no CPU fallback\\), got .* on cpu"):
        ops.blur_synth(frames, [[0, 2]])
    with pytest.raises(RefidHipError, match="frames must be .* got ndarray"):
        ops.blur_synth(frames.numpy(), [[0, 2]])
    with pytest.raises(RefidHipError, match="no CPU fallback"):
        blur_synth.synthesize(frames, 2, 1)
    with pytest.raises(RefidHipError, match="no CPU fallback"):
        blur_synth.synthesize(frames, 2, 1, gamma=2.2)


def test_the_command_line_names_bad_blur_flags_and_keeps_the_old_messages(tmp_path, monkeypatch):
    import torch
    from refid_amd import simulate
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    np.save(str(tmp_path / "stack.npy"), np.zeros((3, 4, 4, 3), dtype=np.uint8))
    base = ["--frames", str(tmp_path / "stack.npy"), "--out", str(tmp_path / "out")]
    fps, blur = ["--fps", "240"], ["--blur", "3", "--gap", "1"]
    for extra, word in ((fps + blur + ["--split", "8"], "--blur and --split exclude each other"),
                        (fps + ["--gap", "1"], "--gap: needs --blur"), (fps + ["--blur-gamma", "2.2"], "--blur-gamma: needs --blur"),
                        (fps + ["--blur", "3"], "--blur: needs --gap"),
                        (fps + ["--blur", "0", "--gap", "1"], "--blur: 0 must be 1 .. 64"), (fps + ["--blur", "65", "--gap", "1"], "--blur: 65 must be"),
                        (fps + ["--blur", "3", "--gap", "-1"], "--gap: -1 must be 0 .. 100"), (fps + ["--blur", "3", "--gap", "101"], "--gap: 101"),
                        (fps + ["--blur", "40", "--gap", "21"], "--blur 40 --gap 21: a pair has 2 M \\+ N = 101 ground-truth frames"),
                        (fps + blur + ["--blur-gamma", "0.5"], "--blur-gamma: 0.5 must be 1 .. 3"), (fps + blur + ["--blur-gamma", "3.5"], "--blur-gamma: 3.5"),
                        (fps + blur + ["--blur-gamma", "nan"], "--blur-gamma: nan"),
                        # the messages the command line had before come back unchanged from a run that also passes --blur
                        (blur, "exactly one of --fps and --stamps"), (fps + ["--stamps", "s.txt"] + blur, "exactly one of --fps and --stamps"),
                        (["--fps", "fast"] + blur, "--fps: 'fast' is not a number"), (["--fps", "0"] + blur, "--fps: 0 must be positive"),
                        (fps + ["--chunk", "1"] + blur, "--chunk: 1 must be 2 .. 512"), (fps + ["--chunk", "513"] + blur, "--chunk: 513"),
                        (fps + ["--eps", "0"] + blur, "--eps: 0.0 must be positive"), (fps + ["--sigma-c", "-1"] + blur, "--sigma-c: -1.0"),
                        (fps + ["--c-pos", "0.02"] + blur, "--c-pos: 0.02 must be at least 0.0271 \\(1776"),
                        (fps + ["--c-neg", "0"] + blur, "--c-neg: 0.0 must be at least"),
                        (fps + ["--split", "1"], "--split: 1 must be"),
                        (fps + blur, "refid_amd.simulate needs the GPU: .* no host fallback"),
                        (fps + ["--blur", "40", "--gap", "20", "--blur-gamma", "1", "--bgr"], "needs the GPU"),
                        (fps + ["--blur", "1", "--gap", "0", "--blur-gamma", "3"], "needs the GPU")):
        with pytest.raises(SystemExit, match=word):
            simulate.main(base + extra)
    assert not os.path.exists(tmp_path / "out")
    for word in ("--blur M --gap N", "--blur-gamma", "gt_mid", "--layout blur", "refid_amd.deblur", "--split"):
        assert word in simulate.__doc__, word
