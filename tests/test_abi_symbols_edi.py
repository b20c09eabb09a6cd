"""CPU-only: the double integral's entry point of include/refid_hip.h -- the ctypes mirror of refid_edi_desc has the header's
field order and types, the constants agree with the header and with tests/edi_ref.py, the library exports the entry point,
the ABI version stays 9 (additive), a bad descriptor is turned down on the host with a message that names the field,
before anything is launched, ``ops.edi`` and the runners check their arguments on the host, and the command lines name a
bad ``--method edi`` flag while the messages they had before stay as they were."""
import ctypes
import os
import re

import numpy as np
import pytest

import edi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "uint8_t": ctypes.c_uint8,
           "int8_t": ctypes.c_int8, "float": ctypes.c_float, "double": ctypes.c_double}


def _header():
    with open(os.path.join(ROOT, "include", "refid_hip.h")) as f:
        return f.read()


def _fields(struct_name):
    """[(name, ctypes type)] of a struct of the header, parsed as test_abi_symbols_blur_synth.py does: pointers are c_void_p."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct_name, struct_name), _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        mt = re.match(r"^(const\s+)?(uint8_t|int8_t|int32_t|uint32_t|int64_t|float|double)\s*(.*)$", stmt)
        assert mt, stmt
        for name in mt.group(3).split(","):
            name = name.strip()
            out.append((name.lstrip("*").strip(), ctypes.c_void_p if name.startswith("*") else C_TYPES[mt.group(2)]))
    return out


def test_the_struct_and_constants_match_the_header():
    from refid_amd import _lib
    assert _fields("refid_edi_desc") == list(_lib.EdiDesc._fields_)
    assert [f[0] for f in _lib.EdiDesc._fields_] == [
        "frames", "ev_t", "ev_p", "seg", "items_host", "items", "bounds_host", "bounds", "samples_host", "samples", "instants_host",
        "instants", "tables", "out", "clamped", "eps255", "n_events", "n_frames", "height", "width", "n_items", "n_instants", "m",
        "exposure", "c_pos", "c_neg"]
    assert ctypes.sizeof(_lib.EdiDesc) == 15 * 8 + 8 + 8 + 9 * 4 + 4                 # (tail padding to the pointers' 8)
    src = _header()
    const = lambda name: int(re.search(r"#define %s (\d+)" % name, src).group(1))       # noqa: E731
    assert const("REFID_EDI_SAMPLES") == _lib.EDI_SAMPLES == R.SAMPLES == 0
    assert const("REFID_EDI_CONTINUOUS") == _lib.EDI_CONTINUOUS == R.CONTINUOUS == 1
    assert const("REFID_EDI_THREADS") == _lib.EDI_THREADS == 256
    assert const("REFID_EDI_CLAMP") == _lib.EDI_CLAMP == R.CLAMP == 32
    assert const("REFID_EDI_TABLE") == _lib.EDI_TABLE == R.TABLE == 577
    assert const("REFID_EDI_MAX_INSTANTS") == _lib.EDI_MAX_INSTANTS == R.MAX_INSTANTS == 256
    assert const("REFID_EDI_MAX_ITEMS") == _lib.EDI_MAX_ITEMS == 65535
    assert const("REFID_EDI_MAX_PIXELS") == _lib.EDI_MAX_PIXELS == R.MAX_PIXELS == 1 << 25
    assert const("REFID_EDI_MAX_THRESHOLD") == _lib.EDI_MAX_THRESHOLD == R.MAX_THRESHOLD == 1 << 20
    assert const("REFID_BLUR_MAX_COUNT") == _lib.BLUR_MAX_COUNT == R.MAX_COUNT
    assert re.search(r"int refid_edi\(const refid_edi_desc\* d, void\* stream\);", src)
    assert const("REFID_ABI_VERSION") == 9 == _lib.ABI_VERSION


def test_the_library_exports_the_entry_point():
    from refid_amd import _lib, deblur, edi, interpolate, ops
    from refid_amd.build import build
    L = ctypes.CDLL(build())
    assert hasattr(L, "refid_edi")
    bound = _lib.lib()
    assert bound.refid_abi_version() == 9                                          # additive: the ABI version stays
    assert bound.refid_edi.argtypes[0]._type_ is _lib.EdiDesc
    assert callable(ops.edi) and callable(edi.EdiInterpolator) and callable(edi.EdiDeblurrer) and callable(edi.EdiStream)
    assert callable(interpolate.main) and callable(deblur.main)
    assert np.array_equal(edi.gain_tables(), R.gain_tables()) and edi.to_fixed(0.2) == R.to_fixed(0.2) == 13107


def test_the_entry_rejects_bad_descriptors_before_any_launch():
    """The argument checks run on the host and launch nothing, so they hold without a GPU (a launch without one would
    return 2, 'launch failed').  The device pointers are never followed; the host tables are real."""
    from refid_amd import _lib
    L = _lib.lib()
    items = np.array([[0, 1], [1, -1]], dtype=np.int32)
    bounds = np.array([[1.0, 1.5, 2.0, 2.5], [2.0, 2.5, 0.0, 0.0]], dtype=np.float32)
    instants = np.array([[1.0, 1.75, 2.5], [2.0, 2.25, 2.5]], dtype=np.float32)
    samples = np.array([[1.0, 1.5, 2.0, 2.5], [2.0, 2.5, 9.0, 9.0]], dtype=np.float32)          # (m = 2; no right key: not read)

    def changed(base, at, value):
        other = base.copy()
        other.reshape(-1)[at] = value
        return other

    bad = {"left": changed(items, 0, 3), "left_neg": changed(items, 2, -1), "right": changed(items, 1, 3),
           "order": changed(bounds, 1, 2.25), "order_single": changed(bounds, 5, 1.0), "nan": changed(bounds, 2, np.nan),
           "tau_out": changed(instants, 2, 2.75), "tau_single": changed(instants, 5, 2.75), "tau_back": changed(instants, 1, 0.5 + 0.25),
           "tau_desc": changed(instants, 2, 1.5), "smp_out": changed(samples, 1, 1.75), "smp_desc": changed(samples, 3, 1.5 + 0.25),
           "smp_right": changed(samples, 2, 1.75)}
    bad["smp_desc"] = changed(changed(samples, 2, 2.5), 3, 2.25)
    ok = dict(frames=4099, ev_t=8192, ev_p=12289, seg=16384, items_host=items.ctypes.data, items=20480, bounds_host=bounds.ctypes.data,
              bounds=24576, samples_host=samples.ctypes.data, samples=28672, instants_host=instants.ctypes.data, instants=32768,
              tables=36864, out=40961, clamped=45056, eps255=0.255, n_events=10, n_frames=3, height=5, width=67, n_items=2, n_instants=3,
              m=2, exposure=0, c_pos=13107, c_neg=13107)
    assert L.refid_edi(None, None) == 1 and "descriptor" in L.refid_last_error().decode()
    host = lambda name: bad[name].ctypes.data               # noqa: E731
    cases = [
        (dict(frames=None), "frames is null"), (dict(out=None), "out is null"), (dict(seg=None), "seg is null"), (dict(ev_t=None), "ev_t is null"),
        (dict(ev_p=None), "ev_p is null"), (dict(items=None), "items is null"), (dict(items_host=None), "items_host is null"),
        (dict(bounds=None), "bounds is null"), (dict(instants_host=None), "instants_host is null"), (dict(tables=None), "tables is null"),
        (dict(clamped=None), "clamped is null"), (dict(seg=16386), "seg is not aligned to 4"), (dict(ev_t=8194), "ev_t is not aligned to 4"),
        (dict(tables=36868), "tables is not aligned to 8"), (dict(clamped=45058), "clamped is not aligned to 4"),
        (dict(bounds=24577), "bounds is not aligned to 4"), (dict(samples=None), "samples is null but samples_host is not"),
        (dict(samples_host=None), "samples_host is null but samples is not"),
        (dict(samples=None, samples_host=None), "samples is null in REFID_EDI_SAMPLES mode"),
        (dict(exposure=1), "samples is given in REFID_EDI_CONTINUOUS mode"), (dict(exposure=2), "exposure 2 is neither"),
        (dict(n_items=0), "n_items 0 is not 1 .. 65535"), (dict(n_items=65536), "n_items 65536"),
        (dict(n_instants=0), "n_instants 0 is not 1 .. 256"), (dict(n_instants=257), "n_instants 257"),
        (dict(m=0), "m 0 is not 1 .. 64"), (dict(m=65), "m 65 is not 1 .. 64"), (dict(height=0), "height 0"), (dict(width=-5), "width -5"),
        (dict(height=8192, width=8192), "height 8192 \\* width 8192 = 67108864 pixels exceed 33554432"), (dict(n_frames=0), "n_frames 0"),
        (dict(n_events=-1), "n_events -1 is not 0 .. 2\\^31 - 1"), (dict(n_events=2 ** 31), "n_events 2147483648"),
        (dict(c_pos=0), "c_pos 0 is not 1 .. 1048576"), (dict(c_neg=1048577), "c_neg 1048577 is not"),
        (dict(eps255=-0.1), "eps255 -0.1 must be finite"), (dict(eps255=float("nan")), "eps255 nan"),
        (dict(items_host=host("left")), "items\\[0\\]: left 3 lies outside the n_frames 3"),
        (dict(items_host=host("left_neg")), "items\\[1\\]: left -1 lies outside"),
        (dict(items_host=host("right")), "items\\[0\\]: right 3 lies outside the n_frames 3"),
        (dict(n_frames=1), "items\\[0\\]: right 1 lies outside the n_frames 1"),
        (dict(bounds_host=host("order")), "bounds\\[0\\] = \\[1, 2.25, 2, 2.5\\] is not ordered s0 <= e0 <= s1 <= e1"),
        (dict(bounds_host=host("order_single")), "bounds\\[1\\] = \\[2, 1, 0, 0\\] is not ordered"),
        (dict(bounds_host=host("nan")), "bounds\\[0\\]\\[2\\] is not finite"),
        (dict(instants_host=host("tau_out")), "instants\\[0\\]\\[2\\] = 2.75 lies outside \\[1, 2.5\\]"),
        (dict(instants_host=host("tau_single")), "instants\\[1\\]\\[2\\] = 2.75 lies outside \\[2, 2.5\\]"),
        (dict(instants_host=host("tau_back")), "instants\\[0\\]\\[1\\] = 0.75 lies outside"),
        (dict(instants_host=host("tau_desc")), "instants\\[0\\] is not ascending: \\[2\\] = 1.5 after 1.75"),
        (dict(samples_host=host("smp_out")), "samples\\[0\\]\\[1\\] = 1.75 lies outside \\[1, 1.5\\]"),
        (dict(samples_host=host("smp_right")), "samples\\[0\\]\\[2\\] = 1.75 lies outside \\[2, 2.5\\]"),
        (dict(samples_host=host("smp_desc")), "samples\\[0\\] is not ascending: \\[3\\] = 2.25 after 2.5"),
    ]
    for change, word in cases:
        desc = _lib.EdiDesc(**{**ok, **change})
        assert L.refid_edi(ctypes.byref(desc), None) == 1, change
        message = L.refid_last_error().decode()
        assert message.startswith("edi:") and re.search(word, message), (change, message)
    empty = _lib.EdiDesc(**{**ok, "n_events": 0, "ev_t": None, "ev_p": None, "height": 0})       # an empty stream needs neither array
    assert L.refid_edi(ctypes.byref(empty), None) == 1 and "height 0" in L.refid_last_error().decode()
    del bad


def test_ops_edi_and_the_runners_check_their_arguments_on_the_host():
    import torch
    from refid_amd import edi, ops
    from refid_amd._lib import RefidHipError
    frames = torch.zeros((3, 4, 5, 3), dtype=torch.uint8)
    with pytest.raises(RefidHipError, match="edi: frames must be a non-empty contiguous uint8 \\(N, H, W, 3\\) CUDA tensor \\(no CPU fallback\\), got .* on cpu"):
        ops.edi(frames, None, [[0, 1]], [[0, 0, 1, 1]], [[0.5]])
    with pytest.raises(RefidHipError, match="frames must be .* got ndarray"):
        ops.edi(frames.numpy(), None, [[0, 1]], [[0, 0, 1, 1]], [[0.5]])
    for kw, word in ((dict(device="cpu"), "a GPU device is required \\(csrc/edi.hip has no host fallback\\)"),
                     (dict(exposure="open"), "unknown exposure 'open'"), (dict(m=65, layout="blur"), "m 65 must be 1 .. 64"),
                     (dict(c_pos=0.0), "c_pos 0.0 must be at least 2\\^-16"), (dict(c_neg=float("nan")), "c_neg nan"),
                     (dict(eps=-1.0), "eps -1.0 must be finite"), (dict(max_minibatch=0), "max_minibatch 0"),
                     (dict(layout="single"), "unknown layout 'single'"), (dict(n=0), "n 0 must be at least 1 for layout 'sharp'"),
                     (dict(m=64, n=200, layout="blur"), "328 output frames per item, 256 are the most")):
        with pytest.raises(RefidHipError, match="EdiInterpolator: " + word):
            edi.EdiInterpolator(**{**dict(m=1, n=3, device="cuda" if "device" not in kw else kw["device"]), **kw})
    with pytest.raises(RefidHipError, match="EdiDeblurrer: a GPU device is required"):
        edi.EdiDeblurrer(3, device="cpu")
    with pytest.raises(RefidHipError, match="EdiStream: a GPU device is required"):
        edi.EdiStream("cpu")
    with pytest.raises(RefidHipError, match="exposure_pairs: 3 exposure starts, 2 exposure ends"):
        edi.exposure_pairs([0, 1, 2], [0, 1])
    pairs = edi.exposure_pairs([0.0, 1.0, 2.0], [0.5, 1.5, 2.5])
    assert pairs == [edi.EdiPair(0, 1, 0, 0, 0.0, 1.5, 0.5, 1.0), edi.EdiPair(1, 2, 0, 0, 1.0, 2.5, 1.5, 2.0)]


def test_the_command_lines_name_bad_edi_flags_and_keep_the_old_messages(tmp_path, monkeypatch):
    import torch
    from refid_amd import deblur, interpolate
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    base = ["--frames", str(tmp_path / "none.npy"), "--events", str(tmp_path / "none.npz"), "--stamps", str(tmp_path / "none.txt"),
            "--out", str(tmp_path / "out")]
    edi = ["--method", "edi"]
    shared = ((edi + ["--checkpoint", "net.pth"], "--checkpoint: --method edi runs no network and takes no checkpoint"),
              (edi + ["--opt", "test.yml"], "--opt: --method edi runs no network"),
              (edi + ["--c-pos", "0"], "--c-pos: 0.0 must be at least 2\\^-16 and at most 16"), (edi + ["--c-neg", "17"], "--c-neg: 17.0 must be"),
              (edi + ["--c-pos", "nan"], "--c-pos: nan"), (edi + ["--eps", "-1"], "--eps: -1.0 must be finite and not negative"),
              (edi + ["--eps", "inf"], "--eps: inf"), (["--c-pos", "0.2"], "--c-pos: needs --method edi"),
              (["--c-neg", "0.2"], "--c-neg: needs --method edi"), (["--edi-exposure", "continuous"], "--edi-exposure: needs --method edi"),
              (["--eps", "0.001"], "--eps: needs --method edi"), (["--method", "network", "--eps", "0.001"], "--eps: needs --method edi"))
    for main, prog, own in ((interpolate.main, "refid_amd.interpolate", ["--n", "3"]), (deblur.main, "refid_amd.deblur", ["--m", "3"])):
        for extra, word in shared + ((edi + own, f"{prog} --method edi needs the GPU: .* no host fallback"),
                                     (edi + own + ["--edi-exposure", "continuous", "--c-pos", "0.3"], "needs the GPU")):
            with pytest.raises(SystemExit, match=word):
                main(base + extra)
        with pytest.raises(SystemExit) as ex:                  # argparse turns an unknown choice down itself
            main(base + edi + ["--edi-exposure", "open"])
        assert ex.value.code == 2
    with pytest.raises(SystemExit, match="--m: needs --method edi"):
        deblur.main(base + ["--m", "3"])
    # blurry frames in samples mode need M: it is not taken to be 1 in silence; what only the network reads is refused
    for main, extra, word in ((deblur.main, [], "--m: --method edi with --edi-exposure samples needs the number of frames"),
                              (interpolate.main, ["--n", "1", "--layout", "blur"], "--m: --method edi --layout blur with --edi-exposure samples"),
                              (interpolate.main, [], "--method edi: give --n"),
                              (deblur.main, ["--m", "3", "--stamps-mode", "bounds"], "--stamps-mode: --method edi runs no network and does not read it"),
                              (deblur.main, ["--m", "3", "--num-bins", "6"], "--num-bins: --method edi"),
                              (deblur.main, ["--m", "3", "--crop-size", "64"], "--crop-size: --method edi"),
                              (deblur.main, ["--edi-exposure", "continuous"], "needs the GPU"),
                              (interpolate.main, ["--n", "1", "--layout", "blur", "--edi-exposure", "continuous"], "needs the GPU"),
                              (interpolate.main, ["--n", "7"], "needs the GPU")):
        with pytest.raises(SystemExit, match=word):
            main(base + edi + extra)
    # the messages the command lines had before come back unchanged, with and without the new flag's default
    for extra in ([], ["--method", "network"]):
        with pytest.raises(SystemExit, match="give --opt \\(datasets.test.num_inter_interpolation\\) or --n"):
            interpolate.main(base + extra)
        with pytest.raises(SystemExit, match="give --opt \\(datasets.test.num_bins\\) or --num-bins"):
            deblur.main(base + extra)
        with pytest.raises(SystemExit, match="give --out, --video or both"):
            interpolate.main(base[:-2] + extra)
        with pytest.raises(SystemExit, match="--video-quality: 'best' is not an integer 1 .. 100"):
            deblur.main(base + extra + ["--video", "v.avi", "--video-quality", "best"])
    with pytest.raises(SystemExit, match="--gt and --niqe write their files into --out: give --out"):
        interpolate.main(base[:-2] + edi + ["--video", "v.avi", "--gt", "gt"])
    assert not os.path.exists(tmp_path / "out")
    for doc in (interpolate.__doc__, deblur.__doc__):
        for word in ("--method edi", "--c-pos", "refid_amd.edi", "no checkpoint"):
            assert word in doc, word
