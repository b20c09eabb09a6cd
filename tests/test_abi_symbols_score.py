"""CPU-only: the scoring entry points of include/refid_hip.h -- the library exports both symbols, the header declares them
with the argument list the ctypes binding uses, the flag constant agrees, the ABI version stays 9 (additive) -- and the
host half of ``python -m refid_amd.score``: file pairing, size chunks, the report, and the messages that name a file."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_score_entry_points():
    from refid_amd import _lib
    from refid_amd.build import build
    L = ctypes.CDLL(build())
    assert hasattr(L, "refid_score_u8") and hasattr(L, "refid_score_u8_parts")
    assert hasattr(L, "refid_ssim3d_u8") and hasattr(L, "refid_val_tail") and hasattr(L, "refid_niqe_moments")
    bound = _lib.lib()
    assert bound.refid_abi_version() == 9 and _lib.ABI_VERSION == 9
    assert bound.refid_score_u8_parts.restype is ctypes.c_longlong
    assert bound.refid_score_u8_parts(3, 40, 50, 4) == 4 * 3 * 2 * 3           # 32x42 cropped: 2 x 3 tiles, four outputs
    assert bound.refid_score_u8_parts(1, 7, 9, 0) == 4
    for bad in ((0, 8, 8, 0), (1, 8, 8, -1), (1, 8, 8, 4), (1, 9, 8, 4), (100, 4000, 4000, 0)):
        assert bound.refid_score_u8_parts(*bad) == 0, bad                        # what the entry point turns down


def test_binding_matches_the_header():
    from refid_amd import _lib
    src = open(os.path.join(ROOT, "include", "refid_hip.h")).read()
    decl = re.search(r"int refid_score_u8\((.*?)\);", src, re.S).group(1)
    args = [a.strip() for a in decl.replace("\n", " ").split(",")]
    kinds = [ctypes.c_void_p if "*" in a else ctypes.c_int for a in args]
    assert [a.split()[-1].lstrip("*") for a in args] == ["a_u8", "b_u8", "n_frames", "h", "w", "flags", "crop_border", "sq_rgb",
                                                         "sq_y", "ssim3d", "ssim_y", "parts", "ya_out", "ssim_y_map_out", "stream"]
    assert list(_lib.lib().refid_score_u8.argtypes) == kinds
    parts = re.search(r"long long refid_score_u8_parts\((.*?)\);", src, re.S).group(1)
    assert [a.split()[-1] for a in parts.split(",")] == ["n_frames", "h", "w", "crop_border"]
    assert list(_lib.lib().refid_score_u8_parts.argtypes) == [ctypes.c_int] * 4
    assert int(re.search(r"#define REFID_SCORE_BGR (\d+)", src).group(1)) == _lib.SCORE_BGR
    assert int(re.search(r"#define REFID_ABI_VERSION (\d+)", src).group(1)) == 9


def test_refusals_need_no_gpu():
    """Every refusal returns 1 before anything touches the device, and names its cause."""
    from refid_amd._lib import lib
    L = lib()
    fake = ctypes.c_void_p(4096)                                                 # never dereferenced: the call is turned down
    for args, word in (((None, fake, 1, 8, 8, 0, 0), b"NULL frames"), ((fake, None, 1, 8, 8, 0, 0), b"NULL frames"),
                       ((fake, fake, 1, 8, 8, 0, -1), b"negative"), ((fake, fake, 1, 8, 8, 0, 4), b"leaves nothing"),
                       ((fake, fake, 1, 9, 8, 0, 4), b"leaves nothing"), ((fake, fake, 1, 8, 8, 2, 0), b"unknown flags"),
                       ((fake, fake, 100, 4000, 4000, 0, 0), b"31 bits")):
        assert L.refid_score_u8(*args, fake, None, None, None, fake, None, None, None) == 1, args
        assert word in L.refid_last_error(), (args, L.refid_last_error())
    assert L.refid_score_u8(fake, fake, 1, 8, 8, 0, 0, fake, None, None, None, None, None, None, None) == 1
    assert b"need parts" in L.refid_last_error()
    assert L.refid_score_u8(fake, fake, 1, 8, 8, 0, 0, None, None, None, None, fake, None, fake, None) == 1
    assert b"needs ssim_y" in L.refid_last_error()


def _touch_png(path, h=4, w=5, value=0):
    from refid_amd.png import write_png
    write_png(str(path), np.full((h, w, 3), value, dtype=np.uint8))


def test_pairing_two_directories(tmp_path):
    from refid_amd._lib import RefidHipError
    from refid_amd.score import pair_files, png_key, size_chunks
    for name in ("b", "a", "c"):
        _touch_png(tmp_path / "pred" / f"{name}.png")
        _touch_png(tmp_path / "gt" / f"{name}.png")
    (tmp_path / "gt" / "notes.txt").write_text("not a frame")
    pairs = pair_files(str(tmp_path / "pred"), str(tmp_path / "gt"))
    assert [p[0] for p in pairs] == ["a.png", "b.png", "c.png"]
    assert pairs[1][1:] == (str(tmp_path / "pred" / "b.png"), str(tmp_path / "gt" / "b.png"))
    assert png_key(pairs[0][1]) == (4, 5, 2)
    assert [[p[0] for p in c] for c in size_chunks(pairs, per=2)] == [["a.png", "b.png"], ["c.png"]]
    _touch_png(tmp_path / "pred" / "d.png")
    with pytest.raises(RefidHipError, match=r"pred/d\.png has no ground truth .*gt/d\.png"):
        pair_files(str(tmp_path / "pred"), str(tmp_path / "gt"))
    os.remove(tmp_path / "pred" / "d.png")
    _touch_png(tmp_path / "gt" / "e.png")
    with pytest.raises(RefidHipError, match=r"gt/e\.png has no prediction .*pred/e\.png"):
        pair_files(str(tmp_path / "pred"), str(tmp_path / "gt"))
    os.remove(tmp_path / "gt" / "e.png")
    _touch_png(tmp_path / "gt" / "b.png", h=6)                                   # the sizes of a pair differ
    with pytest.raises(RefidHipError, match=r"pred/b\.png is 4x5, its ground truth .*gt/b\.png is 6x5"):
        size_chunks(pair_files(str(tmp_path / "pred"), str(tmp_path / "gt")))
    _touch_png(tmp_path / "pred" / "b.png", h=6)                                 # a new size starts a new chunk
    chunks = size_chunks(pair_files(str(tmp_path / "pred"), str(tmp_path / "gt")), per=8)
    assert [[p[0] for p in c] for c in chunks] == [["a.png"], ["b.png"], ["c.png"]]
    (tmp_path / "pred" / "c.png").write_bytes(b"no png")
    with pytest.raises(RefidHipError, match=r"pred/c\.png is not a PNG"):
        size_chunks(pair_files(str(tmp_path / "pred"), str(tmp_path / "gt")))
    with pytest.raises(RefidHipError, match="not a directory"):
        pair_files(str(tmp_path / "pred"), str(tmp_path / "nowhere"))
    with pytest.raises(RefidHipError, match="--gt-suffix"):
        pair_files(str(tmp_path / "pred"), str(tmp_path / "pred"))


def test_pairing_suffix_siblings(tmp_path):
    """The validation loop's X.png / X_gt.png dumps in one directory; the suffix also works across two directories."""
    from refid_amd._lib import RefidHipError
    from refid_amd.score import pair_files
    d = tmp_path / "val"
    for name in ("000001_00", "000000_00"):
        _touch_png(d / f"{name}.png")
        _touch_png(d / f"{name}_gt.png")
    pairs = pair_files(str(d), None, "_gt")
    assert [p[0] for p in pairs] == ["000000_00.png", "000001_00.png"]
    assert pairs[0][2] == str(d / "000000_00_gt.png")
    _touch_png(d / "000002_00.png")
    with pytest.raises(RefidHipError, match=r"000002_00\.png has no ground truth .*000002_00_gt\.png"):
        pair_files(str(d), None, "_gt")
    os.remove(d / "000002_00.png")
    _touch_png(d / "000003_00_gt.png")
    with pytest.raises(RefidHipError, match=r"000003_00_gt\.png has no prediction .*000003_00\.png"):
        pair_files(str(d), None, "_gt")
    os.remove(d / "000003_00_gt.png")
    _touch_png(tmp_path / "p" / "x.png")
    _touch_png(tmp_path / "g" / "x_gt.png")
    assert pair_files(str(tmp_path / "p"), str(tmp_path / "g"), "_gt") == [
        ("x.png", str(tmp_path / "p" / "x.png"), str(tmp_path / "g" / "x_gt.png"))]
    with pytest.raises(RefidHipError, match="no prediction"):
        pair_files(str(tmp_path / "g"), None, "_gt")                              # only ground truth there


def test_report_lines_and_host_finish():
    import torch
    from refid_amd.score import Scores, format_lines, psnr_y_from_sq, scores_from_words
    lines = format_lines(["a.png", "b.png"], ["psnr", "niqe"], [(30.0, 4.5), (float("inf"), float("nan"))])
    assert lines == ["# file psnr niqe", "a.png 30.000000 4.500000", "b.png inf nan", "mean inf 4.500000"]
    words = torch.zeros((4, 2), dtype=torch.int64)
    words[0] = torch.tensor([0, 3 * 6 * 255 * 255])
    f64 = words.view(torch.float64)
    f64[1] = torch.tensor([0.0, 6.0 * 4.0])
    f64[2] = torch.tensor([18.0, 9.0])
    f64[3] = torch.tensor([6.0, 3.0])
    sc = scores_from_words(words, 2, 3, True, True, True, True)
    assert sc == Scores([float("inf"), 0.0], [1.0, 0.5], [float("inf"), psnr_y_from_sq(24.0, 6)], [1.0, 0.5])
    assert abs(sc.psnr_y[1] - 20 * np.log10(255.0 / 2.0)) < 1e-12
    assert scores_from_words(words, 2, 3, False, True, False, False) == Scores(None, [1.0, 0.5], None, None)
