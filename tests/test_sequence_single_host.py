"""CPU-only: deblurring whole sequences -- the numpy restatement of refid_seq_assemble_single (tests/sequence_single_ref.py)
against the reference's own __getitem__ on a sequence fixture (tests/golden/seq_single_whole.npz,
tools/make_seq_single_golden.py), and the host-side layers above the kernels: frame_windows, the command line's settings,
the ctypes mirror, the rejections that need no GPU.

The comparisons are those of test_single_assembly_host.py, with no new tolerance: lq bit for bit; the pre-norm voxel
under check_voxel ((cnt+1)*mass*2^-24 against the reference's sequential fp32 sum, cnt*2^-32 + ulp/2 against float64) with
the same non-zero mask; the restated normalisation of THE REFERENCE's pre-norm voxel within (1 + d_ref) * B of the
reference's normalised voxel and within B of float64, B = single_assembly_ref.bound."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest

import sequence_single_ref as R
import single_assembly_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _items(z, stamps="events"):
    from refid_amd.sequence import frame_windows, make_pairs
    w = z["windows"]
    return make_pairs(z["events"][:, 0], *frame_windows(w[:, 0], w[:, 1]), stamps=stamps)


# ---- the restatement against the reference-generated fixture -------------------------------------------------------------
def test_fixture_is_the_sequence_the_tests_need(golden_dir):
    z, bins = R.load_fixture(golden_dir)
    assert bins == 6 and z["frames"].shape == (3, 26, 38, 3) and z["frames"].dtype == np.uint8
    ev = z["events"]
    assert ev.dtype == np.float32 and 2500 <= len(ev) <= 3500 and np.all(ev[1:, 0] >= ev[:-1, 0])
    items = _items(z)
    assert [[p.row0, p.row1] for p in items] == z["rows"].tolist() and [p.left for p in items] == [0, 1, 2]
    assert items[0].row1 > items[1].row0, "windows 0 and 1 overlap"
    for k, p in enumerate(items):                          # the reference's stamps (event_util.py:25-31) are stamps='events'
        assert (p.first_stamp, p.last_stamp) == (float(ev[p.row0, 0]), float(ev[p.row1 - 1, 0]))
        assert z[f"i{k}/pre"].shape == z[f"i{k}/voxel"].shape == (6, 26, 38) and z[f"i{k}/lq"].shape == (3, 26, 38)


def test_stage1_assembly_matches_the_reference(golden_dir):
    z, bins = R.load_fixture(golden_dir)
    ev = z["events"]
    for k, item in enumerate(_items(z)):
        what = f"item {k}"
        lq, voxel, pre = R.assemble_item(z["frames"], ev, item, bins, 26, 38, bgr=True)
        assert np.array_equal(lq.view(np.uint32), z[f"i{k}/lq"].view(np.uint32)), what
        e, cnt, mass = S.float64_sums(ev[item.row0:item.row1], bins, 26, 38, 0, 0, 26, 38, False, False, False)
        assert cnt.max() >= 20, (what, "a hot pixel must be inside the window")
        S.check_voxel(pre, z[f"i{k}/pre"], e, cnt, mass, what)
        assert np.array_equal(pre != 0, z[f"i{k}/pre"] != 0), what              # the same mask: the same S0
        assert np.array_equal(S.normalise(pre, acc=True).view(np.uint32), voxel.view(np.uint32)), what


def test_stage2_normalisation_matches_the_reference(golden_dir):
    z, bins = R.load_fixture(golden_dir)
    for k in range(3):
        what = f"item {k}"
        ref_pre, ref_out, d_ref = z[f"i{k}/pre"], z[f"i{k}/voxel"], float(z[f"i{k}/d_ref"])
        out = S.normalise(ref_pre)
        x64, mu, sigma = S.float64_norm(ref_pre)
        b = S.bound(ref_pre, mu, sigma, ref_pre.size)
        nz = ref_pre != 0
        assert nz.sum() > 500 and np.all(out[~nz] == 0) and np.all(ref_out[~nz] == 0), what
        d64 = np.abs(out.astype(np.float64) - x64)
        assert np.all(d64[nz] <= b[nz]), (what, "vs float64", float((d64[nz] / b[nz]).max()))
        d = np.abs(out.astype(np.float64) - ref_out.astype(np.float64))
        assert np.all(d[nz] <= (1 + d_ref) * b[nz]), (what, float((d[nz] / b[nz]).max()), d_ref)


def test_padding_is_edge_for_images_zero_for_voxels_and_outside_the_statistics(golden_dir):
    z, bins = R.load_fixture(golden_dir)
    items = _items(z)
    lq, voxel = R.assemble_items(z["frames"], z["events"], items, bins, multiple=4, bgr=True)
    assert lq.shape == (3, 3, 28, 40) and voxel.shape == (3, 6, 28, 40)
    assert np.all(voxel[:, :, 26:] == 0) and np.all(voxel[:, :, :, 38:] == 0) and np.abs(voxel).max() > 3
    assert np.all(lq[:, :, 26:, :] == lq[:, :, 25:26, :]) and np.all(lq[:, :, :, 38:] == lq[:, :, :, 37:38])
    assert lq[1, 0, 3, 5] == np.float32(z["frames"][1, 3, 5, 2]) / np.float32(255)     # BGR input: R comes from channel 2
    lq1, voxel1 = R.assemble_items(z["frames"], z["events"], items, bins, multiple=1, bgr=True)
    assert lq1.shape == (3, 3, 26, 38) and voxel1.shape == (3, 6, 26, 38)
    assert np.array_equal(voxel[:, :, :26, :38].view(np.uint32), voxel1.view(np.uint32))   # padding changes no statistic
    assert np.array_equal(lq[:, :, :26, :38].view(np.uint32), lq1.view(np.uint32))
    rgb, _ = R.assemble_items(z["frames"], z["events"], items, bins, multiple=1, bgr=False)
    assert np.array_equal(rgb, lq1[:, ::-1])
    plain = R.assemble_items(z["frames"], z["events"], items, bins, multiple=4, norm=False, bgr=True)[1]
    assert np.array_equal(plain[0, :, :26, :38], R.assemble_item(z["frames"], z["events"], items[0], bins, 26, 38)[2])


# ---- frame_windows -----------------------------------------------------------------------------------------------------
def test_frame_windows_with_make_pairs():
    from refid_amd._lib import RefidHipError
    from refid_amd.sequence import frame_windows, make_pairs
    t = np.array([1, 2, 2, 2, 3, 5, 5, 8], dtype=np.float32)
    l, r, b, e = frame_windows([1, 2, 6, 3], [2, 5, 7, 9])
    assert (l.tolist(), r.tolist(), b.tolist(), e.tolist()) == ([0, 1, 2, 3], [0, 1, 2, 3], [1, 2, 6, 3], [2, 5, 7, 9])
    items = make_pairs(t, l, r, b, e)
    # half-open: the 2s open window 1, the 5s are outside it; [6, 7) holds no event: rows (7, 7), stamps (0, 0)
    assert [tuple(p) for p in items] == [(0, 0, 0, 1, 1.0, 1.0), (1, 1, 1, 5, 2.0, 3.0), (2, 2, 7, 7, 0.0, 0.0),
                                         (3, 3, 4, 8, 3.0, 8.0)]
    bounds = make_pairs(t, l, r, b, e, stamps="bounds")
    assert [tuple(p) for p in bounds] == [(0, 0, 0, 1, 1.0, 2.0), (1, 1, 1, 5, 2.0, 5.0), (2, 2, 7, 7, 6.0, 7.0),
                                          (3, 3, 4, 8, 3.0, 9.0)]
    assert [len(v) for v in frame_windows([], [])] == [0, 0, 0, 0]
    with pytest.raises(RefidHipError, match="2 exposure starts, 1 exposure ends"):
        frame_windows([1, 2], [3])


# ---- the command line's settings -----------------------------------------------------------------------------------------
TEST_YAML = """
name: tiny-deblur
model_type: TestImageEventRestorationModel
num_gpu: 1
datasets:
  test:
    name: highrev-test
    type: GoProSingleImageEventDataset
    num_bins: 6
network_g:
  type: SingleMultiConnectEVHINet
  wf: 8
  depth: 3
  ev_chn: 6
val:
  max_minibatch: 2
  crop_size: 24
path:
  pretrain_network_g: ~
"""


def test_deblur_settings(tmp_path):
    from refid_amd import deblur as D
    ns = lambda **kw: argparse.Namespace(**dict(dict(opt=None, checkpoint=None, num_bins=None, max_minibatch=None,  # noqa: E731
                                                     crop_size=None), **kw))
    yml = tmp_path / "t.yml"
    yml.write_text(TEST_YAML)
    net, ckpt, bins, mb, crop = D.settings(ns(opt=str(yml)))
    assert net == dict(type="SingleMultiConnectEVHINet", wf=8, depth=3, ev_chn=6)
    assert (ckpt, bins, mb, crop) == (None, 6, 2, None), "val.crop_size counts only when val.grids is set"
    grids = tmp_path / "g.yml"
    grids.write_text(TEST_YAML.replace("val:\n", "val:\n  grids: true\n"))
    assert D.settings(ns(opt=str(grids)))[2:] == (6, 2, 24)
    assert D.settings(ns(opt=str(grids), checkpoint="w.pth", num_bins=2, max_minibatch=5, crop_size=32))[1:] == ("w.pth", 2, 5, 32)
    nocrop = tmp_path / "n.yml"
    nocrop.write_text(TEST_YAML.replace("val:\n", "val:\n  grids: true\n").replace("  crop_size: 24\n", ""))
    with pytest.raises(SystemExit, match="val.crop_size"):
        D.settings(ns(opt=str(nocrop)))
    net, ckpt, bins, mb, crop = D.settings(ns(checkpoint="w.pth", num_bins=6))
    assert net == dict(type="SingleMultiConnectEVHINet", ev_chn=6) and (ckpt, bins, mb, crop) == ("w.pth", 6, 1, None)
    with pytest.raises(SystemExit, match="--num-bins"):
        D.settings(ns(checkpoint="w.pth"))


# ---- the C ABI and its mirror ------------------------------------------------------------------------------------------
C_TYPES = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float}


def _fields(struct_name):
    """[(name, ctypes type)] of a struct of the header: pointers are c_void_p."""
    src = open(os.path.join(ROOT, "include", "refid_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct_name, struct_name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for stmt in (s.strip() for s in body.split(";")):
        if not stmt:
            continue
        mt = re.match(r"^(const\s+)?(unsigned char|long long|float|int|void|refid_seq_pair)\s*(.*)$", stmt)
        assert mt, stmt
        for name in (n.strip() for n in mt.group(3).split(",")):
            out.append((name.lstrip("*").strip(), ctypes.c_void_p if name.startswith("*") else C_TYPES[mt.group(2)]))
    return out


def test_header_and_ctypes_mirror_agree():
    from refid_amd import _lib
    from refid_amd.build import build
    assert _fields("refid_seq_single_desc") == list(_lib.SeqSingleDesc._fields_)
    names = [f[0] for f in _lib.SeqSingleDesc._fields_]
    resident = ["events", "n_events", "frames", "n_frames", "frame_stride", "row_pitch", "height", "width", "bgr"]
    assert names[:9] == resident == [f[0] for f in _lib.SeqDesc._fields_[:9]]
    assert names[9:] == ["items_host", "items_dev", "n_items", "bins", "norm", "out_h", "out_w", "scratch", "parts", "lq", "voxel"]
    assert ctypes.sizeof(_lib.SeqPair) == 32 and ctypes.sizeof(_lib.SeqDesc) == 120 and ctypes.sizeof(_lib.SingleDesc) == 80
    L = ctypes.CDLL(build())
    for sym in ("refid_seq_assemble_single", "refid_seq_assemble", "refid_assemble_single", "refid_voxel_norm"):
        assert hasattr(L, sym), sym
    bound = _lib.lib()
    assert bound.refid_seq_assemble_single.argtypes[0]._type_ is _lib.SeqSingleDesc
    assert bound.refid_abi_version() == 9 == _lib.ABI_VERSION                  # purely additive


def test_rejections_without_a_gpu():
    from refid_amd._lib import RefidHipError
    from refid_amd.build import build
    from refid_amd.sequence import SequenceAssembler
    build()
    with pytest.raises(RefidHipError, match="img2tensor"):
        SequenceAssembler(layout="single", num_bins=3)
    with pytest.raises(RefidHipError, match="num_bins >= 1"):
        SequenceAssembler(layout="single", num_bins=0)
    with pytest.raises(RefidHipError, match="unknown layout 'double'"):
        SequenceAssembler(1, 1, layout="double")
    a = SequenceAssembler(layout="single", num_bins=6)
    assert (a.layout, a.bins, a.multiple, a.norm_voxel) == ("single", 6, 4, True)
    assert SequenceAssembler(layout="single", num_bins=2, norm_voxel=False, multiple=1).norm_voxel is False
    assert SequenceAssembler(1, 3, "sharp").multiple == 8                      # the pair layouts keep their default


def test_tile_origins_on_a_4d_geometry_equal_the_oracle():
    from oracle import refid_oracle as O
    from refid_amd.tiling import grid_indices
    for h, w, c in [(40, 56, 24), (28, 40, 24), (1224, 1632, 512), (720, 1280, 256), (24, 24, 24)]:
        got, ch, cw = grid_indices(h, w, c)
        assert got == O.tile_grid(h, w, c) and (ch, cw) == (c, c), (h, w, c)
    idx, _, _ = grid_indices(40, 56, 24)
    assert len(idx) == 2 * 3 and idx[0] == dict(i=0, j=0) and idx[-1] == dict(i=16, j=32)
    cover = np.zeros((40, 56), int)
    for d in idx:
        cover[d["i"]:d["i"] + 24, d["j"]:d["j"] + 24] += 1
    assert set(np.unique(cover)) == {1, 2, 4}                                   # dividing by a power of two is exact


@pytest.mark.parametrize("key,value", [("trans_num", 8), ("random_crop_num", 2)])
def test_unsupported_grid_options_name_the_key(key, value):
    from refid_amd import train as T
    from refid_amd._lib import RefidHipError
    for cls in (T.ImageEventRestorationModel, T.TestImageEventRestorationModel):
        m = cls.__new__(cls)
        m.opt = {"val": {"grids": True, "crop_size": 24, key: value}}
        with pytest.raises(RefidHipError, match=rf"val\.{key} = {value}"):
            m._val_forward()
