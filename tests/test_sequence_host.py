"""CPU-only: the host side of the test-time entry -- window search (refid_amd.sequence.pair_windows / make_pairs), the
numpy restatement of the pair assembly against the reference-generated fixtures, read_png on all five filter types,
create_model's name resolution and the sharp models' bookkeeping."""
import os
import random
import struct
import zlib

import numpy as np
import pytest

import sample_assembly_ref as R
import sequence_ref as S


# ---- pair_windows ---------------------------------------------------------------------------------------------------
def test_windows_are_half_open_with_repeated_stamps_on_the_bounds():
    from refid_amd.sequence import make_pairs, pair_windows
    t = np.array([1, 2, 2, 2, 3, 5, 5, 8], dtype=np.float32)
    rows = pair_windows(t, [1, 2, 5, 0], [2, 5, 8, 1])
    # an event exactly at ends[k] belongs to the next window: the three 2s open window 1, both 5s open window 2
    assert rows.dtype == np.int64 and rows.tolist() == [[0, 1], [1, 5], [5, 7], [0, 0]]
    pairs = make_pairs(t, [0, 1, 2, 3], [1, 2, 3, 4], [1, 2, 5, 0], [2, 5, 8, 1])
    assert [tuple(p) for p in pairs] == [(0, 1, 0, 1, 1.0, 1.0), (1, 2, 1, 5, 2.0, 3.0), (2, 3, 5, 7, 5.0, 5.0),
                                         (3, 4, 0, 0, 0.0, 0.0)]                 # the empty window: stamps (0, 0)
    bounds = make_pairs(t, [0], [1], [2], [5], stamps="bounds")
    assert tuple(bounds[0]) == (0, 1, 1, 5, 2.0, 5.0)


def test_empty_windows_windows_past_the_end_and_an_empty_stream():
    from refid_amd.sequence import pair_windows
    t = np.array([1, 2, 3], dtype=np.float32)
    assert pair_windows(t, [2.5, 3.5, 10, 2], [2.75, 9, 20, 1]).tolist() == [[2, 2], [3, 3], [3, 3], [1, 1]]
    assert pair_windows(t, [0], [100]).tolist() == [[0, 3]]
    assert pair_windows(np.zeros(0, np.float32), [0, 1], [1, 2]).tolist() == [[0, 0], [0, 0]]
    # bounds are compared as float32, the type of the column: 16777217 rounds to 16777216 and 16777218.5 to 16777218
    # (compared as float64 the window would be rows [1, 2))
    big = np.array([16777216, 16777218], dtype=np.float32)
    assert pair_windows(big, [16777217], [16777218.5]).tolist() == [[0, 1]]


def test_an_unsorted_stream_raises():
    from refid_amd._lib import RefidHipError
    from refid_amd.sequence import make_pairs, pair_windows
    with pytest.raises(RefidHipError, match="non-decreasing"):
        pair_windows(np.array([1, 3, 2], dtype=np.float32), [0], [4])
    with pytest.raises(RefidHipError, match="stamps"):
        make_pairs(np.array([1, 2], dtype=np.float32), [0], [1], [0], [4], stamps="frames")


def test_sharp_and_exposure_windows_index_pairs():
    from refid_amd.sequence import exposure_windows, sharp_windows
    l, r, b, e = sharp_windows([10, 20, 35, 40])
    assert (l.tolist(), r.tolist(), b.tolist(), e.tolist()) == ([0, 1, 2], [1, 2, 3], [10, 20, 35], [20, 35, 40])
    l, r, b, e = exposure_windows([10, 20, 30], [14, 24, 34])
    assert (l.tolist(), r.tolist(), b.tolist(), e.tolist()) == ([0, 1], [1, 2], [10, 20], [24, 34])   # windows overlap
    assert [len(v) for v in sharp_windows([7])] == [0, 0, 0, 0]


# ---- the restatement against the reference-generated fixtures ------------------------------------------------------------
@pytest.mark.parametrize("name", ["sample_sharp_n7", "sample_whole_frame"])
def test_one_pair_sequence_equals_the_sample_restatement(golden_dir, name):
    """The fixture's frames and events as a one-pair sequence (left = frame 0, right = frame 1, all rows,
    stamps='events'): bit-equal to assemble_sample of the same raw sample without augmentation; and where the fixture
    itself is whole-frame and its draw has no flip, bit-equal to what the reference's dataset code produced."""
    from refid_amd.data import draw_augmentation
    from refid_amd.sequence import make_pairs
    z, cfg = R.load_fixture(golden_dir, name)
    frames, ev = z["frames"], z["events"]
    m, n, layout = cfg["m"], cfg["n"], cfg["layout"]
    H, W = frames.shape[1:3]
    assert H % 8 == 0 and W % 8 == 0
    pairs = make_pairs(ev[:, 0], [0], [1], [ev[0, 0]], [np.nextafter(ev[-1, 0], np.float32(np.inf))])
    assert tuple(pairs[0]) == (0, 1, 0, len(ev), float(ev[0, 0]), float(ev[-1, 0]))
    lq, voxel = S.assemble_pairs(frames, ev, pairs, m, n, layout, multiple=8, bgr=True)
    want_lq, want_voxel, _ = R.assemble_sample(dict(frames=frames, events=ev), m, n, layout, None)
    assert np.array_equal(lq[0].view(np.uint32), want_lq.view(np.uint32))
    assert np.array_equal(voxel[0].view(np.uint32), want_voxel.view(np.uint32))
    assert np.abs(voxel).max() > 10                                               # the hot pixel is there
    checked = 0
    for seed in cfg["seeds"]:
        aug = draw_augmentation(random.Random(seed), H, W, cfg["gt_size"], cfg["use_hflip"], cfg["use_rot"])
        if cfg["gt_size"] is None and not any(aug[2:]):
            # float32 sums in the reference's order differ from the fixed-point sums in the last bits only
            np.testing.assert_allclose(voxel[0], z[f"s{seed}/voxel"], rtol=0, atol=1e-4)
            np.testing.assert_array_equal(R.image_channels(lq[0], m, layout), R.image_channels(z[f"s{seed}/lq"], m, layout))
            checked += 1
    print(name, "compared with the stored reference output for", checked, "seeds")


def test_padding_is_edge_for_images_and_zero_for_voxels(golden_dir):
    z, cfg = R.load_fixture(golden_dir, "sample_whole_frame")
    frames, ev = z["frames"][:, :21, :27], z["events"]
    m, n = cfg["m"], cfg["n"]
    pair = (0, 1, 0, len(ev), float(ev[0, 0]), float(ev[-1, 0]))
    lq, voxel = S.assemble_pairs(frames, ev, [pair], m, n, "blur", multiple=8, bgr=True)
    assert lq.shape == (1, 6 + 2 * (m - 1), 24, 32) and voxel.shape == (1, 2 * m + n, 2, 24, 32)
    assert np.all(voxel[0, :, :, 21:] == 0) and np.all(voxel[0, :, :, :, 27:] == 0)
    img, vox = R.image_channels(lq[0], m, "blur"), R.voxel_channels(lq[0], m, "blur")
    assert np.all(vox[:, 21:] == 0) and np.all(vox[:, :, 27:] == 0) and np.abs(vox).max() > 0
    assert np.all(img[:, 21:, :] == img[:, 20:21, :]) and np.all(img[:, :, 27:] == img[:, :, 26:27])
    assert img[0, 3, 5] == np.float32(frames[0, 3, 5, 2]) / np.float32(255)        # BGR input: R comes from channel 2


# ---- read_png on every filter type ---------------------------------------------------------------------------------------
def _filter_rows(img, types):
    """PNG-filters the rows of a uint8 (H, W, C) image by hand with the given per-row filter types."""
    h = img.shape[0]
    bpp = img.shape[2] if img.ndim == 3 else 1
    raw = img.reshape(h, -1).astype(np.int32)
    out = bytearray()
    for y in range(h):
        cur = raw[y]
        up = raw[y - 1] if y else np.zeros_like(cur)
        a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]])
        c = np.concatenate([np.zeros(bpp, np.int32), up[:-bpp]])
        ft = types[y]
        if ft == 0:
            pred = np.zeros_like(cur)
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = up
        elif ft == 3:
            pred = (a + up) // 2
        else:
            pa, pb, pc = np.abs(up - c), np.abs(a - c), np.abs(a + up - 2 * c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
        out += bytes([ft]) + ((cur - pred) & 0xff).astype(np.uint8).tobytes()
    return bytes(out)


def _png_bytes(img, types):
    from refid_amd.png import SIGNATURE, _chunk
    h, w = img.shape[:2]
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2 if img.ndim == 3 else 0, 0, 0, 0)
    data = zlib.compress(_filter_rows(img, types), 6)
    half = len(data) // 2                                                      # two IDAT chunks: they are concatenated
    return SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", data[:half]) + _chunk(b"IDAT", data[half:]) + _chunk(b"IEND", b"")


@pytest.mark.parametrize("shape", [(13, 17, 3), (9, 11)], ids=["rgb", "grey"])
@pytest.mark.parametrize("ft", [0, 1, 2, 3, 4, "mixed"])
def test_read_png_decodes_every_filter_type(tmp_path, shape, ft):
    from refid_amd.png import read_png
    rng = np.random.Generator(np.random.PCG64(5))
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    img[2:5] = 255                                                             # wrap-around in Sub / Average / Paeth sums
    img[5] = 0
    types = [(y % 5) if ft == "mixed" else ft for y in range(shape[0])]
    path = tmp_path / "f.png"
    path.write_bytes(_png_bytes(img, types))
    got = read_png(str(path))
    assert got.dtype == np.uint8 and got.shape == shape and np.array_equal(got, img)


def test_read_png_round_trips_write_png_and_rejects_a_bad_filter(tmp_path):
    from refid_amd.png import SIGNATURE, _chunk, read_png, write_png
    rng = np.random.Generator(np.random.PCG64(6))
    for shape in ((37, 50, 3), (4, 6)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        assert np.array_equal(read_png(write_png(str(tmp_path / "w.png"), img)), img)
    bad = tmp_path / "bad.png"
    raw = bytearray(_filter_rows(np.zeros((2, 2, 3), np.uint8), [0, 0]))
    raw[7] = 5                                                                 # row 1's filter byte
    ihdr = struct.pack(">IIBBBBB", 2, 2, 8, 2, 0, 0, 0)
    bad.write_bytes(SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(bytes(raw))) + _chunk(b"IEND", b""))
    with pytest.raises(ValueError, match="filter type 5"):
        read_png(str(bad))


def test_load_event_npz_concatenates_float32_rows(tmp_path):
    from refid_amd.sequence import load_event_npz
    a = dict(x=np.array([1, 2], np.uint16), y=np.array([3, 4], np.uint16), timestamp=np.array([10, 11], np.int64),
             polarity=np.array([1, 0], np.uint8))
    b = dict(x=np.array([5], np.uint16), y=np.array([6], np.uint16), timestamp=np.array([16777217], np.int64),
             polarity=np.array([1], np.uint8))
    np.savez(tmp_path / "a.npz", **a)
    np.savez(tmp_path / "b.npz", **b)
    ev = load_event_npz([tmp_path / "a.npz", tmp_path / "b.npz"])
    assert ev.dtype == np.float32 and ev.tolist() == [[10, 1, 3, 1], [11, 2, 4, 0], [16777216, 5, 6, 1]]   # float32 stamps
    sw = load_event_npz(str(tmp_path / "a.npz"), swap_xy=True)
    assert sw.tolist() == [[10, 3, 1, 1], [11, 4, 2, 0]]
    assert load_event_npz([]).shape == (0, 4)


# ---- the command-line front: everything before the GPU -------------------------------------------------------------------
TEST_YAML = """
name: tiny-7skip
model_type: TestTwoSharpImageEventRecurrentRestorationModel
num_gpu: 1
datasets:
  test:
    name: gopro-test
    type: NpyPngSharpSingleDeblurDataset
    num_end_interpolation: 1
    num_inter_interpolation: 7
network_g:
  type: FinalBidirectionAttenfusion
  img_chn: 6
  ev_chn: 2
  num_encoders: 3
  base_num_channels: 8
  num_block: 1
path:
  pretrain_network_g: ~
"""


def test_interpolate_settings_and_frame_loading(tmp_path):
    import argparse
    from refid_amd import interpolate as I
    from refid_amd.png import write_png
    yml = tmp_path / "t.yml"
    yml.write_text(TEST_YAML)
    ns = lambda **kw: argparse.Namespace(**dict(dict(opt=None, checkpoint=None, m=None, n=None, layout=None), **kw))  # noqa: E731
    net, ckpt, m, n, layout = I.settings(ns(opt=str(yml)))
    assert (ckpt, m, n, layout) == (None, 1, 7, "sharp") and net["base_num_channels"] == 8 and net["type"] == "FinalBidirectionAttenfusion"
    net, ckpt, m, n, layout = I.settings(ns(opt=str(yml), checkpoint="w.pth", n=3))
    assert (ckpt, m, n, layout) == ("w.pth", 1, 3, "sharp")
    net, ckpt, m, n, layout = I.settings(ns(checkpoint="w.pth", n=1, m=3, layout="blur"))
    assert (m, n, layout) == (3, 1, "blur") and net == dict(I.RELEASED_NETWORK, img_chn=10)
    with pytest.raises(SystemExit, match="--n"):
        I.settings(ns(checkpoint="w.pth"))
    rng = np.random.Generator(np.random.PCG64(8))
    stack = rng.integers(0, 256, (3, 5, 7, 3), dtype=np.uint8)
    for k in (2, 0, 1):
        write_png(str(tmp_path / "fr" / f"{k:04d}.png"), stack[k])
    assert np.array_equal(I.load_frames(str(tmp_path / "fr")), stack)             # sorted by name
    np.save(tmp_path / "s.npy", stack)
    assert np.array_equal(I.load_frames(str(tmp_path / "s.npy")), stack)
    np.save(tmp_path / "f.npy", stack.astype(np.float32))
    with pytest.raises(SystemExit, match="uint8"):
        I.load_frames(str(tmp_path / "f.npy"))


# ---- create_model's name resolution ------------------------------------------------------------------------------------
def test_model_class_resolves_the_six_names():
    from refid_amd import train as T
    want = {"TwoImageEventRecurrentRestorationModel": (T.TwoImageEventRecurrentRestorationModel, "val", False),
            "ImageEventRestorationModel": (T.ImageEventRestorationModel, "val", False),
            "TwoSharpImageEventRecurrentRestorationModel": (T.TwoSharpImageEventRecurrentRestorationModel, "val", False),
            "TestTwoImageEventRecurrentRestorationModel": (T.TestTwoImageEventRecurrentRestorationModel, "test", True),
            "Test_TwoSharpImageEventRecurrentRestorationModel": (T.Test_TwoSharpImageEventRecurrentRestorationModel, "test", True),
            "TestTwoSharpImageEventRecurrentRestorationModel": (T.Test_TwoSharpImageEventRecurrentRestorationModel, "test", True)}
    for name, (cls, dataset, test_only) in want.items():
        got = T.model_class(name)
        assert got is cls and got.VAL_DATASET == dataset and got.TEST_ONLY is test_only, name
    for sharp in ("TwoSharpImageEventRecurrentRestorationModel", "Test_TwoSharpImageEventRecurrentRestorationModel"):
        assert issubclass(T.model_class(sharp), T.TwoSharpImageEventRecurrentRestorationModel)
    assert not issubclass(T.TestTwoImageEventRecurrentRestorationModel, T.TwoSharpImageEventRecurrentRestorationModel)
    for bad in ("TwoImageEventRecurrentRestorationModels", "", "BaseModel"):
        with pytest.raises(ValueError) as ei:
            T.model_class(bad)
        assert str(ei.value) == f"Model {bad} is not found."
    with pytest.raises(ValueError) as ei:
        T.create_model({"model_type": "VideoModel"})
    assert str(ei.value) == "Model VideoModel is not found."


# ---- the sharp bookkeeping against a hand-computed example -------------------------------------------------------------
def test_sharp_bookkeeping_by_hand():
    from refid_amd.metrics import InterpolationMetrics
    opts = dict(psnr=dict(type="calculate_psnr", crop_border=0, test_y_channel=False),
                ssim=dict(type="calculate_ssim", crop_border=0, test_y_channel=False))
    book = InterpolationMetrics(opts)
    assert book.with_metrics and book.metric_types() == {"calculate_psnr", "calculate_ssim"}
    book.add_item({"calculate_psnr": [30.0, 31.0, 32.5], "calculate_ssim": [0.5, 0.25, 0.75]})
    book.add_item({"calculate_psnr": [20.0, 40.0, 27.0], "calculate_ssim": [0.125, 1.0, 0.375]})
    ret = book.finish()
    # 2 items x T = 3 frames: every frame is an interpolation frame, the divisor is cnt * T = 6
    assert book.cnt == 2 and book.frames == 3
    assert book.interpo == {"psnr": 180.5 / 6, "ssim": 3.0 / 6}
    assert ret == 0.5                                                          # the last interpolation metric
    assert book.log_lines("GoPro-7skip") == ["Validation GoPro-7skip [interpolation],\t\t # psnr: 30.0833\t # ssim: 0.5000"]
    assert not hasattr(book, "deblur") and not hasattr(book, "total")
    none = InterpolationMetrics(None)
    none.add_item({})
    assert none.finish() == 0. and not none.with_metrics and none.metric_types() == set()
