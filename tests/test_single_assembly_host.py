"""CPU-only: the single-image event deblurring path -- refid_assemble_single / refid_voxel_norm (csrc/sample.hip) through
their numpy restatement (tests/single_assembly_ref.py) against the reference's own __getitem__ (fixtures
tests/golden/single_*.npz, tools/make_single_golden.py), and the host-side layers above the kernels.

Stage 1, assembly: the pre-norm voxel under the bounds of test_sample_assembly_host.py ((cnt+1)*mass*2^-24 against the
reference's sequential fp32 sum, cnt*2^-32 + ulp/2 against float64); lq and gt bit for bit.

Stage 2, normalisation: the restated voxel_norm applied to THE REFERENCE's pre-norm voxel against the reference's
normalised voxel, per element within (1 + d_ref) * B, where d_ref is the reference's own distance from the float64
normalisation of that voxel in units of B, recorded by the generator; the restatement itself lies within 1 * B of
float64.  B (single_assembly_ref.bound, derived in test_hip_voxel_norm.py), with mu, sigma the float64 mean and standard
deviation of the non-zero v, u = 2^-24, D = 25 + chunks the depth of the float64 summation:
    B(v) = (3|v-mu| + |mu|) u/sigma (1 + 4u) + |v-mu|/sigma eps_sigma + (D+2) 2^-53 sqrt(sigma^2+mu^2)/sigma + 2^-149,
    eps_sigma = (2D+8) 2^-53 (1 + (mu/sigma)^2)."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import single_assembly_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUG = ("top", "left", "hflip", "vflip", "rot90")


def _cases(golden_dir):
    from refid_amd.data import draw_augmentation
    for name in S.FIXTURES:
        z, cfg = S.load_fixture(golden_dir, name)
        H, W = z["frames"].shape[1:3]
        for seed in cfg["seeds"]:
            aug = draw_augmentation(random.Random(seed), H, W, cfg["gt_size"], cfg["use_hflip"], cfg["use_rot"])
            yield name, z, cfg, seed, aug


def test_fixture_set_covers_the_cases(golden_dir):
    combos, corner, bins = set(), False, set()
    for name, z, cfg, seed, (top, left, hf, vf, rt) in _cases(golden_dir):
        H, W = z["frames"].shape[1:3]
        combos.add((hf, vf, rt))
        bins.add(cfg["bins"])
        corner = corner or (top in (0, H - cfg["gt_size"]) and left in (0, W - cfg["gt_size"]))
        assert z["frames"].shape[0] == 2 and z[f"s{seed}/voxel"].shape == (cfg["bins"], cfg["gt_size"], cfg["gt_size"])
    assert len(combos) == 8 and corner and bins == {6, 2}


def test_stage1_assembly_matches_the_reference(golden_dir):
    for name, z, cfg, seed, aug in _cases(golden_dir):
        what = f"{name} seed {seed} aug {aug}"
        sample = dict(frames=z["frames"], events=z["events"], **dict(zip(AUG, aug)))
        lq, voxel, gt, pre = S.assemble_sample(sample, cfg["bins"], cfg["gt_size"])
        assert np.array_equal(lq.view(np.uint32), z[f"s{seed}/lq"].view(np.uint32)), what
        assert np.array_equal(gt.view(np.uint32), z[f"s{seed}/gt"].view(np.uint32)), what
        H, W = z["frames"].shape[1:3]
        g = cfg["gt_size"]
        e, cnt, mass = S.float64_sums(z["events"], cfg["bins"], H, W, aug[0], aug[1], g, g, *aug[2:])
        assert cnt.max() >= 50, (what, "a hot pixel must be inside the crop")
        S.check_voxel(pre, z[f"s{seed}/pre"], e, cnt, mass, what)
        assert np.array_equal(pre != 0, z[f"s{seed}/pre"] != 0), what          # the same mask: the same S0


def test_stage2_normalisation_matches_the_reference(golden_dir):
    for name, z, cfg, seed, aug in _cases(golden_dir):
        what = f"{name} seed {seed}"
        ref_pre, ref_out, d_ref = z[f"s{seed}/pre"], z[f"s{seed}/voxel"], float(z[f"s{seed}/d_ref"])
        out = S.normalise(ref_pre)
        x64, mu, sigma = S.float64_norm(ref_pre)
        b = S.bound(ref_pre, mu, sigma, ref_pre.size)
        nz = ref_pre != 0
        assert np.all(out[~nz] == 0) and np.all(ref_out[~nz] == 0), what
        d64 = np.abs(out.astype(np.float64) - x64)
        assert np.all(d64[nz] <= b[nz]), (what, "vs float64", float((d64[nz] / b[nz]).max()))
        d = np.abs(out.astype(np.float64) - ref_out.astype(np.float64))
        assert np.all(d[nz] <= (1 + d_ref) * b[nz]), (what, float((d[nz] / b[nz]).max()), d_ref)


def test_fused_and_standalone_statistics_agree(golden_dir):
    """On event data (multiples of 2^-32, sums far below 2^21) the float64 tree sum of v is exact, so the int64 S1 of the
    fused route and the float64 S1 of the stand-alone route are the same number."""
    for name, z, cfg, seed, aug in _cases(golden_dir):
        sample = dict(frames=z["frames"], events=z["events"], **dict(zip(AUG, aug)))
        lq, voxel, gt, pre = S.assemble_sample(sample, cfg["bins"], cfg["gt_size"])
        assert S.stats(pre) == S.stats(pre, acc=True)
        assert np.array_equal(S.normalise(pre).view(np.uint32), voxel.view(np.uint32))


def _events(rows):
    return np.array(rows, dtype=np.float32).reshape(-1, 4)


def test_degenerate_samples():
    frames = np.zeros((2, 8, 8, 3), dtype=np.uint8)
    # no events: zeros
    lq, voxel, gt, pre = S.assemble_sample(dict(frames=frames, events=_events([])), 6, None)
    assert voxel.shape == (6, 8, 8) and not voxel.any()
    # one event: its two bins hold different values, so that is a sample WITH spread; one event at the first stamp fills one
    # element only -- no spread: zeros here, where the reference divides 0 by 0 and returns an all-NaN voxel
    lq, voxel, gt, pre = S.assemble_sample(dict(frames=frames, events=_events([[0.0, 3, 2, 1]])), 6, None)
    assert np.count_nonzero(pre) == 1 and pre[0, 2, 3] == 1.0
    assert not voxel.any() and not np.isnan(voxel).any(), "deliberate departure: the reference gives NaN here"
    import torch
    t = torch.from_numpy(pre)
    ref = (t != 0).float() * (t - t.sum() / 1) / torch.sqrt((t ** 2).sum() / 1 - (t.sum() / 1) ** 2)      # event_util.py:155-158
    assert torch.isnan(ref).all()
    # +1 and -1 at the same pixel and time: that element is masked out and not counted in S0
    ev = _events([[0.0, 1, 1, 1], [0.5, 3, 2, 1], [0.5, 3, 2, 0], [0.5, 5, 5, 1], [1.0, 6, 6, 0]])
    lq, voxel, gt, pre = S.assemble_sample(dict(frames=frames, events=ev), 2, None)
    assert pre[0, 2, 3] == 0 and pre[1, 2, 3] == 0 and voxel[0, 2, 3] == 0 and voxel[1, 2, 3] == 0
    s0, s1, s2 = S.stats(pre)
    assert s0 == np.count_nonzero(pre) == 4                                  # (1,1)@bin0, (5,5)@bins 0 and 1, (6,6)@bin1
    x64, mu, sigma = S.float64_norm(pre)
    nz = pre != 0
    assert np.all(np.abs(voxel.astype(np.float64) - x64)[nz] <= S.bound(pre, mu, sigma, pre.size)[nz])


def test_tree_sum_is_the_documented_order():
    """One chunk and a bit: thread t adds k*256 + t in sequence, lanes pairwise, waves and chunks in order."""
    rng = np.random.Generator(np.random.PCG64(3))
    x = rng.standard_normal(S.CHUNK + 700) * 10.0 ** rng.integers(-8, 8, S.CHUNK + 700)
    total = np.float64(0)
    for c0 in (0, S.CHUNK):
        chunk = np.zeros(S.CHUNK)
        chunk[:len(x[c0:c0 + S.CHUNK])] = x[c0:c0 + S.CHUNK]
        lanes = []
        for t in range(256):
            s = np.float64(0)
            for k in range(16):
                s = s + chunk[k * 256 + t]
            lanes.append(s)
        waves = []
        for w in range(4):
            v = lanes[w * 64:(w + 1) * 64]
            o = 1
            while o < 64:
                v = [v[i] + v[i ^ o] for i in range(64)]
                o *= 2
            assert len(set(v)) == 1                                           # every lane ends with the same bits
            waves.append(v[0])
        total = total + (((waves[0] + waves[1]) + waves[2]) + waves[3])
    assert S._tree_sum(x) == total


def test_single_image_metrics_by_hand():
    from refid_amd.metrics import SingleImageMetrics, check_metric_options
    from refid_amd._lib import RefidHipError
    opts = dict(psnr=dict(type="calculate_psnr", crop_border=0, test_y_channel=False),
                ssim=dict(type="calculate_ssim", crop_border=0, test_y_channel=False))
    book = SingleImageMetrics(opts)
    assert book.with_metrics and book.metric_types() == {"calculate_psnr", "calculate_ssim"}
    for p, s in ((30.0, 0.9), (32.0, 0.8), (25.0, 0.4)):
        book.add_item({"calculate_psnr": [p], "calculate_ssim": [s]})
    assert book.finish() == (0.9 + 0.8 + 0.4) / 3                              # the last metric in dict order
    assert book.results == {"psnr": (30.0 + 32.0 + 25.0) / 3, "ssim": (0.9 + 0.8 + 0.4) / 3}
    assert book.log_lines("GoPro") == ["Validation GoPro,\t\t # psnr: 29.0000\t # ssim: 0.7000"]
    none = SingleImageMetrics(None)
    none.add_item({})
    assert not none.with_metrics and none.finish() == 0. and none.metric_types() == set()
    empty = SingleImageMetrics({})
    empty.add_item({})
    assert empty.finish() == 0.
    check_metric_options({"metrics": opts}, True, groups=("metrics",))
    with pytest.raises(RefidHipError, match=r"val\.metrics\.psnr\.crop_border"):
        check_metric_options({"metrics": dict(psnr=dict(type="calculate_psnr", crop_border=2))}, True, groups=("metrics",))


def test_model_class_resolves_the_single_image_test_model():
    from refid_amd import train as T
    cls = T.model_class("TestImageEventRestorationModel")
    assert cls is T.TestImageEventRestorationModel and issubclass(cls, T.ImageEventRestorationModel)
    assert cls.TEST_ONLY is True and cls.VAL_DATASET == "test" and cls.__test__ is False
    assert T.ImageEventRestorationModel.nondist_validation is T.TwoImageEventRecurrentRestorationModel.nondist_validation


def test_single_model_file_names():
    """image_event_restoration_model.py:428-450 without a GPU: the naming hook of the loop."""
    from refid_amd import train as T
    m = T.ImageEventRestorationModel.__new__(T.ImageEventRestorationModel)
    data = {"seq": ["a", "b"], "origin_index": ["000007", "000031"]}
    m.opt = {"is_train": False, "path": {"visualization": "/v"}}
    assert m._val_stems(data, 2, 1, "GoPro", 500, 3) == ["/v/GoPro/a/000007", "/v/GoPro/b/000031"]
    m.opt = {"is_train": True, "path": {"visualization": "/v"}}
    assert m._val_stems(data, 2, 1, "GoPro", 500, 0) == [None, "/v/000031/000031_500"]      # cnt == 1 only
    assert m._val_stems(data, 2, 1, "GoPro", 500, 1) == ["/v/000007/000007_500", None]
    assert m._val_stems(data, 2, 1, "GoPro", 500, 2) == [None, None]


def _header_fields(struct_name):
    src = open(os.path.join(ROOT, "include", "refid_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct_name, struct_name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            names = re.sub(r"^(const\s+)?(unsigned char|long long|float|int|void|refid_sample_desc)\s*\*?", "", stmt)
            out += [n.strip().lstrip("*").strip() for n in names.split(",")]
    return out


def test_header_and_ctypes_mirror_agree():
    from refid_amd import _lib, ops
    from refid_amd.build import build
    assert _header_fields("refid_single_desc") == [f[0] for f in _lib.SingleDesc._fields_]
    assert ctypes.sizeof(_lib.SingleDesc) == 80 and _lib.SingleDesc.scratch.offset == 40
    assert ctypes.sizeof(_lib.SampleDesc) == 80 and ctypes.sizeof(_lib.AssembleDesc) == 72    # unchanged
    src = open(os.path.join(ROOT, "include", "refid_hip.h")).read()
    assert int(re.search(r"#define REFID_ASSEMBLE_STATS (\d+)", src).group(1)) == _lib.ASSEMBLE_STATS == ops.ASSEMBLE_STATS == 16
    assert _lib.ASSEMBLE_STATS & _lib.ASSEMBLE_ALL == 0
    lib = ctypes.CDLL(build())
    for sym in ("refid_voxel_norm", "refid_voxel_norm_parts", "refid_assemble_single", "refid_single_bins"):
        assert hasattr(lib, sym), sym
    lib.refid_abi_version.restype = ctypes.c_int
    assert lib.refid_abi_version() == 9 == _lib.ABI_VERSION                   # purely additive
    lib.refid_voxel_norm_parts.restype = ctypes.c_longlong
    lib.refid_voxel_norm_parts.argtypes = [ctypes.c_int, ctypes.c_longlong]
    assert lib.refid_voxel_norm_parts(1, 4096) == 3 and lib.refid_voxel_norm_parts(5, 4097) == 30
    assert lib.refid_voxel_norm_parts(0, 10) == 0


def test_option_mapping_and_rejections_without_a_gpu():
    from refid_amd._lib import RefidHipError
    from refid_amd.build import build
    from refid_amd.data import DeviceBatchAssembler, draw_augmentation
    from refid_amd.options import assembler_from_dataset_opt
    build()
    ds = dict(type="GoProSingleImageEventDataset", num_bins=6, gt_size=256, use_hflip=True, use_rot=True, norm_voxel=False)
    assert assembler_from_dataset_opt(ds) is None
    a = assembler_from_dataset_opt(dict(ds, device_assemble=True))
    assert (a.layout, a.bins, a.gt_size, a.use_hflip, a.use_rot) == ("single", 6, 256, True, True)
    assert a.norm_voxel is True, "the reference normalises unconditionally (Single_image_npy_dataset.py:187)"
    drawn = draw_augmentation(random.Random(3), 720, 1280, 256, True, True)
    assert a.draw(random.Random(3), 720, 1280) == dict(zip(AUG, drawn))
    assert assembler_from_dataset_opt(dict(ds, num_bins=2, device_assemble=True)).bins == 2
    with pytest.raises(RefidHipError, match="img2tensor"):
        assembler_from_dataset_opt(dict(ds, num_bins=3, device_assemble=True))
    with pytest.raises(RefidHipError, match="img2tensor"):
        DeviceBatchAssembler(layout="single", num_bins=3)
    with pytest.raises(RefidHipError, match="num_bins >= 1"):
        DeviceBatchAssembler(layout="single", num_bins=0)
    with pytest.raises(RefidHipError, match="unknown layout"):
        DeviceBatchAssembler(1, 1, layout="double")
    with pytest.raises(RefidHipError, match="num_bins"):
        assembler_from_dataset_opt(dict(type="GoProSingleImageEventDataset", device_assemble=True))
    assert DeviceBatchAssembler(layout="single", num_bins=6, norm_voxel=False).norm_voxel is False
