"""CPU-only: batch assembly from raw frames and events (refid_amd.data.DeviceBatchAssembler, csrc/sample.hip) against the
reference's own __getitem__ (fixtures tests/golden/sample_*.npz, tools/make_sample_golden.py), through the numpy
restatement of the device algorithm in tests/sample_assembly_ref.py.

Bounds.  The reference sums fp32-rounded per-event values sequentially in fp32 (np.add.at): for an element with `cnt`
contributions of total magnitude `mass` it is within (cnt+1)*mass*2^-24 of the exact sum, and no closer in general (on a
pixel-bin with thousands of events it is ~1e-4 away from the float64 sum, where the project's usual rtol 1e-5 / atol 2e-6
does not hold).  The fixed-point sum truncates each contribution by < 2^-32 and rounds once: |out - e| <= cnt*2^-32 +
ulp32(e)/2 against the float64 sum e of the reference's per-event values."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import sample_assembly_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases(golden_dir):
    from refid_amd.data import draw_augmentation
    for name in R.FIXTURES:
        z, cfg = R.load_fixture(golden_dir, name)
        H, W = z["frames"].shape[1:3]
        for seed in cfg["seeds"]:
            aug = draw_augmentation(random.Random(seed), H, W, cfg["gt_size"], cfg["use_hflip"], cfg["use_rot"])
            yield name, z, cfg, seed, aug


def _float64_sums(events, bins, H, W, top, left, ch, cw, hflip, vflip, rot90):
    """Per output element: float64 sum of the reference's per-event values (event_util.py:44-47), number of contributions
    and their total magnitude."""
    keep, ti, idx, q, sign = R.event_terms(events, events[0, 0], events[-1, 0], bins, H, W, top, left, ch, cw, hflip, vflip, rot90)
    dT = np.float32(events[-1, 0] - events[0, 0])
    ts = (np.float32(bins - 1) * (events[:, 0] - events[0, 0])) / (dT if dT != 0 else np.float32(1))
    dts = ts.astype(np.float64) - ti                                         # as numpy promotes float32 - int64
    e, cnt, mass = (np.zeros((bins, ch * cw), dtype=t) for t in (np.float64, np.int64, np.float64))
    for sel, b, v in ((keep, ti, sign * (1.0 - dts)), (keep & (ti + 1 < bins), ti + 1, sign * dts)):
        np.add.at(e, (b[sel], idx[sel]), v[sel])
        np.add.at(cnt, (b[sel], idx[sel]), 1)
        np.add.at(mass, (b[sel], idx[sel]), np.abs(v[sel]))
    return (a.reshape(bins, ch, cw) for a in (e, cnt, mass))


def _bins_of(voxel):
    """(bins-1, 2, h, w) sliding pairs -> (bins, h, w)."""
    return np.concatenate([voxel[:, 0], voxel[-1:, 1]], axis=0)


def _check_voxel(out, ref, e, cnt, mass, what):
    assert out.shape == ref.shape == e.shape
    assert np.all(out[cnt == 0] == 0) and np.all(ref[cnt == 0] == 0), what
    d = np.abs(out.astype(np.float64) - ref.astype(np.float64))
    bound = (cnt + 1) * mass * 2.0 ** -24
    assert np.all(d <= bound), (what, float((d - bound).max()), int(cnt.max()))
    d = np.abs(out.astype(np.float64) - e)
    bound = cnt * 2.0 ** -32 + 0.5 * np.spacing(np.abs(e).astype(np.float32)).astype(np.float64)
    assert np.all(d <= bound), (what, "vs float64", float((d - bound).max()))


def test_draw_augmentation_consumes_the_reference_draws():
    from refid_amd.data import draw_augmentation
    for k in range(20):
        for gt_size, hf, rot in ((16, True, True), (16, False, True), (16, True, False), (None, True, True), (16, False, False)):
            a, b = random.Random(k), random.Random(k)
            got = draw_augmentation(a, 40, 56, gt_size, hf, rot)
            top, left = (b.randint(0, 40 - 16), b.randint(0, 56 - 16)) if gt_size else (0, 0)     # transforms.py:212-213
            want = (top, left, hf and b.random() < 0.5, rot and b.random() < 0.5, rot and b.random() < 0.5)   # :110-112
            assert got == want
            assert a.random() == b.random()                                                        # same number of draws
    with pytest.raises(ValueError):
        draw_augmentation(random.Random(0), 8, 56, 16, True, True)


def test_fixture_set_covers_the_cases(golden_dir):
    combos, corner, hot = set(), False, []
    for name, z, cfg, seed, (top, left, hf, vf, rt) in _cases(golden_dir):
        combos.add((hf, vf, rt))
        H, W = z["frames"].shape[1:3]
        ch, cw = (H, W) if cfg["gt_size"] is None else (cfg["gt_size"],) * 2
        corner = corner or (cfg["gt_size"] is not None and top in (0, H - ch) and left in (0, W - cw))
        ev = z["events"]
        inside = (ev[:, 1] >= left) & (ev[:, 1] < left + cw) & (ev[:, 2] >= top) & (ev[:, 2] < top + ch)
        pix = (ev[inside, 2].astype(np.int64) * W + ev[inside, 1].astype(np.int64))
        hot.append(np.bincount(pix).max())
    assert len(combos) == 8 and corner
    assert min(hot) >= 2000, hot


def test_restatement_matches_the_reference_getitem(golden_dir):
    for name, z, cfg, seed, aug in _cases(golden_dir):
        m, n, layout = cfg["m"], cfg["n"], cfg["layout"]
        sample = dict(frames=z["frames"], events=z["events"], **dict(zip(("top", "left", "hflip", "vflip", "rot90"), aug)))
        lq, voxel, gt = R.assemble_sample(sample, m, n, layout, cfg["gt_size"])
        what = f"{name} seed {seed} aug {aug}"
        ref_lq, ref_voxel, ref_gt = z[f"s{seed}/lq"], z[f"s{seed}/voxel"], z[f"s{seed}/gt"]
        assert lq.shape == ref_lq.shape and voxel.shape == ref_voxel.shape and gt.shape == ref_gt.shape, what
        # image data: bit-identical
        assert np.array_equal(gt.view(np.uint32), ref_gt.view(np.uint32)), what
        assert np.array_equal(R.image_channels(lq, m, layout).view(np.uint32),
                              R.image_channels(ref_lq, m, layout).view(np.uint32)), what
        # voxel data: the reference's own rounding bound, and the fixed-point bound against float64
        H, W = z["frames"].shape[1:3]
        ch, cw = (H, W) if cfg["gt_size"] is None else (cfg["gt_size"],) * 2
        bins = R.num_bins(m, n, layout)
        e, cnt, mass = _float64_sums(z["events"], bins, H, W, aug[0], aug[1], ch, cw, *aug[2:])
        assert cnt.max() >= 100, (what, "the hot pixel must be inside the crop")
        _check_voxel(_bins_of(voxel), _bins_of(ref_voxel), e, cnt, mass, what)
        assert np.array_equal(voxel[1:, 0], voxel[:-1, 1]) and np.array_equal(ref_voxel[1:, 0], ref_voxel[:-1, 1])
        if layout == "blur":
            pick = list(range(1, m)) + list(range(m + 2 + n, bins))
            assert np.array_equal(R.voxel_channels(lq, m, layout), _bins_of(voxel)[pick]), what
            assert np.array_equal(R.voxel_channels(ref_lq, m, layout), _bins_of(ref_voxel)[pick]), what


def test_whole_frame_voxel_without_augmentation(golden_dir):
    for name in R.FIXTURES:
        z, cfg = R.load_fixture(golden_dir, name)
        ev = z["events"]
        H, W = z["frames"].shape[1:3]
        bins = R.num_bins(cfg["m"], cfg["n"], cfg["layout"])
        out = R.fixed_to_float(R.accumulate(ev, ev[0, 0], ev[-1, 0], bins, H, W, 0, 0, H, W, False, False, False))
        e, cnt, mass = _float64_sums(ev, bins, H, W, 0, 0, H, W, False, False, False)
        _check_voxel(out, z["voxel_full"], e, cnt, mass, name)


def test_fixed_point_mass_is_conserved(golden_dir):
    """Per pixel, the accumulators of all bins add up to 2^32 x the net polarity of the events that have both bins, exactly
    (the events in the last bin have no right neighbour: their left contributions are taken out first)."""
    for name, z, cfg, seed, aug in _cases(golden_dir):
        ev = z["events"]
        H, W = z["frames"].shape[1:3]
        ch, cw = (H, W) if cfg["gt_size"] is None else (cfg["gt_size"],) * 2
        bins = R.num_bins(cfg["m"], cfg["n"], cfg["layout"])
        args = (ev[0, 0], ev[-1, 0], bins, H, W, aug[0], aug[1], ch, cw) + tuple(aug[2:])
        acc = R.accumulate(ev, *args).reshape(bins, -1)
        keep, ti, idx, q, sign = R.event_terms(ev, *args)
        both = keep & (ti + 1 < bins)
        lone = keep & ~both
        assert lone.any() or cfg["gt_size"] is not None, "whole frame: the event at last_stamp has no right bin"
        net = np.zeros(ch * cw, dtype=np.int64)
        np.add.at(net, idx[both], sign[both])
        alone = np.zeros(ch * cw, dtype=np.int64)
        np.add.at(alone, idx[lone], (sign * (R.ONE - q))[lone])
        assert np.array_equal(acc.sum(axis=0) - alone, net * R.ONE), (name, seed)


def test_fixed_point_is_half_an_ulp_from_float64_where_fp32_summation_is_not():
    """5300 events on one pixel-bin: sequential fp32 summation (what np.add.at does) drifts; the fixed-point sum does not."""
    rng = np.random.Generator(np.random.PCG64(5))
    n = 5300
    t = np.sort(rng.uniform(0.30, 0.45, n)).astype(np.float32)
    ev = np.stack([t, np.full(n, 2, np.float32), np.full(n, 1, np.float32), np.ones(n, np.float32)], axis=1)
    ev = np.concatenate([np.array([[0, 0, 0, 1]], np.float32), ev, np.array([[1, 0, 0, 1]], np.float32)])
    out = R.fixed_to_float(R.accumulate(ev, 0.0, 1.0, 3, 4, 4, 0, 0, 4, 4, False, False, False))
    e, cnt, mass = _float64_sums(ev, 3, 4, 4, 0, 0, 4, 4, False, False, False)
    assert cnt[1, 1, 2] == n
    d = np.abs(out.astype(np.float64) - e)
    assert np.all(d <= cnt * 2.0 ** -32 + 0.5 * np.spacing(np.abs(e).astype(np.float32)))


def _header_fields(struct_name):
    src = open(os.path.join(ROOT, "include", "refid_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct_name, struct_name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            names = re.sub(r"^(const\s+)?(unsigned char|long long|float|int|refid_sample_desc)\s*\*?", "", stmt)
            out += [n.strip().lstrip("*").strip() for n in names.split(",")]
    return out


def test_header_exports_and_ctypes_mirror_agree():
    from refid_amd import _lib
    from refid_amd.build import build
    assert _header_fields("refid_sample_desc") == [f[0] for f in _lib.SampleDesc._fields_]
    assert _header_fields("refid_assemble_desc") == [f[0] for f in _lib.AssembleDesc._fields_]
    assert ctypes.sizeof(_lib.SampleDesc) == 80 and ctypes.sizeof(_lib.AssembleDesc) == 72
    assert _lib.SampleDesc.frames.offset == 32 and _lib.SampleDesc.rot90.offset == 76
    src = open(os.path.join(ROOT, "include", "refid_hip.h")).read()
    for name, val in (("REFID_LAYOUT_BLUR", _lib.LAYOUT_BLUR), ("REFID_LAYOUT_SHARP", _lib.LAYOUT_SHARP),
                      ("REFID_ASSEMBLE_ZERO", _lib.ASSEMBLE_ZERO), ("REFID_ASSEMBLE_SCATTER", _lib.ASSEMBLE_SCATTER),
                      ("REFID_ASSEMBLE_FINISH", _lib.ASSEMBLE_FINISH), ("REFID_ASSEMBLE_FRAMES", _lib.ASSEMBLE_FRAMES),
                      ("REFID_ASSEMBLE_ALL", _lib.ASSEMBLE_ALL)):
        assert int(re.search(r"#define %s (\d+)" % name, src).group(1)) == val
    lib = ctypes.CDLL(build())
    assert hasattr(lib, "refid_assemble_batch") and hasattr(lib, "refid_assemble_bins")
    lib.refid_abi_version.restype = ctypes.c_int
    assert lib.refid_abi_version() == 9 == _lib.ABI_VERSION


def test_layouts_and_rejections_without_a_gpu():
    from refid_amd import _lib, ops
    from refid_amd._lib import RefidHipError
    from refid_amd.build import build
    from refid_amd.data import DeviceBatchAssembler, draw_augmentation
    build()                                                             # (incremental; these are host-side queries of the library)
    from refid_amd.options import assembler_from_dataset_opt
    assert ops.assemble_bins(11, 1, _lib.LAYOUT_BLUR) == 24 and ops.assemble_bins(1, 7, _lib.LAYOUT_SHARP) == 8
    with pytest.raises(RefidHipError, match="img2tensor"):
        DeviceBatchAssembler(1, 2, layout="sharp")                      # 3 bins
    with pytest.raises(RefidHipError, match="img2tensor"):
        DeviceBatchAssembler(1, 0, layout="blur")
    with pytest.raises(RefidHipError):
        DeviceBatchAssembler(2, 7, layout="sharp")                      # image_sharp_npy_dataset.py:48
    ds = dict(type="GoProEventRecurrentDataset", num_end_interpolation=11, num_inter_interpolation=1, gt_size=256,
              use_hflip=True, use_rot=True, norm_voxel=True, one_voxel_flag=True, return_deblur_voxel=True)
    assert assembler_from_dataset_opt(ds) is None                       # key absent: nothing changes
    a = assembler_from_dataset_opt(dict(ds, device_assemble=True))
    assert (a.m, a.n, a.layout, a.bins, a.gt_size, a.use_hflip, a.use_rot) == (11, 1, "blur", 24, 256, True, True)
    drawn = draw_augmentation(random.Random(3), 720, 1280, 256, True, True)
    assert a.draw(random.Random(3), 720, 1280) == dict(zip(("top", "left", "hflip", "vflip", "rot90"), drawn))
    s = assembler_from_dataset_opt(dict(ds, type="GoProSharpEventRecurrentDataset", num_end_interpolation=1,
                                        num_inter_interpolation=7, return_deblur_voxel=False, device_assemble=True))
    assert (s.layout, s.bins) == ("sharp", 8)
    with pytest.raises(RefidHipError, match="one_voxel_flag"):
        assembler_from_dataset_opt(dict(ds, device_assemble=True, one_voxel_flag=False))
    with pytest.raises(RefidHipError, match="return_deblur_voxel"):
        assembler_from_dataset_opt(dict(ds, type="GoProSharpEventRecurrentDataset", num_end_interpolation=1,
                                        num_inter_interpolation=7, device_assemble=True))
