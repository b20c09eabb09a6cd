"""MI355X: the event simulator (csrc/event_sim.hip, refid_amd.event_sim) against tests/event_sim_ref.py, bit for bit on rows,
offsets and final state: every data family and shape of the list below, scalar thresholds and maps, BGR, stamps near 1e9,
a custom table, chunked against one call, E = 0, an unaligned view, run-to-run identity, the cap without and with
overflow (a bounded loop behind guard bands), the rows through ``SequenceAssembler`` and the command line with ``--split``."""
import ctypes
import functools
import glob
import os

import numpy as np
import pytest

import event_sim_ref as R

pytestmark = pytest.mark.gpu

C02 = 13107                  # 0.2 in units of 2^-16


def _noise(seed, n, h, w):
    return np.random.default_rng(seed).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)


def _grey(v):
    return np.repeat(np.asarray(v, dtype=np.uint8)[..., None], 3, axis=-1)


def _ramps(n, h, w):
    """A horizontal ramp that brightens over time in the upper half and darkens in the lower."""
    x = np.arange(w)[None, None, :] * (200.0 / max(w - 1, 1))
    k = np.arange(n)[:, None, None] * (250.0 / max(n - 1, 1))
    y = np.arange(h)[None, :, None]
    up = np.clip(x * 0.2 + k, 0, 255)
    down = np.clip(255 - x * 0.2 - k, 0, 255)
    return _grey(np.where(y < (h + 1) // 2, up, down))


def _flash(n, h, w):
    f = np.zeros((n, h, w, 3), dtype=np.uint8)
    f[1::2, h // 2, w // 2] = 255
    return f


def _checker(n, h, w):
    board = (np.arange(h)[:, None] + np.arange(w)[None, :]) % 2
    return _grey(np.stack([np.where(board == k % 2, 255, 0) for k in range(n)]))


def _maps(seed, h, w, lo=2000, hi=30000):
    rng = np.random.default_rng(seed)
    return rng.integers(lo, hi, size=(h, w)).astype(np.int32), rng.integers(lo, hi, size=(h, w)).astype(np.int32)


def _uniform(n, fps=240.0, t0=0.0):
    return t0 + np.arange(n, dtype=np.float64) / fps


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> dict(frames, stamps, lut, cp, cn, bgr); the restatement's answer is added once per case (``_want``)."""
    lut = R.default_lut()
    jitter = np.cumsum(np.random.default_rng(40).uniform(1e-4, 2e-2, size=9))
    out = {
        "noise_17x35_n9": dict(frames=_noise(0, 9, 17, 35), stamps=_uniform(9), cp=C02, cn=C02),
        "noise_1x1_n3": dict(frames=_noise(1, 3, 1, 1), stamps=_uniform(3), cp=3000, cn=3000),
        "noise_3x5_n2": dict(frames=_noise(2, 2, 3, 5), stamps=_uniform(2), cp=C02, cn=2 * C02),
        "noise_16x16_n3": dict(frames=_noise(3, 3, 16, 16), stamps=_uniform(3), cp=4000, cn=C02),
        "noise_9x57_n9_maps": dict(frames=_noise(4, 9, 9, 57), stamps=_uniform(9), cp=_maps(4, 9, 57)[0], cn=_maps(4, 9, 57)[1]),
        "noise_9x57_n3_pos_map_only": dict(frames=_noise(5, 3, 9, 57), stamps=_uniform(3), cp=_maps(5, 9, 57)[0], cn=9000),
        "noise_9x57_n3_bgr": dict(frames=_noise(6, 3, 9, 57), stamps=_uniform(3), cp=8000, cn=6000, bgr=True),
        "noise_17x35_n9_jitter": dict(frames=_noise(7, 9, 17, 35), stamps=jitter, cp=C02, cn=9000),
        "noise_3x5_n9_near_1e9": dict(frames=_noise(8, 9, 3, 5), stamps=_uniform(9, 240.0, 1e9), cp=5000, cn=5000),
        "noise_16x16_n3_near_1e9_slow": dict(frames=_noise(9, 3, 16, 16), stamps=1e9 + 300.0 * np.arange(3.0), cp=5000, cn=5000),
        "noise_17x35_n3_linear_table": dict(frames=_noise(10, 3, 17, 35), stamps=_uniform(3), cp=2500, cn=1001,
                                            lut=(1000 * np.arange(256) - 77).astype(np.int32)),
        "ramps_17x35_n9": dict(frames=_ramps(9, 17, 35), stamps=_uniform(9), cp=C02, cn=C02),
        "ramps_9x57_n3": dict(frames=_ramps(3, 9, 57), stamps=_uniform(3), cp=2000, cn=3000),
        "ramps_1x1_n9": dict(frames=_ramps(9, 1, 1), stamps=_uniform(9), cp=1776, cn=1776),
        "static_9x57_n3": dict(frames=np.repeat(_noise(11, 1, 9, 57), 3, axis=0), stamps=_uniform(3), cp=1776, cn=1776),
        "static_1x1_n2": dict(frames=np.repeat(_noise(12, 1, 1, 1), 2, axis=0), stamps=_uniform(2), cp=C02, cn=C02),
        "flash_3x5_n9_min_threshold": dict(frames=_flash(9, 3, 5), stamps=_uniform(9), cp=1776, cn=1776),
        "flash_16x16_n3_min_threshold": dict(frames=_flash(3, 16, 16), stamps=_uniform(3), cp=1776, cn=1776),
        "checker_16x16_n9": dict(frames=_checker(9, 16, 16), stamps=_uniform(9), cp=C02, cn=23000),
        "checker_9x57_n3_min_threshold": dict(frames=_checker(3, 9, 57), stamps=_uniform(3), cp=1776, cn=1776),
        "checker_3x5_n2": dict(frames=_checker(2, 3, 5), stamps=_uniform(2), cp=C02, cn=C02),
    }
    for c in out.values():
        c.setdefault("lut", lut)
        c.setdefault("bgr", False)
    return out


@functools.lru_cache(maxsize=None)
def _want(name):
    c = _cases()[name]
    state = R.reset(c["frames"][0], c["lut"], c["bgr"])
    rows, offsets, new_state, over = R.simulate(c["frames"], c["stamps"], state, c["lut"], c["cp"], c["cn"], c["bgr"])
    assert not over
    return rows, offsets, new_state


def _dev(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v


def _run(c, frames=None, lut_range=None, c_min=None):
    """reset + one ``ops.event_sim`` call -> (rows, offsets, state) on the host."""
    from refid_amd import ops
    frames = _dev(c["frames"]) if frames is None else frames
    lut = _dev(c["lut"])
    state = ops.event_sim_reset(frames[0], lut, bgr=c["bgr"])
    rows, offsets = ops.event_sim(frames, c["stamps"], state, lut, _dev(c["cp"]), _dev(c["cn"]), bgr=c["bgr"], lut_range=lut_range, c_min=c_min)
    assert rows.is_cuda and rows.dtype.is_floating_point and rows.dim() == 2 and rows.shape[1] == 4 and isinstance(offsets, np.ndarray)
    return rows.cpu().numpy(), offsets, state.cpu().numpy()


def _same(got, want, what):
    rows, offsets, state = got
    assert offsets.dtype == np.int64 and offsets.tolist() == want[1].tolist(), what
    assert rows.dtype == np.float32 and rows.shape == want[0].shape, what
    if rows.tobytes() != want[0].tobytes():
        bad = np.flatnonzero(np.any(rows.view(np.uint32) != want[0].view(np.uint32), axis=1))
        raise AssertionError(f"{what}: {len(bad)} of {len(rows)} rows differ, first at {bad[0]}: {rows[bad[0]]} != {want[0][bad[0]]}")
    assert state.dtype == np.int32 and state.tobytes() == want[2].tobytes(), what


@pytest.mark.parametrize("name", sorted(_cases()))
def test_the_device_equals_the_restatement_bit_for_bit(name):
    c, want = _cases()[name], _want(name)
    if name.startswith("static"):
        assert want[0].shape == (0, 4)
    elif "min_threshold" in name:
        assert int(np.diff(want[1]).max()) >= 254                       # the cap path, without overflow
    else:
        assert len(want[0]) > 0
    assert not np.any(np.diff(want[0][:, 0]) < 0)
    _same(_run(c), want, name)


def test_the_reset_state_is_the_table_at_the_luma():
    from refid_amd import ops
    for name in ("noise_9x57_n3_bgr", "noise_17x35_n3_linear_table", "noise_1x1_n3"):
        c = _cases()[name]
        state = ops.event_sim_reset(_dev(c["frames"])[1], _dev(c["lut"]), bgr=c["bgr"])
        assert state.cpu().numpy().tobytes() == R.reset(c["frames"][1], c["lut"], c["bgr"]).tobytes()


def test_known_extremes_and_reductions_in_ops_give_the_same_rows():
    """``lut_range`` / ``c_min`` from the caller against the reductions ``ops.event_sim`` makes itself."""
    for name in ("noise_9x57_n9_maps", "noise_17x35_n3_linear_table"):
        c = _cases()[name]
        lut_range = (int(c["lut"].min()), int(c["lut"].max()))
        c_min = int(min(np.min(c["cp"]), np.min(c["cn"])))
        _same(_run(c, lut_range=lut_range, c_min=c_min), _want(name), name)


def test_no_events_returns_an_empty_tensor_and_leaves_the_state():
    import torch
    from refid_amd import ops
    c = _cases()["static_9x57_n3"]
    frames, lut = _dev(c["frames"]), _dev(c["lut"])
    state = ops.event_sim_reset(frames[0], lut)
    before = state.clone()
    rows, offsets = ops.event_sim(frames, c["stamps"], state, lut, 1776, 1776)
    assert tuple(rows.shape) == (0, 4) and rows.dtype == torch.float32 and rows.is_cuda and offsets.tolist() == [0, 0, 0]
    assert torch.equal(state, before)


def test_an_unaligned_view_of_the_frames_gives_the_same_rows():
    import torch
    for name in ("noise_17x35_n9", "noise_9x57_n3_bgr"):
        c = _cases()[name]
        flat = torch.from_numpy(c["frames"]).reshape(-1)
        for shift in (1, 2, 3):
            buf = torch.zeros(flat.numel() + 8, dtype=torch.uint8, device="cuda")
            buf[shift:shift + flat.numel()] = flat.cuda()
            view = buf[shift:shift + flat.numel()].view(c["frames"].shape)
            assert view.data_ptr() % 4 == shift and view.is_contiguous()
            _same(_run(c, frames=view), _want(name), (name, shift))


def test_two_runs_are_identical():
    c = _cases()["noise_9x57_n9_maps"]
    a, b = _run(c), _run(c)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tolist() == b[1].tolist() and a[2].tobytes() == b[2].tobytes()


@pytest.mark.parametrize("name", ["noise_17x35_n9", "noise_9x57_n9_maps", "ramps_17x35_n9", "noise_3x5_n9_near_1e9"])
def test_chunks_that_share_boundary_frames_equal_one_call(name):
    """N = 9 in one call against chunks of 3 + 3 + 5 frames through ``EventSimulator.step``, and ``simulate(chunk=...)``."""
    import torch
    from refid_amd.event_sim import EventSimulator
    c, want = _cases()[name], _want(name)
    h, w = c["frames"].shape[1:3]
    sim = EventSimulator(h, w, lut=c["lut"])
    sim.c_pos, sim.c_neg = _dev(c["cp"]), _dev(c["cn"])                 # the case's fixed-point thresholds, as they are
    sim.c_min = int(min(np.min(c["cp"]), np.min(c["cn"]))) if isinstance(c["cp"], np.ndarray) else None
    frames = _dev(c["frames"])
    sim.reset(frames[0])
    rows, offsets, at = [], [np.zeros(1, dtype=np.int64)], 0
    for count in (3, 3, 5):
        r, o = sim.step(frames[at:at + count], c["stamps"][at:at + count])
        rows.append(r)
        offsets.append(o[1:] + offsets[-1][-1])
        at += count - 1
    _same((torch.cat(rows).cpu().numpy(), np.concatenate(offsets), sim.state.cpu().numpy()), want, name)
    for chunk in (2, 5, 9, 64):
        events, offsets = sim.simulate(c["frames"] if chunk == 5 else frames, c["stamps"], chunk=chunk)      # chunk 5: a host clip
        _same((events.cpu().numpy(), offsets, sim.state.cpu().numpy()), want, (name, chunk))
    from refid_amd._lib import RefidHipError
    with pytest.raises(RefidHipError, match="is not the previous chunk's last stamp"):
        sim.step(frames[:2], c["stamps"][:2])


def test_the_simulator_draws_its_maps_from_the_seed():
    from refid_amd.event_sim import EventSimulator, threshold_maps
    c = _cases()["noise_17x35_n9"]
    sim = EventSimulator(17, 35, c_pos=0.2, c_neg=0.3, sigma=0.05, seed=11)
    cp, cn = threshold_maps(17, 35, 0.2, 0.3, sigma=0.05, seed=11)
    assert sim.c_pos.cpu().numpy().tobytes() == cp.tobytes() and sim.c_min == int(min(cp.min(), cn.min()))
    events, offsets = sim.simulate(c["frames"], c["stamps"], chunk=4)
    want = R.simulate_chunked(c["frames"], c["stamps"], c["lut"], cp, cn, [9])
    _same((events.cpu().numpy(), offsets, sim.state.cpu().numpy()), want, "sigma")


def test_overflow_raises_the_flag_and_stays_inside_its_slots():
    """A threshold map whose smallest value belies ``c_min`` gets past the host check through the raw entry: the loop stops at
    255 events, the flag is raised, and nothing outside ``counts`` / ``rows`` / ``keys`` / ``state`` is written (guard bands
    on both sides).  Through ``ops.event_sim`` the same data raises and leaves ``state`` alone."""
    import torch
    from refid_amd import _lib, ops
    from refid_amd._lib import RefidHipError
    h, w, guard = 3, 5, 64
    hw = h * w
    frames_host = _flash(2, h, w)
    frames_host[:, 0, 0] = [[10, 10, 10], [200, 200, 200]]             # an ordinary pixel beside it
    cp_host = np.full((h, w), C02, dtype=np.int32)
    cp_host[h // 2, w // 2] = 600                                        # 452773 / 600 = 754 crossings wanted
    lut_host = R.default_lut()
    stamps = _uniform(2)
    state0 = R.reset(frames_host[0], lut_host)
    want_rows, want_offsets, want_state, over = R.simulate(frames_host, stamps, state0, lut_host, cp_host, C02)
    assert over and int(want_offsets[-1]) > 255 and int(np.sum((want_rows[:, 1] == w // 2) & (want_rows[:, 2] == h // 2))) == 255
    frames, lut, cp = _dev(frames_host), _dev(lut_host), _dev(cp_host)

    def banded(count, dtype, fill):
        buf = torch.full((count + 2 * guard,), fill, dtype=dtype, device="cuda")
        return buf, buf[guard:guard + count]

    state_buf, state = banded(hw, torch.int32, -7)
    state.copy_(_dev(state0).reshape(-1))
    counts_buf, counts = banded(hw, torch.int32, -7)
    totals_buf, totals = banded(2, torch.int64, -7)
    totals.zero_()
    stamps_dev = torch.from_numpy(stamps).cuda()
    desc = _lib.EventSimDesc(frames=frames.data_ptr(), stamps_host=stamps.ctypes.data, stamps_dev=stamps_dev.data_ptr(), lut=lut.data_ptr(),
                             c_pos_map=cp.data_ptr(), state=state.data_ptr(), counts=counts.data_ptr(), totals=totals.data_ptr(), n_frames=2,
                             height=h, width=w, c_neg=C02, c_min=1776, lut_min=int(lut_host.min()), lut_max=int(lut_host.max()),
                             stage=_lib.EVENT_SIM_COUNT)
    L = _lib.lib()
    stream = ops._stream()
    assert L.refid_event_sim(ctypes.byref(desc), stream) == 0, L.refid_last_error()
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    got = totals.cpu().tolist()
    total = int(ends[-1])
    assert got == [int(want_offsets[-1]), _lib.EVENT_SIM_FLAG_OVERFLOW] and total == got[0]
    assert int(counts.view(h, w)[h // 2, w // 2]) == 255
    rows_buf, rows = banded(total * 4, torch.float32, -7.0)
    keys_buf, keys = banded(total, torch.int64, -7)
    assert rows.data_ptr() % 16 == 0
    totals.zero_()
    desc.ends, desc.rows, desc.keys, desc.n_rows, desc.stage = ends.data_ptr(), rows.data_ptr(), keys.data_ptr(), total, _lib.EVENT_SIM_EMIT
    assert L.refid_event_sim(ctypes.byref(desc), stream) == 0, L.refid_last_error()
    torch.cuda.synchronize()
    assert totals.cpu().tolist() == [0, _lib.EVENT_SIM_FLAG_OVERFLOW]
    for buf, count in ((state_buf, hw), (counts_buf, hw), (totals_buf, 2), (rows_buf, total * 4), (keys_buf, total)):
        host = buf.cpu().numpy()
        assert np.all(host[:guard] == -7) and np.all(host[guard + count:] == -7)
    assert np.all(rows.cpu().numpy() != -7.0) and np.all(keys.cpu().numpy() >= 0) and len(np.unique(keys.cpu().numpy())) == total
    order = np.argsort(keys.cpu().numpy())
    assert rows.cpu().numpy().reshape(total, 4)[order].tobytes() == want_rows.tobytes()
    assert state.cpu().numpy().reshape(h, w).tobytes() == want_state.tobytes()
    # the public route: the flag becomes an error at the call's one synchronisation, before the emit pass
    state = _dev(state0)
    with pytest.raises(RefidHipError, match="overflow: a pixel has more than 255 events"):
        ops.event_sim(frames, stamps, state, lut, cp, C02, c_min=1776)
    assert state.cpu().numpy().tobytes() == state0.tobytes()
    with pytest.raises(RefidHipError, match="smallest threshold 600 allows"):
        ops.event_sim(frames, stamps, state, lut, cp, C02)              # with the map's true minimum the host refuses


def test_the_rows_feed_the_sequence_assembler_as_a_host_array_does():
    """End to end at 17x35, n = 1: the simulated rows, resident, into ``SequenceAssembler`` against the same rows as numpy."""
    import torch
    from refid_amd.event_sim import EventSimulator
    from refid_amd.sequence import SequenceAssembler, make_pairs, sharp_windows
    c = _cases()["noise_17x35_n9_jitter"]
    events, offsets = EventSimulator(17, 35, c_pos=0.2, c_neg=9000 / 65536).simulate(c["frames"], c["stamps"], chunk=4)
    host = events.cpu().numpy()
    assert host.tobytes() == _want("noise_17x35_n9_jitter")[0].tobytes()
    keys = c["frames"][::2]
    pairs = make_pairs(host[:, 0], *sharp_windows(c["stamps"][::2]))
    assert len(pairs) == 4 and sum(p.row1 - p.row0 for p in pairs) > 0
    out = [SequenceAssembler(1, 1, "sharp").load(keys, ev).assemble(pairs) for ev in (events, host)]
    assert torch.count_nonzero(out[0]["voxel"]) > 0
    assert torch.equal(out[0]["voxel"], out[1]["voxel"]) and torch.equal(out[0]["lq"], out[1]["lq"])


def test_the_command_line_with_split_writes_what_the_interpolator_reads(tmp_path):
    from refid_amd import png, sequence, simulate
    c = _cases()["noise_17x35_n9"]
    os.makedirs(tmp_path / "clip")
    for k, f in enumerate(c["frames"]):
        png.write_png(str(tmp_path / "clip" / f"{k:04d}.png"), f)
    out = str(tmp_path / "sim")
    assert simulate.main(["--frames", str(tmp_path / "clip"), "--fps", "240", "--out", out, "--split", "2", "--chunk", "4"]) == 0
    files = sorted(glob.glob(os.path.join(out, "events", "*.npz")))
    assert [os.path.basename(f) for f in files] == [f"{k:06d}.npz" for k in range(8)]
    want = _want("noise_17x35_n9")
    assert sequence.load_event_npz(files).tobytes() == want[0].tobytes()
    assert [len(np.load(f)["x"]) for f in files] == np.diff(want[1]).tolist()
    assert np.loadtxt(os.path.join(out, "stamps.txt")).tobytes() == c["stamps"].tobytes()
    assert np.loadtxt(os.path.join(out, "key_stamps.txt")).tobytes() == c["stamps"][::2].tobytes()
    assert sorted(os.listdir(os.path.join(out, "keys"))) == [f"{i:06d}.png" for i in range(5)]
    # gt/: the names SequenceInterpolator gives the outputs of pair i for n = 1
    runner_names = [os.path.basename(p) for i in range(4) for p in sequence.SequenceInterpolator._paths(None, "", f"{i:06d}", np.zeros((1, 1)))]
    assert sorted(os.listdir(os.path.join(out, "gt"))) == runner_names == [f"{i:06d}_00.png" for i in range(4)]
    for i in range(5):
        assert png.read_png(os.path.join(out, "keys", f"{i:06d}.png")).tobytes() == c["frames"][2 * i].tobytes()
    for i in range(4):
        assert png.read_png(os.path.join(out, "gt", f"{i:06d}_00.png")).tobytes() == c["frames"][2 * i + 1].tobytes()
