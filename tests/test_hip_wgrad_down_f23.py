"""conv_down's weight gradient in its F(2,3) x F(2,4) form (csrc/wgrad_wino24.hip: wgrad_wino24_down_kernel, 3 x 4 gradient
tiles and a 4 x 5 window per parity phase, 20 transform planes) against a float64 per-tap GEMM on the CPU, and against the
direct tile (algo 0).

Exact data is family (g) of test_hip_wgrad_precision (integers times 2^s per channel, the gradient 1/128 dense): every product
and partial sum of the K loop, the slabs and the fold is an integer below 2^24 units whatever its order, so the only rounding is
the final inverse transform (1/2, 1/6, 1/3) -- held to C_EXACT_W24 x 2^-24 S^W on every one of the 16 taps.  A lost phase, tile
row, transform point, K tile, slab or a tap scattered to the wrong (ky, kx) is off by whole units and fails it outright; the
bookkeeping cases (thin tiles, two sources, grouped / accumulated / queued launches, short K ranges) therefore run on it too.
Sums over several launches are compared with the float64 sum under the same gate (the slabs add exactly; the one inverse
transform rounds as for one launch), which holds them to the sum of the one-shot gradients as tightly as fp32 can."""
import functools

import pytest
import torch

from test_hip_wgrad_precision import C_EXACT_W24, R_W24, fam_tensor, ref_direct, unit, wino_scale
from test_hip_precision import check

pytestmark = pytest.mark.gpu

GEO = dict(kh=4, kw=4, stride=2, pad=1, algo=7)
# (N, Ho, Wo): 7 x 21 = one full 6-row K tile + a 1-row remainder, one full 16-column tile + a 4-column tile + 1 column, and a
# sample boundary; 16 x 16 the engine's smallest; 6 x 10 one partial K tile
SHAPES = [(2, 7, 21), (2, 16, 16), (2, 6, 10)]
IDS = ["7x21", "16x16", "6x10"]


def _ops():
    from refid_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def exact_steps(N, Ho, Wo, Co, Ci, T=1):
    """[(g, x)] float64 of family (g), and per step (dW, db, S^W) in float64."""
    steps, refs = [], []
    for t in range(T):
        g = fam_tensor("g", "g", (N, Ho, Wo, 64), 700 + 10 * t)[..., :Co].contiguous()
        x = fam_tensor("g", "x", (N, 2 * Ho, 2 * Wo, 64), 701 + 10 * t)[..., :Ci].contiguous()
        dW, _, db, _ = ref_direct(g, x, 4, 2, 1)
        SW = wino_scale(g, x, 7)
        units = unit("g", 64)[:Co].view(-1, 1) * unit("x", 64)[:Ci].view(1, -1)
        assert float((R_W24 * SW / units).max()) < 2.0 ** 24, "family (g) data not exact at this size"
        steps.append((g, x))
        refs.append((dW, db, SW))
    return steps, refs


def gpu_step(g, x, Ca=None):
    """(g, in_a, in_b) fp32 on the GPU; Ca splits x's channels into two sources."""
    gf, xf = g.float().cuda(), x.float().cuda()
    if Ca is None:
        return gf, xf, None
    return gf, xf[..., :Ca].contiguous(), xf[..., Ca:].contiguous()


def one_shot(step, Co, Ci, **geo):
    g, a, b = step
    dw = torch.zeros(Co, Ci, 4, 4, device="cuda"); db = torch.zeros(Co, device="cuda")
    _ops().conv2d_wgrad(g, a, dw, in_b=b, db=db, i_total=Ci, **{**GEO, **geo})
    torch.cuda.synchronize()
    return dw.double().cpu(), db.double().cpu()


def hold_exact(dw, db, dW, dbr, SW, what):
    worst = check(dw, dW, SW.view(*SW.shape, 1, 1).expand_as(dW), C_EXACT_W24, what + " vs S^W")
    print(f"{what}: worst err / (2^-24 S^W) = {worst:.3g}")
    assert float(dW.abs().max()) > 0
    assert torch.equal(db, dbr), f"{what}: bias gradient differs from float64 (max {float((db - dbr).abs().max()):.3e})"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exact_data_every_tap(shape):
    N, Ho, Wo = shape
    steps, refs = exact_steps(N, Ho, Wo, 64, 64)
    dw, db = one_shot(gpu_step(*steps[0]), 64, 64)
    hold_exact(dw, db, *refs[0], f"down F(2,3)xF(2,4) 64->64 at {N}x{Ho}x{Wo}")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_random_data_against_the_direct_tile(shape):
    """|F23 - direct| < 3e-5 max|dW| (the bar test_hip_conv::test_conv_down_wgrad_through_parity_phases sets between algo 7 and
    the direct tile), db against sum g < 1e-5, and each side against float64 per tap, so a failure says which side moved."""
    N, Ho, Wo = shape
    gen = torch.Generator().manual_seed(11 + Ho)
    g = (torch.rand(N, Ho, Wo, 64, generator=gen) * 2 - 1).cuda()
    x = (torch.rand(N, 2 * Ho, 2 * Wo, 64, generator=gen) * 2 - 1).cuda()
    dw1, db1 = one_shot((g, x, None), 64, 64)
    dw0, db0 = one_shot((g, x, None), 64, 64, algo=0)
    d = float((dw1 - dw0).abs().max() / dw0.abs().max())
    print(f"F(2,3) x F(2,4) vs direct tile at {shape}: {d:.3g} of max|dW|")
    assert not torch.equal(dw1, dw0), "both calls took the same kernel"
    assert d < 3e-5
    dbr = g.double().cpu().sum((0, 1, 2))
    assert float((db1 - dbr).abs().max() / dbr.abs().max()) < 1e-5
    # and against float64 per tap
    dW, _, _, _ = ref_direct(g.double().cpu(), x.double().cpu(), 4, 2, 1)
    d1, d0 = (float((dw - dW).abs().max() / dW.abs().max()) for dw in (dw1, dw0))
    print(f"vs float64 at {shape}: F(2,3) x F(2,4) {d1:.3g}, direct tile {d0:.3g} of max|dW|")
    assert d1 < 3e-5
    assert d0 < 3e-5


@pytest.mark.parametrize("Co,Ci", [(32, 64), (64, 32), (32, 32)], ids=["co32", "ci32", "co32_ci32"])
def test_thin_tiles(Co, Ci):
    """c_o = 32 takes the 32-channel output tile (NS = 1), c_i = 32 a single input tile."""
    N, Ho, Wo = SHAPES[0]
    steps, refs = exact_steps(N, Ho, Wo, Co, Ci)
    dw, db = one_shot(gpu_step(*steps[0]), Co, Ci)
    hold_exact(dw, db, *refs[0], f"down F(2,3)xF(2,4) {Ci}->{Co}")


def phased(steps, grouping, Co, Ci, phase4=False, first_without_b=False):
    ops = _ops()
    dw = torch.zeros(Co, Ci, 4, 4, device="cuda"); db = torch.zeros(Co, device="cuda")
    sl, first = None, True
    for grp in grouping:
        (g, a, b), more = steps[grp[0]], [steps[i] for i in grp[1:]]
        if first and first_without_b:
            b = None
        sl = ops.conv2d_wgrad(g, a, dw, in_b=b, db=db, phase=1 if first else 2, slabs=sl, more=more, i_total=Ci, **GEO)
        first = False
    g, a, b = steps[grouping[-1][0]]
    ops.conv2d_wgrad(g, a, dw, in_b=b, db=db, phase=4 if phase4 else 3, slabs=sl, i_total=Ci, **GEO)
    if phase4:
        ops.wgrad_finish_flush()
    torch.cuda.synchronize()
    return dw.double().cpu(), db.double().cpu()


def test_two_sources_and_first_step_without_the_second():
    N, Ho, Wo = SHAPES[0]
    steps, refs = exact_steps(N, Ho, Wo, 64, 64, T=2)
    gs = [gpu_step(g, x, Ca=32) for g, x in steps]
    dw, db = one_shot(gs[0], 64, 64)
    hold_exact(dw, db, *refs[0], "two sources 32 + 32, one shot")
    # first step without its second source: its columns beyond Ca stay exactly 0
    dw, db = phased(gs[:1], [[0]], 64, 64, first_without_b=True)
    assert float(dw[:, 32:].abs().max()) == 0.0
    dW, dbr, SW = refs[0]
    hold_exact(dw[:, :32], db, dW[:, :32], dbr, SW[:, :32], "first step without the second source")
    # ... and the second step adds both sources
    dw, db = phased(gs, [[0], [1]], 64, 64, first_without_b=True)
    dWa, dWb = refs[0][0].clone(), refs[1][0]
    dWa[:, 32:] = 0
    x0 = steps[0][1].clone(); x0[..., 32:] = 0
    hold_exact(dw, db, dWa + dWb, refs[0][1] + refs[1][1], wino_scale(steps[0][0], x0, 7) + refs[1][2], "accumulated second step")


@pytest.mark.parametrize("phase4", [False, True], ids=["phase3", "phase4_flush"])
def test_grouped_time_steps_and_accum(phase4):
    """Three grouped time steps in one launch (phase 1), a further launch added to the slabs (phase 2), then the reduction
    (phase 3) or its queued form with the batched flush (phase 4): the float64 sum of the four one-shot gradients."""
    N, Ho, Wo = SHAPES[0]
    steps, refs = exact_steps(N, Ho, Wo, 64, 64, T=4)
    gs = [gpu_step(g, x) for g, x in steps]
    dw, db = phased(gs, [[0, 1, 2], [3]], 64, 64, phase4=phase4)
    hold_exact(dw, db, sum(r[0] for r in refs), sum(r[1] for r in refs), sum(r[2] for r in refs), "grouped + accumulated")
    shots = [one_shot(s, 64, 64) for s in gs]
    # each one-shot gradient is within the gate of its own float64 value (and S^W adds over the steps), the phased one within
    # the gate of the float64 sum: the two are at most two gates apart (the one-shot gradients are added in float64 here)
    check(dw, sum(s[0] for s in shots), sum(r[2] for r in refs).view(64, 64, 1, 1).expand_as(dw), 2 * C_EXACT_W24, "one-shot sum")


# 64 -> 64 at 2 x 7 x 21 has 8 K tiles and 8 workgroups per split (two input tiles x four phases):
#   512 -> 8 splits of 1 tile | 40 -> 5 splits of 2, 2, 2, 2, 0 | 24 -> 3 splits of 3, 3, 2 | 16 -> 2 splits of 4:
# the two-stage loop's odd last tile, its whole pairs, and an empty range
@pytest.mark.parametrize("wgs", [512, 40, 24, 16])
def test_short_k_ranges(monkeypatch, wgs):
    N, Ho, Wo = SHAPES[0]
    monkeypatch.setenv("REFID_W24_WGS", str(wgs))
    steps, refs = exact_steps(N, Ho, Wo, 64, 64)
    dw, db = one_shot(gpu_step(*steps[0]), 64, 64)
    hold_exact(dw, db, *refs[0], f"REFID_W24_WGS={wgs}")


def test_pair_switch_has_no_effect(monkeypatch):
    """REFID_W24_PAIR does not touch this form: =0 and =2 (which must not raise) give the default's bits."""
    N, Ho, Wo = SHAPES[1]
    steps, _ = exact_steps(N, Ho, Wo, 64, 64)
    gs = gpu_step(*steps[0])
    ref = one_shot(gs, 64, 64)
    for mode in ("0", "2"):
        monkeypatch.setenv("REFID_W24_PAIR", mode)
        got = one_shot(gs, 64, 64)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
