"""The pair form of the 2x4-tile Winograd weight gradient (csrc/wgrad_wino24.hip: eight waves, two input-channel tiles per
workgroup, the gradient tile staged once, a three-stage LDS-DMA ring) against the four-wave form it replaces.

A wave of the pair form runs the four-wave form's K loop on the same tiles in the same order, so the two forms must agree
BIT FOR BIT (torch.equal, no tolerance): every case runs the same call with REFID_W24_PAIR=0 and then =1.  Which form a call
took is observed through REFID_W24_PAIR=2, which turns the fallback to the four-wave form into an error.  Three cases on exact
data (small integers times powers of two: every sum is exact in fp32 whatever its order) -- 64 -> 64 (pair form), 64 -> 32 and
96 -> 64 (the four-wave kernel under both modes) -- are also held to a float64 per-tap GEMM at zero tolerance, so a lost or
doubled K tile fails even if both forms shared the bug."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ops():
    from refid_amd import ops
    return ops


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.rand(*shape, generator=g) * 2 - 1).cuda()


def make_steps(T, N, H, W, Ca, Cb, Co, down=False):
    Ho, Wo = (H // 2, W // 2) if down else (H, W)
    return [(rnd(N, Ho, Wo, Co, seed=100 + t), rnd(N, H, W, Ca, seed=200 + t), rnd(N, H, W, Cb, seed=300 + t) if Cb else None)
            for t in range(T)]


def geo_of(Ca, Cb, down=False):
    if down:
        return dict(kh=4, kw=4, stride=2, pad=1, algo=7, i_total=Ca + Cb)
    return dict(kh=3, kw=3, stride=1, pad=1, algo=5, i_total=Ca + Cb)


def both_forms(monkeypatch, fn):
    """fn() under the four-wave form and under the pair form: [(dw, db), (dw, db)]."""
    out = []
    for mode in ("0", "1"):
        monkeypatch.setenv("REFID_W24_PAIR", mode)
        out.append(fn())
        torch.cuda.synchronize()
    return out


def takes_pair(monkeypatch, steps, Ca, Cb, Co, down=False):
    """Does a one-shot call of this geometry take the pair form?  (=2: a launch that would fall back is an error.)"""
    from refid_amd import _lib
    ops = _ops()
    k = 4 if down else 3
    dw = torch.zeros(Co, Ca + Cb, k, k, device="cuda")
    g, a, b = steps[0]
    monkeypatch.setenv("REFID_W24_PAIR", "2")
    try:
        ops.conv2d_wgrad(g, a, dw, in_b=b, **geo_of(Ca, Cb, down))
        torch.cuda.synchronize()
        return True
    except _lib.RefidHipError:
        return False
    finally:
        monkeypatch.setenv("REFID_W24_PAIR", "1")


def one_shot(steps, Ca, Cb, Co, down=False):
    ops = _ops()
    k = 4 if down else 3
    dw = torch.zeros(Co, Ca + Cb, k, k, device="cuda"); db = torch.zeros(Co, device="cuda")
    g, a, b = steps[0]
    ops.conv2d_wgrad(g, a, dw, in_b=b, db=db, more=steps[1:], **geo_of(Ca, Cb, down))
    return dw, db


def assert_same(res):
    (dw0, db0), (dw1, db1) = res
    assert float(dw0.abs().max()) > 0 and float(db0.abs().max()) > 0
    assert torch.equal(dw0, dw1), float((dw0 - dw1).abs().max())
    assert torch.equal(db0, db1), float((db0 - db1).abs().max())


@pytest.mark.parametrize("cfg", [(1, 12, 40, 64, 0, 64), (2, 12, 40, 128, 0, 64), (1, 12, 40, 64, 64, 64)],
                         ids=["64to64", "128to64", "64+64to64"])
def test_pair_equals_four_wave(monkeypatch, cfg):
    """Partial tiles on both axes (12 = 3 x 4, 40 = 2.5 x 16), two and four input-channel tiles, one and two sources."""
    N, H, W, Ca, Cb, Co = cfg
    steps = make_steps(1, N, H, W, Ca, Cb, Co)
    assert takes_pair(monkeypatch, steps, Ca, Cb, Co)
    assert_same(both_forms(monkeypatch, lambda: one_shot(steps, Ca, Cb, Co)))


@pytest.mark.parametrize("cfg", [(1, 12, 40, 96, 0, 64), (1, 12, 40, 64, 0, 32)], ids=["three_input_tiles", "thin_output_tile"])
def test_fallback_to_four_wave(monkeypatch, cfg):
    """96 -> 64 has an odd number of input tiles, 64 -> 32 the 32-channel output tile: both stay on the four-wave form."""
    N, H, W, Ca, Cb, Co = cfg
    steps = make_steps(1, N, H, W, Ca, Cb, Co)
    assert not takes_pair(monkeypatch, steps, Ca, Cb, Co)
    assert_same(both_forms(monkeypatch, lambda: one_shot(steps, Ca, Cb, Co)))


def phased(steps, grouping, Ca, Cb, Co, phase4=False, first_without_b=False, down=False):
    ops = _ops()
    geo = geo_of(Ca, Cb, down)
    k = 4 if down else 3
    dw = torch.zeros(Co, Ca + Cb, k, k, device="cuda"); db = torch.zeros(Co, device="cuda")
    sl, first = None, True
    for grp in grouping:
        (g, a, b), more = steps[grp[0]], [steps[i] for i in grp[1:]]
        if first and first_without_b:
            b = None
        sl = ops.conv2d_wgrad(g, a, dw, in_b=b, db=db, phase=1 if first else 2, slabs=sl, more=more, **geo)
        first = False
    g, a, b = steps[grouping[-1][0]]
    ops.conv2d_wgrad(g, a, dw, in_b=b, db=db, phase=4 if phase4 else 3, slabs=sl, **geo)
    if phase4:
        ops.wgrad_finish_flush()
    return dw, db


def test_first_step_without_second_source(monkeypatch):
    """The first recurrent step has no second source yet: input tiles 2 / 3 lie beyond the sources (zero slabs), the later
    steps add both sources (accum)."""
    N, H, W, Ca, Cb, Co = 1, 12, 40, 64, 64, 64
    steps = make_steps(2, N, H, W, Ca, Cb, Co)
    res = both_forms(monkeypatch, lambda: phased(steps, [[0], [1]], Ca, Cb, Co, first_without_b=True))
    assert_same(res)
    only_first = both_forms(monkeypatch, lambda: phased(steps[:1], [[0]], Ca, Cb, Co, first_without_b=True))
    assert_same(only_first)
    assert float(only_first[1][0][:, Ca:].abs().max()) == 0.0


@pytest.mark.parametrize("phase4", [False, True], ids=["phase3", "phase4_flush"])
def test_grouped_time_steps_and_accum(monkeypatch, phase4):
    """Three grouped time steps in one launch (phase 1), a further launch added to the slabs (phase 2: accum), then the
    reduction (phase 3) or its queued form with the batched flush (phase 4)."""
    N, H, W, Ca, Cb, Co = 1, 12, 40, 64, 64, 64
    steps = make_steps(4, N, H, W, Ca, Cb, Co)
    assert_same(both_forms(monkeypatch, lambda: phased(steps, [[0, 1, 2], [3]], Ca, Cb, Co, phase4=phase4)))


def test_down_form(monkeypatch):
    """conv_down (4x4, stride 2; a 24 x 80 input) has a kernel of its own with no pair layout: REFID_W24_PAIR=2 does not raise
    for it, and =0 / =1 give the same bits, one-shot and phased."""
    N, H, W, Ca, Cb, Co = 1, 24, 80, 64, 0, 64
    steps = make_steps(2, N, H, W, Ca, Cb, Co, down=True)
    assert takes_pair(monkeypatch, steps, Ca, Cb, Co, down=True)
    assert_same(both_forms(monkeypatch, lambda: one_shot(steps[:1], Ca, Cb, Co, down=True)))
    assert_same(both_forms(monkeypatch, lambda: phased(steps, [[0], [1]], Ca, Cb, Co, down=True)))


# 64 -> 64 at 1 x 12 x 40 has 9 K tiles and 2 workgroups per split, so REFID_W24_WGS = 2 nsplit (nsplit < 8) plans
#   512 -> 9 splits of 1 tile | 16 -> 8 splits of 2, 2, 2, 2, 1, 0, 0, 0 | 10 -> 5 splits of 2, 2, 2, 2, 1
#   6 -> 3 splits of 3 | 4 -> 2 splits of 5 and 4 | 2 -> one split of 9:
# the ring's prologue (one or two requests), its drain, and the whole triples in between.
@pytest.mark.parametrize("wgs", [512, 16, 10, 6, 4, 2])
def test_short_k_ranges(monkeypatch, wgs):
    N, H, W, Ca, Cb, Co = 1, 12, 40, 64, 0, 64
    monkeypatch.setenv("REFID_W24_WGS", str(wgs))
    steps = make_steps(1, N, H, W, Ca, Cb, Co)
    res = both_forms(monkeypatch, lambda: one_shot(steps, Ca, Cb, Co))
    assert_same(res)
    monkeypatch.delenv("REFID_W24_WGS")
    ref = both_forms(monkeypatch, lambda: one_shot(steps, Ca, Cb, Co))[0][0]
    assert float((res[1][0] - ref).abs().max()) <= 1e-5 * float(ref.abs().max())       # another split plan: fp32 reordering only


# (Ca, Co) -> the split plan of 2 x 12 x 40 (18 K tiles) under REFID_W24_WGS=8, and the slab planes' padded channel counts:
#   64 -> 64  two input tiles, pair form:          8 / 2 = 4 splits of 5, 5, 5, 3 tiles
#   64 -> 32  32-channel output tile (NS = 1):     8 * 3 / 2 / 2 = 6 splits of 3
#   96 -> 64  three input tiles, four-wave form:   ceil(8 / 3) = 3 splits of 6
EXACT_CASES = {(64, 64): dict(nsplit=4, CoP=64, CiP=64), (64, 32): dict(nsplit=6, CoP=32, CiP=64),
               (96, 64): dict(nsplit=3, CoP=64, CiP=96)}


@pytest.mark.parametrize("chan", list(EXACT_CASES), ids=["64to64", "64to32", "96to64"])
def test_exact_data_against_float64_taps(monkeypatch, chan):
    """Small integers times powers of two: every product and every partial sum of the K loop is an integer below 2^24 times a
    power of two, so the slabs are exact in fp32 and 48 dW is an INTEGER combination of their transform planes
    (2 Ay^T and 24 Ax^T have integer entries) -- compared in float64 with 48 x the per-tap GEMM at zero tolerance.  The
    final gradients of the two forms are compared bit for bit as everywhere else; the bias gradient (a plain sum) is exact
    too.  K is pixels, not channels, so the data stay exact for every channel count: 64 -> 32 (NS = 1) and 96 -> 64 (an odd
    number of input tiles) take the four-wave kernel under both REFID_W24_PAIR modes and are held to float64 here."""
    ops = _ops()
    N, H, W = 2, 12, 40
    Ca, Co = chan
    plan = EXACT_CASES[chan]
    monkeypatch.setenv("REFID_W24_WGS", "8")
    gen = torch.Generator().manual_seed(5)
    x = torch.randint(-4, 5, (N, H, W, Ca), generator=gen).double() * 2.0 ** -3
    g = torch.randint(-4, 5, (N, H, W, Co), generator=gen).double() * 2.0 ** 5
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    ref = torch.stack([torch.stack([torch.einsum("nyxo,nyxi->oi", g, xp[:, ky:ky + H, kx:kx + W]) for kx in range(3)], -1)
                       for ky in range(3)], -2)                                     # (Co, Ca, 3, 3), float64, exact
    steps = [(g.float().cuda(), x.float().cuda(), None)]
    geo = geo_of(Ca, 0)
    nsplit, CoP, CiP = plan["nsplit"], plan["CoP"], plan["CiP"]
    planes = 24 * CoP * CiP

    def run():
        dw = torch.zeros(Co, Ca, 3, 3, device="cuda"); db = torch.zeros(Co, device="cuda")
        sl = ops.conv2d_wgrad(*steps[0][:2], dw, db=db, phase=1, **geo)
        ops.conv2d_wgrad(*steps[0][:2], dw, db=db, phase=3, slabs=sl, **geo)
        assert sl.numel() > nsplit * (planes + CoP) and (sl.numel() - nsplit * (planes + CoP)) % planes == 0, "split plan"
        u = sl[:nsplit * planes].double().cpu().view(nsplit, 4, 6, CoP, CiP).sum(0)[:, :, :Co, :Ca]   # [row][column point][o][i]
        t = [2 * u[0] + u[1] + u[2], u[1] - u[2], u[1] + u[2] + 2 * u[3]]          # 2 Ay^T u: [p][column point][o][i]
        dw48 = torch.stack([torch.stack([6 * tp[0] - 4 * (tp[1] + tp[2]) + (tp[3] + tp[4]),
                                         4 * (tp[2] - tp[1]) + 2 * (tp[3] - tp[4]),
                                         4 * ((tp[3] + tp[4]) - (tp[1] + tp[2])) + 24 * tp[5]], -1) for tp in t], -2)
        return dw, db, dw48

    for mode in ("0", "1"):
        monkeypatch.setenv("REFID_W24_PAIR", mode)
        dw, db, dw48 = run()
        assert torch.equal(dw48, 48 * ref), (mode, float((dw48 - 48 * ref).abs().max()))
        assert torch.equal(db.double().cpu(), g.sum((0, 1, 2))), mode
        if mode == "0":
            dw0, db0 = dw, db
    assert torch.equal(dw0, dw) and torch.equal(db0, db)
    assert float((dw.double().cpu() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
