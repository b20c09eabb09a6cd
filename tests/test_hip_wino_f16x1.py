"""The ONE-fp16-product Winograd form (refid_conv2d algo 5, mfma_terms 1: compute_dtype 'fp16') per element against float64.

Contract, for every output element o:

    |got_o - ref_o| <= C * 2^-11 * S_o,        C = 2

with ref the float64 torch convolution and S_o the patch-max error scale of tests/test_hip_precision.py::ref_wino, on that file's
data families a, b, c, d and e9 (e9 = its S_ENV_WINO envelope), forward and input gradient, under ops.WINO_SPLIT 0 and 2.  NaN or
inf fails.  2^-11 is the unit roundoff of an fp16 operand: the form rounds U = G g G^T (times a per-tensor power of two) and
V = B^T d B (times a per-tile, per-transform-row power of two) ONCE to fp16 and accumulates in fp32.

Where C comes from: the float64 emulation in this file (emulate_x1: F(2,3) transforms, both operands rounded to nearest even to
fp16 including subnormals, one V scale per tile and transform row) gave a worst ratio err / (2^-11 S) of 0.65 over exactly the
shapes and families below when the bound was set (family d, the 32-row input gradient; 0.47 with this file's seeds).  C = 2
leaves a factor 3 for what the emulation does not model: the ONLINE reference exponent along K (a chunk may be scaled by the exponent of an earlier, up to 2^6 smaller, maximum) and the
fp32 rounding inside the transforms.  test_emulation_meets_the_bound (no GPU) holds the emulation to C, so the bound cannot drift
away from the arithmetic it describes.  The bf16 one-product direct tile (algo 4, terms 1: what compute_dtype 'bf16' runs) sits at
0.24 - 2.2 in the same units on the same data.

Family e20 (operand scales 2^-20 .. 2^20 along K, compensated in the weights) is OUTSIDE the contract: the weights of the channels
at one end fall below fp16's subnormal step of the per-tensor scaled U (the emulation gives ~170 x the unit); only finiteness is
asserted.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_hip_precision import S_ENV_WINO, make_data, nchw, nhwc, ref_wino

C_X1 = 2.0
U16 = 2.0 ** -11
FAMILIES = ["a", "b", "c", "d", "e%d" % S_ENV_WINO]

# (role, N, Ca, Cb, Co, H, W, rows): forward: in_a / in_b channels -> Co; input gradient: the output gradient has Ca channels,
# the conv is Ca -> Co ... and rows = (base, count) asks for a row range of the Co input-gradient channels (refid_conv_desc.co_base)
CASES = [
    ("fwd", 1, 64, 0, 64, 20, 36, None),        # ragged tiles, 64-channel workgroup tile
    ("fwd", 1, 64, 64, 64, 13, 35, None),       # two sources
    ("fwd", 2, 32, 0, 3, 16, 40, None),         # thin output (pred), 32-channel tile
    ("fwd", 1, 40, 0, 64, 12, 34, None),        # partial last K chunk
    ("fwd", 1, 128, 0, 128, 16, 24, None),      # split-K under policy 2
    ("dgrad", 1, 64, 0, 64, 20, 36, None),
    ("dgrad", 1, 128, 0, 128, 20, 36, None),
    ("dgrad", 1, 64, 0, 64, 18, 34, (32, 32)),  # a 32-row range of the 64 input-gradient channels
]


def _id(c):
    return "%s-%d-%d+%dto%d-%dx%d%s" % (c[:7] + ("-rows%d+%d" % c[7] if c[7] else "",))


@functools.lru_cache(maxsize=None)
def problem(case, family):
    """(x, w, ref, S) of a case, computed once per session: the float64 reference is shared by the GPU test and the emulation."""
    role, N, Ca, Cb, Co, H, W, rows = case
    dgrad = role == "dgrad"
    seed = 40 + CASES.index(case) if case in CASES else 39
    if dgrad:
        x, w = make_data(family, (N, Ca, H, W), (Ca, Co, 3, 3), 0, seed=seed, hot=(8, 32, 5, 13))
    else:
        x, w = make_data(family, (N, Ca + Cb, H, W), (Co, Ca + Cb, 3, 3), 1, seed=seed, hot=(8, 32, 5, 13))
    ref, S, _ = ref_wino(x, w, dgrad)
    if rows is not None:
        ref, S = ref[:, rows[0]:rows[0] + rows[1]], S[:, rows[0]:rows[0] + rows[1]]
    return x, w, ref, S


def worst_ratio(got, ref, S, what, c=C_X1):
    """Largest |got - ref| / (2^-11 S); every element within c of it, NaN / inf fail."""
    assert bool(torch.isfinite(got).all()), f"{what}: NaN or inf in the result"
    err = (got - ref).abs()
    ratio = torch.where(S > 0, err / (U16 * S), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio.max())
    print(f"{what}: worst |err| / (2^-11 S) = {worst:.3g}")
    assert worst <= c, f"{what}: worst |err| / (2^-11 S) = {worst:.3g} > {c} ({int((ratio > c).sum())} of {ratio.numel()} elements)"
    return worst


# ---- float64 emulation of the arithmetic (no GPU) ---------------------------------------------------------------------------
def rne16(v):
    """Round float64 values to the nearest fp16 number, ties to even, subnormals included (step 2^-24 below 2^-14)."""
    a = v.abs()
    _, e = torch.frexp(a)                                     # a = m 2^e, m in [0.5, 1)
    q = torch.exp2((torch.clamp(e - 1, min=-14) - 10).double())
    r = torch.round(a / q) * q                                # torch.round: half to even
    assert float(r.max()) <= 65504.0, "fp16 overflow in the emulation"
    return torch.sign(v) * r


_G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
_BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
_AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)


def _floor_log2(a):
    return torch.frexp(a)[1] - 1


def emulate_x1(x, w, dgrad):
    """The one-product form in float64: U 2^eU and V 2^(7 - e) rounded once to fp16, exact products and sums, exact un-scale."""
    g = w.transpose(0, 1).flip(2, 3) if dgrad else w          # (rows, K, 3, 3): the input gradient is a conv with these taps
    U = torch.einsum("ia,rkab,jb->rkij", _G, g, _G)
    eU = 12 - int(_floor_log2(w.abs().max()))                 # refid_pack_conv_weights_wino1h: max |U| 2^eU in [2^12, 2^15)
    Uh = rne16(U * 2.0 ** eU)
    N, C, H, W = x.shape
    ty, tx = -(-H // 2), -(-W // 2)
    xp = F.pad(x, (1, 2 * tx + 1 - W, 1, 2 * ty + 1 - H))
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)                    # (N, C, ty, tx, 4, 4)
    t = torch.einsum("ia,nctuab->nctuib", _BT, d)             # row transform: what a lane scales
    m = t.abs().amax(dim=(1, 5))                              # (N, ty, tx, i): per tile and transform row, all of K
    sc = torch.exp2((7 - _floor_log2(torch.where(m > 0, m, torch.ones_like(m)))).double())[:, None, :, :, :, None]
    Vh = rne16(torch.einsum("jb,nctuib->nctuij", _BT, t * sc))
    M = torch.einsum("rkij,nktuij->nrtuij", Uh, Vh) / sc * 2.0 ** -eU
    Y = torch.einsum("ai,nrtuij,bj->nrtaub", _AT, M, _AT)     # (N, rows, ty, 2, tx, 2)
    return Y.reshape(N, g.shape[0], 2 * ty, 2 * tx)[:, :, :H, :W]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_emulation_meets_the_bound(case, family):
    """Keeps C honest: the arithmetic the bound was derived from meets it on every shape and family of the GPU test."""
    x, w, ref, S = problem(case, family)
    got = emulate_x1(x, w, case[0] == "dgrad")
    if case[7] is not None:
        got = got[:, case[7][0]:case[7][0] + case[7][1]]
    worst_ratio(got, ref, S, f"emulation {_id(case)} family {family}")


def test_rne16_is_fp16_rounding():
    """The emulation's rounding against torch's own float32 -> float16 conversion (normal, subnormal, ties, zero)."""
    g = torch.Generator().manual_seed(7)
    v = (torch.rand(4096, generator=g, dtype=torch.float64) * 2 - 1) * torch.exp2(torch.randint(-28, 16, (4096,), generator=g).double())
    v = torch.cat([v.float().double(), torch.tensor([0.0, 2.0 ** -25, 3 * 2.0 ** -25, 2049.0, 2051.0, -2.0 ** -24, 1.0 + 2.0 ** -11])])
    assert torch.equal(rne16(v), v.float().half().double())


# ---- the kernel -------------------------------------------------------------------------------------------------------------
def _ops():
    from refid_amd import ops
    return ops


def run_x1(x, w, dgrad=False, ca=None, rows=None, **epilogue):
    """3x3 / pad 1 forward (two sources when ca < channels of x) or input gradient (rows = (base, count): a row range) on one
    fp16 product.  epilogue: conv2d keywords (NHWC CUDA tensors)."""
    ops = _ops()
    Co, Ci = w.shape[:2]
    total = Ci if dgrad else Co
    base, cnt = rows if rows is not None else (0, total)
    role = ops.ROLE_WINO_DGRAD if dgrad else ops.ROLE_WINO_FWD
    wp = ops.pack_conv_weights_wino6(w.float().cuda().contiguous(), role, Co, Ci, terms=1)
    N, C, H, W = x.shape
    out = torch.full((N, H, W, -(-cnt // 4) * 4), float("nan"), device="cuda")[..., :cnt]
    ca = ca or C
    ops.conv2d(nhwc(x[:, :ca]), wp, out, kh=3, kw=3, stride=1, pad=1, cout=cnt, cout_pad=-(-total // 64) * 64, co_base=base, algo=5,
               terms=1, in_b=nhwc(x[:, ca:]) if ca < C else None, **epilogue)
    return nchw(out)


def run_bf16_direct(x, w, dgrad=False):
    """The bf16 one-product direct tile (algo 4, terms 1): the calibration of the rms gate, not the code under test."""
    ops = _ops()
    Co, Ci = w.shape[:2]
    rows = Ci if dgrad else Co
    bn = ops.conv_bn(3, 3, 1, 0, rows)
    wp = ops.pack_conv_weights_split(w.float().cuda().contiguous(), ops.ROLE_DGRAD if dgrad else ops.ROLE_FWD, bn, 3, 3, Co, Ci, planes=1)
    N, C, H, W = x.shape
    out = torch.full((N, H, W, rows), float("nan"), device="cuda")
    ops.conv2d(nhwc(x), wp, out, kh=3, kw=3, stride=1, pad=1, cout=rows, cout_pad=-(-rows // bn) * bn, algo=4, terms=1)
    return nchw(out)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES + ["e20"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_one_product_form_elementwise_against_float64(monkeypatch, case, family):
    role, N, Ca, Cb, Co, H, W, rows = case
    x, w, ref, S = problem(case, family)
    ops = _ops()
    for split in (0, 2):
        monkeypatch.setattr(ops, "WINO_SPLIT", split)
        got = run_x1(x, w, role == "dgrad", Ca if Cb else None, rows)
        if family == "e20":                                   # outside the contract (module docstring): finite, nothing more
            assert bool(torch.isfinite(got).all()), f"{_id(case)} split {split} family e20: NaN or inf"
        else:
            worst_ratio(got, ref, S, f"one fp16 product {_id(case)} split {split} family {family}")


@pytest.mark.gpu
def test_fused_epilogue_on_the_one_product_form():
    """bias + slope_pre + res + mask + out2 against the same epilogue applied to the float64 conv.  Every epilogue step is
    1-Lipschitz in the conv's value (slopes <= 1), so the conv's bound carries over to both outputs."""
    N, Ci, Co, H, W = 1, 64, 64, 20, 36
    x, w, ref, S = problem(("fwd", N, Ci, 0, Co, H, W, None), "a")
    g = torch.Generator().manual_seed(5)
    bias = (torch.rand(Co, generator=g, dtype=torch.float64) - 0.5).float().double()
    res, mask, add2 = ((torch.rand(N, Co, H, W, generator=g, dtype=torch.float64) * 2 - 1).float().double() for _ in range(3))
    pre = ref + bias.view(1, -1, 1, 1)
    pre = torch.where(pre > 0, pre, 0.2 * pre)
    want = (pre + res) * torch.where(mask > 0, 1.0, 0.3)
    out2 = torch.full((N, H, W, Co), float("nan"), device="cuda")
    got = run_x1(x, w, bias=bias.float().cuda(), slope_pre=0.2, res=nhwc(res), mask=nhwc(mask), slope_mask=0.3, add2=nhwc(add2), out2=out2)
    worst_ratio(got, want, S, "one fp16 product, fused epilogue: out")
    worst_ratio(nchw(out2), want + add2, S, "one fp16 product, fused epilogue: out2")
    assert torch.equal(nchw(out2), (got.float() + add2.float()).double()), "out2 is out + add2, one fp32 add per element"


@pytest.mark.gpu
@pytest.mark.parametrize("role", ["fwd", "dgrad"])
def test_rms_error_and_the_bf16_direct_tile(role):
    """Family (a): rms(err) / rms(ref) <= 1e-3 (the emulation gives 5.0e-4) and smaller than the bf16 one-product direct tile's
    on the same data (2.3e-3: 8 significand bits against 11, on 9/4 of the multiplies)."""
    x, w, ref, S = problem((role, 1, 64, 0, 64, 20, 36, None), "a")
    dgrad = role == "dgrad"
    rms = lambda t: float(t.pow(2).mean().sqrt())
    e1 = rms(run_x1(x, w, dgrad) - ref) / rms(ref)
    eb = rms(run_bf16_direct(x, w, dgrad) - ref) / rms(ref)
    print(f"{role}: rms error / rms result: one fp16 product {e1:.3g}, bf16 direct tile {eb:.3g}")
    assert e1 <= 1.0e-3, (e1, eb)
    assert e1 < eb, (e1, eb)


@pytest.mark.gpu
def test_online_rescale_along_k_and_between_tiles(monkeypatch):
    """The per-lane reference exponent: (1) channels that grow by 2^40 along K (chunk c scaled by 2^(10 c), falling again: the
    accumulators are rescaled at every chunk on the way up), (2) neighbouring 8-column bands 2^20 and 2^-20 (tiles whose patch
    lies inside one band, and tiles that straddle the step).  Both stay inside the per-element bound."""
    N, Ci, Co, H, W = 1, 256, 64, 16, 64
    x, w = make_data("a", (N, Ci, H, W), (Co, Ci, 3, 3), 1, seed=61)
    ramp = torch.tensor([2.0 ** (10 * min(c, 9 - c)) if c < 10 else 1.0 for c in range(Ci // 16)], dtype=torch.float64)
    xr = (x * ramp.repeat_interleave(16).view(1, Ci, 1, 1)).float().double()
    ref, S, _ = ref_wino(xr, w, False)
    for split in (0, 2):
        monkeypatch.setattr(_ops(), "WINO_SPLIT", split)
        worst_ratio(run_x1(xr, w), ref, S, f"2^40 ramp along K, split {split}")
    col = torch.tensor([2.0 ** (20 if (c // 8) % 2 == 0 else -20) for c in range(W)], dtype=torch.float64)
    xs = (x[:, :64] * col.view(1, 1, 1, W)).float().double()
    ws = w[:, :64].contiguous()
    ref, S, _ = ref_wino(xs, ws, False)
    worst_ratio(run_x1(xs, ws), ref, S, "2^+-20 step between neighbouring tiles")


@pytest.mark.gpu
@pytest.mark.parametrize("split", [0, 1])
def test_a_sample_has_the_same_bits_in_any_batch(monkeypatch, split):
    """Sample 0's result bits at B = 1, 2 and 8, forward and input gradient 64 -> 64 at 128^2 on family (c) data: the V scale is
    per tile, the split-K policy per sample."""
    monkeypatch.setattr(_ops(), "WINO_SPLIT", split)
    x, w = make_data("c", (8, 64, 128, 128), (64, 64, 3, 3), 1, seed=33)
    for dgrad in (False, True):
        base = run_x1(x[:1], w, dgrad)
        assert bool(torch.isfinite(base).all())
        for B in (2, 8):
            got = run_x1(x[:B], w, dgrad)[:1]
            assert torch.equal(got, base), (dgrad, B, int((got != base).sum()))


@pytest.mark.gpu
def test_first_source_alone_reads_the_first_chunks_of_the_packing():
    """The first recurrent step of a two-source conv has no second source yet: the call reads the first 64 of the packing's 128
    input channels (chunk-major layout).  Same bound, against the float64 conv over those channels."""
    ops = _ops()
    x, w, _, _ = problem(("fwd", 1, 64, 64, 64, 13, 35, None), "a")
    ref, S, _ = ref_wino(x[:, :64], w[:, :64].contiguous(), False)
    wp = ops.pack_conv_weights_wino6(w.float().cuda().contiguous(), ops.ROLE_WINO_FWD, 64, 128, terms=1)
    out = torch.full((1, 13, 35, 64), float("nan"), device="cuda")
    ops.conv2d(nhwc(x[:, :64]), wp, out, kh=3, kw=3, stride=1, pad=1, cout=64, cout_pad=64, algo=5, terms=1)
    worst_ratio(nchw(out), ref, S, "first source alone")


@pytest.mark.gpu
def test_bad_arguments():
    ops = _ops()
    from refid_amd._lib import RefidHipError
    w = torch.randn(64, 64, 3, 3, device="cuda")
    x, out = torch.randn(1, 8, 32, 64, device="cuda"), torch.empty(1, 8, 32, 64, device="cuda")
    two = ops.pack_conv_weights_wino6(w, ops.ROLE_WINO_FWD, 64, 64, terms=3)
    one = ops.pack_conv_weights_wino6(w, ops.ROLE_WINO_FWD, 64, 64, terms=1)
    assert one.numel() * 2 - 64 == (two.numel() * 2 - 64) // 2 == ops.packed_weight_wino6_bytes(ops.ROLE_WINO_FWD, 64, 64, terms=1) - 64
    assert two.numel() * 2 == ops.packed_weight_wino6_bytes(ops.ROLE_WINO_FWD, 64, 64, f16=True)      # (the older keyword)
    geo = dict(kh=3, kw=3, stride=1, pad=1, cout=64, cout_pad=64, algo=5)
    with pytest.raises(RefidHipError, match="one-plane"):
        ops.conv2d(x, two, out, terms=1, **geo)               # a two-plane packing: the wrong size for one product
    with pytest.raises(RefidHipError, match="mfma_terms"):
        ops.conv2d(x, two, out, terms=2, **geo)
    with pytest.raises(RefidHipError, match="terms"):
        ops.pack_conv_weights_wino6(w, ops.ROLE_WINO_FWD, 64, 64, terms=2)
    ops.conv2d(x, one, out, terms=1, **geo)
    assert bool(torch.isfinite(out).all())
