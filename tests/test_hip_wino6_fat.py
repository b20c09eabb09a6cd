"""conv_wino6's in-group split-K (csrc/conv_wino6.hip, KG = 2): where the small-grid plan asks for exactly two K ranges, one
512-thread workgroup per output tile reduces both (waves 0-3 / 4-7) and adds them in LDS instead of writing two partial outputs
for a finishing launch.  The bits must be the grid split's.  (The other "fat workgroup" form, two pixel blocks per wave for the
32-output-channel tile, was not built: DESIGN.md section 7.)

Every case calls refid_conv2d twice through ops.conv2d -- wino_tile 0 (the library's choice) and wino_tile 5 (the routing
before the in-group split: grid split + finishing kernel) -- and asserts torch.equal on out (and out2).  Routing is asserted
through the split-K workspace the caller lends: the in-group form must leave it untouched, the grid split must write it, so a
silent fallback in either direction fails.  One case per family is also compared with the float64 torch convolution at
test_hip_conv.py's fp32-class tolerance, so the two routes cannot be wrong together.

Plans at N = 1, 8 x 32 pixels under the default split policy (by total grid): 8 or 9-11 chunks of 16 input channels give
ks == 2 (128 channels and fewer take the small-grid 32-channel tile, NT = 1; above, the 64-channel tile), 16 chunks give ks == 4.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5                 # test_hip_conv.py's fp32-class tolerance on O(1) data
SENTINEL = -12345.0
PARENT = 5                              # refid_conv_desc.wino_tile: the parent's routing


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().cuda()


def nhwc_quads(t):
    """NHWC view of the tensor's channels inside a buffer padded to whole channel quads (a 3-channel tensor lives in 4)."""
    c = t.shape[1]
    buf = torch.zeros(t.shape[0], t.shape[2], t.shape[3], -(-c // 4) * 4, device="cuda")
    buf[..., :c] = nhwc(t)
    return buf[..., :c]


def nchw(t):
    return t.permute(0, 3, 1, 2).double().cpu()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale


def lrelu(x, s):
    return torch.where(x > 0, x, x * s)


def run_pair(N, H, W, Ca, Cb, Co, terms=3, bias=True, slope_pre=1.0, res=False, mask=False, two=False, dgrad=False,
             family="unit", ingroup=True, reference=False):
    """Both routes on one set of operands.  ingroup: the route wino_tile 0 is expected to take (False: the grid split, as the
    parent).  family 'ramp': input channel c is scaled by 2^(40 c / Ci), so the two K groups end on reference exponents 20
    binades apart and the online rescale runs in the upper group only."""
    from refid_amd import ops
    Ci = Ca + Cb
    x = rnd(N, Ci, H, W, seed=1)
    if family == "ramp":
        x = x * torch.exp2(torch.floor(40.0 * torch.arange(Ci, dtype=torch.float64) / Ci)).view(1, Ci, 1, 1)
    # forward: weights (Co, Ci); input gradient: the conv's weights are (Ci, Co) and the packing flips / transposes them
    w = rnd(Ci, Co, 3, 3, seed=3, scale=1.0 / np.sqrt(Ci * 9)) if dgrad else rnd(Co, Ci, 3, 3, seed=3, scale=1.0 / np.sqrt(Ci * 9))
    b = rnd(Co, seed=4) if bias else None
    r = rnd(N, Co, H, W, seed=5) if res else None
    m = rnd(N, Co, H, W, seed=6) if mask else None
    a2 = rnd(N, Co, H, W, seed=7) if two else None
    role = ops.ROLE_WINO_DGRAD if dgrad else ops.ROLE_WINO_FWD
    wp = ops.pack_conv_weights_wino6(w.float().cuda(), role, Ci if dgrad else Co, Co if dgrad else Ci, terms=terms)
    xd = nhwc(x)
    xa = xd[..., :Ca].contiguous()
    xb = xd[..., Ca:].contiguous() if Cb else None
    Cop = -(-Co // 4) * 4
    dev = xd.device
    ws = ops._workspace(1 << 20, dev, "conv")
    outs = {}
    for tile in (0, PARENT):
        ops.WINO_TILE = tile
        ws.fill_(SENTINEL)
        outbuf = torch.full((N, H, W, Cop), 7.0, device="cuda")
        out2buf = torch.full((N, H, W, Cop), 9.0, device="cuda") if two else None
        out = outbuf[..., :Co]
        ops.conv2d(xa, wp, out, kh=3, kw=3, stride=1, pad=1, cout=Co, cout_pad=-(-Co // 64) * 64, algo=5, terms=terms,
                   in_b=xb, bias=b.float().cuda() if bias else None, res=nhwc_quads(r) if res else None,
                   mask=nhwc_quads(m) if mask else None, slope_pre=slope_pre, slope_mask=0.3,
                   add2=nhwc_quads(a2) if two else None, out2=out2buf[..., :Co] if two else None)
        torch.cuda.synchronize()
        assert ops._workspace(1 << 20, dev, "conv") is ws
        untouched = bool((ws == SENTINEL).all())
        # routing: the in-group form never touches the workspace, the grid split writes its partial outputs there
        assert untouched == (ingroup and tile == 0), (tile, untouched)
        outs[tile] = (outbuf, out2buf)
    assert torch.equal(outs[0][0], outs[PARENT][0])
    if two:
        assert torch.equal(outs[0][1], outs[PARENT][1])
    if Cop != Co:
        assert float(outs[0][0][..., Co:].min()) == 7.0 and float(outs[0][0][..., Co:].max()) == 7.0
    if reference:
        wf = w.flip(2, 3).transpose(0, 1) if dgrad else w
        ref = lrelu(F.conv2d(x, wf, b, 1, 1), slope_pre)
        if res:
            ref = ref + r
        if mask:
            ref = ref * torch.where(m > 0, 1.0, 0.3)
        np.testing.assert_allclose(nchw(outs[0][0][..., :Co]).numpy(), ref.numpy(), rtol=RTOL, atol=ATOL)
        if two:
            np.testing.assert_allclose(nchw(outs[0][1][..., :Co]).numpy(), (ref + a2).numpy(), rtol=RTOL, atol=ATOL)


@pytest.fixture(autouse=True)
def _routing_switches(monkeypatch):
    from refid_amd import ops
    monkeypatch.setattr(ops, "WINO_TILE", 0)
    monkeypatch.setattr(ops, "WINO_SPLIT", 2)          # split decided by the total grid (the default policy)
    monkeypatch.setattr(ops, "DESC_CACHE", False)
    monkeypatch.setattr(ops, "PROFILE", None)


# (Ca, Cb): even halves on the small-grid 32-channel tile, 5 + 4 chunks, a partial last chunk, a source switch at the group
# boundary, 5 + 5 chunks; Cout: one full 64-channel tile, two tiles (the second half empty), a ragged tile
@pytest.mark.parametrize("cin", [(128, 0), (144, 0), (132, 0), (64, 64), (160, 0)])
@pytest.mark.parametrize("cout", [64, 96, 40])
def test_ingroup_split_geometries(cin, cout):
    run_pair(1, 8, 32, cin[0], cin[1], cout, reference=(cout == 64))


@pytest.mark.parametrize("terms", [3, 1, 0])
@pytest.mark.parametrize("cfg", [(1, 8, 32, 144, 0, 64), (1, 8, 32, 128, 0, 64), (1, 7, 33, 176, 0, 72), (2, 4, 30, 128, 0, 20)])
def test_ingroup_split_products_and_ragged_tiles(cfg, terms):
    """The three product forms (three fp16, one fp16, six bf16); ragged rows / columns with dead rows in the second Winograd
    tile row; the 32-output-channel form (cout 20, a ragged quad) with two samples."""
    run_pair(*cfg, terms=terms, reference=(terms != 1))     # (terms 1 is a reduced-precision form: equality only)


@pytest.mark.parametrize("cfg", [(144, 64), (128, 64), (128, 3)])
def test_ingroup_split_epilogues(cfg):
    """bias / none, LeakyReLU, residual, activation mask, second output -- on the 64-channel tile, the small-grid 32-channel
    tile and the scalar epilogue of a thin output (3 channels in a 4-channel buffer)."""
    ci, co = cfg
    run_pair(1, 8, 32, ci, 0, co, bias=False, reference=True)
    run_pair(1, 8, 32, ci, 0, co, slope_pre=0.1, reference=True)
    run_pair(1, 8, 32, ci, 0, co, res=True, reference=True)
    run_pair(1, 8, 32, ci, 0, co, bias=False, res=True, mask=True, reference=True)
    run_pair(1, 8, 32, ci, 0, co, slope_pre=0.1, res=True, mask=True, two=True, reference=True)


@pytest.mark.parametrize("terms", [3, 1])
@pytest.mark.parametrize("cfg", [(1, 8, 32, 144, 0, 64), (1, 8, 32, 64, 64, 64), (1, 9, 33, 160, 0, 40)])
def test_ingroup_split_ramp_along_k(cfg, terms):
    """2^40 ramp along K: the two groups end on different reference exponents and un-scale by different powers of two."""
    run_pair(*cfg, terms=terms, family="ramp", res=True, mask=True)


@pytest.mark.parametrize("terms", [3, 0])
@pytest.mark.parametrize("cfg", [(1, 8, 32, 144, 64), (1, 8, 32, 128, 64), (1, 6, 40, 160, 96)])
def test_ingroup_split_input_gradient(cfg, terms):
    """The input gradient's call: flipped / transposed packing, residual gradient added, activation-derivative mask."""
    N, H, W, Co, Ci = cfg                                   # the call's "input channels" are the conv's output channels
    run_pair(N, H, W, Co, 0, Ci, terms=terms, dgrad=True, bias=False, res=True, mask=True, reference=True)


def test_four_k_ranges_keep_the_grid_split():
    """ks == 4 (16 chunks): still two launches through the workspace, the parent's bits."""
    run_pair(1, 8, 32, 256, 0, 64, ingroup=False, reference=True)
    run_pair(1, 8, 32, 256, 0, 64, ingroup=False, family="ramp", res=True)
