"""The conv tiles' fused epilogue, separated from their GEMMs and held per element.

    out = mask(post(pre(acc + bias) + res)),   out2 = out + add2          (refid_conv_desc)

Every case runs the same tile twice on the same inputs, weights and split policy: RAW (no bias, slopes 1, no residual / mask /
second output) returns the tile's own fp32 accumulators -- the kernels are deterministic, so these are the very values the FULL
call (bias, slope_pre 0.1, residual, slope_post 0.2, mask with slope_mask 0.3, second output where the tile has one) starts
from.  In float64, from the fp32 tensors:

    s1 = raw + b    p = lrelu(s1, .1)    s2 = p + r    q = lrelu(s2, .2)    o = q * f

Each kernel step is one fp32 rounding and every slope / factor is <= 1 in magnitude, so the fused result lies within
2^-24 (|s1| + |p| + |s2| + |q| + |o|) of o (rounding cannot move s1 or s2 across zero: the kinks are safe); the test allows twice
that for a contracted multiply-add.  out2 is the fp32 sum out + add2 bit for bit, and nothing past Cout is written in either
output buffer.  (maskMode 1 and the pointwise tile's EGACA fusions: tests/test_hip_pw_precision.py.)"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
SLOPES = (0.1, 0.2, 0.3)          # pre, post, mask


def _u(g, *shape):
    return torch.rand(*shape, generator=g, device="cuda") * 2 - 1


def _padded(g, N, H, W, Co, random=False):
    """An NHWC tensor of Co channels as a view of a buffer with spare channels behind them (Co = 6 -> pitch 8, 64 -> 68)."""
    pitch = -(-Co // 4) * 4 if Co % 4 else Co + 4
    buf = _u(g, N, H, W, pitch) if random else torch.full((N, H, W, pitch), SENTINEL, device="cuda")
    return buf, buf[..., :Co]


def _pack(ops, kind, terms, w, Co, Ci):
    """(packed weights, conv2d's geometry / tile keywords)"""
    wd = w.cuda()
    if kind == "direct3":
        kc, bn = ops.conv_kc(3, 3, 1), ops.conv_bn(3, 3, 1, 0, Co)
        return ops.pack_conv_weights(wd, ops.ROLE_FWD, bn, kc, 3, 3, Co, Ci), dict(kh=3, kw=3, pad=1, cout_pad=-(-Co // bn) * bn, algo=0)
    if kind == "direct_down":
        kc, bn = ops.conv_kc(4, 4, 2), ops.conv_bn(4, 4, 2, 0, Co)
        return (ops.pack_conv_weights(wd, ops.ROLE_FWD, bn, kc, 4, 4, Co, Ci),
                dict(kh=4, kw=4, stride=2, pad=1, cout_pad=-(-Co // bn) * bn, algo=0))
    if kind == "wino":
        return (ops.pack_conv_weights(wd, ops.ROLE_WINO_FWD, 64, 8, 3, 3, Co, Ci),
                dict(kh=3, kw=3, pad=1, cout_pad=-(-Co // 64) * 64, algo=1))
    if kind == "wino6":
        return (ops.pack_conv_weights_wino6(wd, ops.ROLE_WINO_FWD, Co, Ci, terms=terms),
                dict(kh=3, kw=3, pad=1, cout_pad=-(-Co // 64) * 64, algo=5, terms=terms))
    if kind == "split3":
        bn = ops.conv_bn(3, 3, 1, 0, Co)
        return (ops.pack_conv_weights_split(wd, ops.ROLE_FWD, bn, 3, 3, Co, Ci, planes=3),
                dict(kh=3, kw=3, pad=1, cout_pad=-(-Co // bn) * bn, algo=4, terms=terms))
    if kind == "split_down":
        bn = ops.conv_bn(4, 4, 2, 0, Co)
        return (ops.pack_conv_weights_split(wd, ops.ROLE_FWD, bn, 4, 4, Co, Ci, planes=3 if terms == 6 else 2, f16=terms == 19),
                dict(kh=4, kw=4, stride=2, pad=1, cout_pad=-(-Co // bn) * bn, algo=4, terms=terms))
    if kind == "split_down_dgrad":      # w is the forward weight (O = Ci of this call, I = Co of this call)
        bn = ops.conv_bn(4, 4, 2, 2, Co)
        return (ops.pack_conv_weights_split(wd, ops.ROLE_DOWN_DGRAD, bn, 4, 4, Ci, Co, planes=3),
                dict(kh=4, kw=4, stride=2, pad=1, mode=2, cout_pad=-(-Co // bn) * bn, algo=4, terms=terms))
    if kind == "pw":
        return ops.pack_conv_weights(wd, ops.ROLE_FWD, 32, 8, 1, 1, Co, Ci), dict(kh=1, kw=1, cout_pad=-(-Co // 32) * 32, algo=3)
    assert kind == "pw_shuffle"         # ConvTranspose2d(2,2): Co real channels, 4 Co GEMM columns
    return (ops.pack_conv_weights(wd, ops.ROLE_CONVT, 32, 8, 2, 2, Co, Ci),
            dict(kh=1, kw=1, mode=1, cout_pad=-(-4 * Co // 32) * 32, algo=3))


def _weight_shape(kind, Co, Ci):
    k = {"direct3": 3, "wino": 3, "wino6": 3, "split3": 3, "direct_down": 4, "split_down": 4, "pw": 1}.get(kind)
    if kind == "split_down_dgrad":
        return (Ci, Co, 4, 4)
    if kind == "pw_shuffle":
        return (Ci, Co, 2, 2)
    return (Co, Ci, k, k)


# (id, kind, terms, (N, H, W, Ca, Cb, Co), split_k, must_split, second output, mask)
def _cases():
    S = (1, 9, 33)                  # one ragged row tile, a one-pixel second column tile
    out = []

    def add(name, kind, terms, shape, split=2, must_split=False, two=True, mask=True):
        out.append(pytest.param(kind, terms, shape, split, must_split, two, mask, id=name))

    add("direct3-64", "direct3", 0, S + (16, 0, 64))
    add("direct3-6", "direct3", 0, S + (16, 0, 6))              # first quad vector, second quad a two-channel tail
    add("direct-down-splitk", "direct_down", 0, (1, 16, 16, 64, 0, 64), split=1, must_split=True)
    for co in (64, 32, 6):
        add(f"wino-{co}", "wino", 0, S + (16, 0, co))
    for co in (64, 6):
        add(f"wino-splitk-{co}", "wino", 0, (1, 8, 8, 256, 0, co), must_split=True)
    for t in (0, 3, 1):
        for co in (64, 32, 6):
            add(f"wino6-t{t}-{co}", "wino6", t, S + (32, 0, co))
        # (under the split policies the small-grid switch gives 64 channels at this size to the 32-channel form: policy 0
        #  reaches the 64-channel form's fused epilogue)
        add(f"wino6-t{t}-64-wide", "wino6", t, S + (32, 0, 64), split=0)
        add(f"wino6-t{t}-two-sources", "wino6", t, S + (16, 16, 64))
        for co in (64, 6):
            add(f"wino6-t{t}-splitk-{co}", "wino6", t, (1, 8, 8, 256, 0, co), must_split=True)
    add("split3", "split3", 6, S + (16, 0, 64))
    add("split-down", "split_down", 6, (1, 18, 66, 16, 0, 64))
    add("split-down-dgrad", "split_down_dgrad", 6, S + (64, 0, 16))     # stores at (2y + py, 2x + px)
    add("split-down-fp16", "split_down", 19, (1, 18, 66, 16, 0, 64))
    add("pw-64", "pw", 0, S + (16, 0, 64))
    add("pw-38-scalar", "pw", 0, S + (16, 0, 38), two=False)     # Cout % 4: the scalar epilogue (it has no second output)
    add("pw-shuffle", "pw_shuffle", 0, (1, 8, 16, 64, 0, 32), two=False, mask=False)
    return out


def _workspace_bytes(lib, a, b, kw, cout, split):
    from refid_amd import _lib
    d = _lib.ConvDesc()
    d.n, d.h, d.w = a.shape[0], a.shape[1], a.shape[2]
    stride = kw.get("stride", 1)
    d.ho, d.wo = (d.h // stride, d.w // stride) if kw.get("mode", 0) == 0 else (d.h, d.w)
    d.c_a, d.c_b, d.cout, d.cout_pad = a.shape[3], 0 if b is None else b.shape[3], cout, kw["cout_pad"]
    d.kh, d.kw, d.stride, d.pad, d.mode = kw["kh"], kw["kw"], stride, kw.get("pad", 0), kw.get("mode", 0)
    d.algo, d.split_k = kw["algo"], split
    return lib.refid_conv_workspace_bytes(C.byref(d))


@pytest.mark.parametrize("kind,terms,shape,split,must_split,two,mask", _cases())
def test_fused_epilogue_per_element(kind, terms, shape, split, must_split, two, mask):
    from refid_amd import ops, _lib
    N, H, W, Ca, Cb, Co = shape
    Ci = Ca + Cb
    g = torch.Generator(device="cuda").manual_seed(1 + sum(shape) + terms)
    w = _u(g, *_weight_shape(kind, Co, Ci)) * (1.0 / (Ci * 4) ** 0.5)
    wp, kw = _pack(ops, kind, terms, w, Co, Ci)
    a = _u(g, N, H, W, Ca)
    b = _u(g, N, H, W, Cb) if Cb else None
    gemm_cols = 4 * Co if kind == "pw_shuffle" else Co
    if kw.get("mode", 0):
        Ho, Wo = 2 * H, 2 * W
    else:
        Ho, Wo = (H // 2, W // 2) if kw.get("stride", 1) == 2 else (H, W)
    bias = _u(g, Co)
    _, res = _padded(g, N, Ho, Wo, Co, random=True)
    _, msk = _padded(g, N, Ho, Wo, Co, random=True)
    _, add2 = _padded(g, N, Ho, Wo, Co, random=True)
    res[_u(g, *res.shape) > 0.8] = 0.0                          # exact zeros: s2 = p, and mask == 0 takes the slope branch
    msk[_u(g, *msk.shape) > 0.8] = 0.0
    assert int((res == 0).sum()) > 0 and int((msk == 0).sum()) > 0
    rawbuf, raw = _padded(g, N, Ho, Wo, Co)
    outbuf, out = _padded(g, N, Ho, Wo, Co)
    out2buf, out2 = _padded(g, N, Ho, Wo, Co)

    old, ops.WINO_SPLIT = ops.WINO_SPLIT, split
    try:
        if must_split:
            assert _workspace_bytes(_lib.lib(), a, b, kw, gemm_cols, split) > 0       # this shape takes the finishing kernel
        ops.conv2d(a, wp, raw, cout=gemm_cols, in_b=b, **kw)
        ops.conv2d(a, wp, out, cout=gemm_cols, in_b=b, bias=bias, res=res, mask=msk if mask else None,
                   slope_pre=SLOPES[0], slope_post=SLOPES[1], slope_mask=SLOPES[2],
                   add2=add2 if two else None, out2=out2 if two else None, **kw)
    finally:
        ops.WINO_SPLIT = old
    torch.cuda.synchronize()

    sl = [float(torch.tensor(s, dtype=torch.float32)) for s in SLOPES]       # the slopes as the kernels receive them
    s1 = raw.double() + bias.double()
    p = torch.where(s1 > 0, s1, s1 * sl[0])
    s2 = p + res.double()
    q = torch.where(s2 > 0, s2, s2 * sl[1])
    f = torch.where(msk.double() > 0, 1.0, sl[2]) if mask else torch.ones_like(q)
    o = q * f
    bound = 2.0 ** -23 * (s1.abs() + p.abs() + s2.abs() + q.abs() + o.abs())
    err = (out.double() - o).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"epilogue {kind} terms={terms} {shape}: max |out - o| / bound = {worst:.3f}, max err = {float(err.max()):.3e}")
    assert bool((err <= bound).all()), (worst, float(err.max()))
    assert float(raw.abs().max()) > 0.05                         # the accumulators are a convolution's, not zeros
    if two:
        assert torch.equal(out2, out + add2)
    # nothing past Cout, in any buffer (the second buffer is untouched altogether where the tile has no second output)
    assert float(rawbuf[..., Co:].min()) == SENTINEL and float(rawbuf[..., Co:].max()) == SENTINEL
    assert float(outbuf[..., Co:].min()) == SENTINEL and float(outbuf[..., Co:].max()) == SENTINEL
    pad2 = out2buf[..., Co:] if two else out2buf
    assert float(pad2.min()) == SENTINEL and float(pad2.max()) == SENTINEL
