"""CPU checks of tests/nongemm_ref.py, the float64 reference of test_hip_nongemm_precision.py.

  1  every hand-written float64 formula agrees with torch (float64 ops and autograd) to 1e-12 of its scale: a wrong reference
     cannot hide a wrong kernel;
  2  the float32 restatement of every kernel meets its bar on every case and family of the GPU file, and every derived constant
     IS the next power of two at or above twice the restatement's worst ratio (nongemm_ref.CONST lists both);
  3  teeth: the float32 HIN restatement with the one-pass variance E[x^2] - m^2 misses the HIN bar on `offset32`.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nongemm_ref as R

TIGHT = 1e-12 / R.EPS            # 1e-12 of scale, in check()'s units of 2^-24


def t(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=grad)


def nchw(a, grad=False):
    return t(np.ascontiguousarray(np.moveaxis(a, -1, 1)), grad)


def nhwc(g):
    return np.moveaxis(g.detach().numpy(), 1, -1)


def close(got, ref_S, what):
    ref, S = ref_S
    R.check(got, ref, S, TIGHT, what)


# ---- (1) the float64 formulas against torch ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", R.NORM_FAMILIES)
@pytest.mark.parametrize("cfg", [(2, 5, 7, 8, 4), (2, 6, 5, 8, 8), (1, 4, 4, 8, 0)])
def test_hin_reference_against_torch(cfg, fam):
    N, H, W, C, ch = cfg
    x = R.family(fam, (N, H, W, C), 1)
    gamma, beta = (R.fp32(1 + 0.3 * R.uni(2, ch)), R.fp32(R.uni(3, ch))) if ch else (None, None)
    g, dg0, db0 = R.fp32(R.uni(4, N, H, W, C)), R.fp32(R.uni(5, ch)), R.fp32(R.uni(6, ch))
    xt = nchw(x, True)
    gt_, bt = (t(gamma, True), t(beta, True)) if ch else (None, None)
    y = torch.cat([F.instance_norm(xt[:, :ch], weight=gt_, bias=bt, eps=R.HIN_EPS), xt[:, ch:]], 1) if ch else xt
    out = F.leaky_relu(y, R.SLOPE)
    out.backward(nchw(g))
    ref, S = R.hin_fwd(x, gamma, beta, ch)
    close(nhwc(out), (ref, S), "hin forward")
    B = R.hin_bwd(g, ref, x, gamma, ch, dg0, db0)
    close(nhwc(xt.grad), B["gx"], "hin gx")
    if ch:
        close(dg0 + gt_.grad.numpy(), B["dgamma"], "hin dgamma")
        close(db0 + bt.grad.numpy(), B["dbeta"], "hin dbeta")


def test_fac_reference_against_torch():
    shape = (2, 3, 5, 8)
    feat, filt, g = R.family("spread", shape, 1), R.family("uniform", (2, 3, 5, 16), 2), R.fp32(R.uni(3, *shape))
    ft, fl = t(feat, True), t(filt, True)
    out = ft * fl[..., :8] + fl[..., 8:]
    out.backward(t(g))
    close(out.detach().numpy(), R.fac_fwd(feat, filt), "fac forward")
    B = R.fac_bwd(g, feat, filt)
    close(ft.grad.numpy(), B["gfeat"], "fac gfeat")
    close(fl.grad.numpy(), B["gfilt"], "fac gfilt")


@pytest.mark.parametrize("fam", R.NORM_FAMILIES)
@pytest.mark.parametrize("res", [False, True])
def test_layernorm_reference_against_torch(fam, res):
    shape = (2, 3, 5, 16)
    x, w, b, g, r, dw0, db0 = R.ln_inputs(shape, fam)
    xt, wt, bt = t(x, True), t(w, True), t(b, True)
    mu = xt.mean(-1, keepdim=True)
    var = ((xt - mu) ** 2).mean(-1, keepdim=True)
    out = (xt - mu) / torch.sqrt(var + R.LN_EPS) * wt + bt
    out.backward(t(g))
    close(out.detach().numpy(), R.ln_fwd(x, w, b), "layernorm forward")
    B = R.ln_bwd(g, x, w, r if res else None, dw0, db0)
    close(xt.grad.numpy() + (r if res else 0.0), B["gx"], "layernorm gx")
    close(dw0 + wt.grad.numpy(), B["dw"], "layernorm dw")
    close(db0 + bt.grad.numpy(), B["db"], "layernorm db")


@pytest.mark.parametrize("shape", [(2, 5, 6, 8), (1, 1, 7, 4), (1, 5, 1, 4)])
def test_depthwise_reference_against_torch(shape):
    x, w, b, gd, dw0, db0 = R.dw_inputs(shape, "uniform")
    C = shape[-1]
    xt, wt, bt = nchw(x, True), t(w.reshape(C, 1, 3, 3), True), t(b, True)
    pre = F.conv2d(xt, wt, bt, padding=1, groups=C)
    act = F.gelu(pre)
    Fw = R.dw_fwd(x, w, b, 16.0)
    close(nhwc(pre), Fw["pre"], "depthwise pre")
    close(nhwc(act), Fw["act"], "depthwise act")
    close(act.sum((2, 3)).detach().numpy(), Fw["pool"], "depthwise pool")
    pre.backward(nchw(gd))
    B = R.dw_bwd(gd, x, w, dw0, db0)
    close(nhwc(xt.grad), B["gin"], "depthwise gin")
    close(dw0 + wt.grad.numpy().reshape(C, 9), B["dw"], "depthwise dw")
    close(db0 + bt.grad.numpy(), B["db"], "depthwise db")


def test_colsum_and_gs_reduce_references_against_torch():
    g, db0 = R.fp32(R.uni(1, 2, 3, 5, 8)), R.fp32(R.uni(2, 8))
    close(db0 + t(g).sum((0, 1, 2)).numpy(), R.colsum(g, db0), "colsum")
    gxs, xi, xe = R.fp32(R.uni(3, 2, 3, 5, 16)), R.fp32(R.uni(4, 2, 3, 5, 8)), R.fp32(R.uni(5, 2, 3, 5, 8))
    s = t(np.ones((2, 1, 1, 8)), True)                     # gs is the gradient of sum(gxs * [xi s | xe s]) w.r.t. s
    (t(gxs) * torch.cat([t(xi) * s, t(xe) * s], -1)).sum().backward()
    close(s.grad.numpy().reshape(2, 8), R.gs_reduce(gxs, xi, xe), "gs_reduce")


@pytest.mark.parametrize("C,parts", [(16, 3), (64, 17)])
def test_squeeze_excite_reference_against_torch(C, parts):
    pool, inv_hw, W1, b1, W2, b2 = R.se_inputs(C, parts)
    Fw = R.se_fwd(pool, inv_hw, W1, b1, W2, b2)
    P = [t(a, True) for a in (W1, b1, W2, b2)]
    m = (t(pool).sum(1) * inv_hw).requires_grad_(True)
    z1 = F.relu(m @ P[0].t() + P[1])
    s = torch.sigmoid(z1 @ P[2].t() + P[3])
    for k, v in (("m", m), ("z1", z1), ("s", s)):
        assert float(np.abs(v.detach().numpy() - Fw[k][0]).max()) <= 1e-14, k
    gs = R.fp32(R.uni(9, 3, C))
    s.backward(t(gs))
    z = [R.fp32(R.uni(10 + i, *a.shape)) for i, a in enumerate((W1, b1, W2, b2))]
    B = R.se_bwd(gs, Fw["s"][0], Fw["z1"][0], Fw["m"][0], W1, W2, *z)
    close(m.grad.numpy(), B["gm"], "se gm")
    for k, i in (("dW1", 0), ("db1", 1), ("dW2", 2), ("db2", 3)):
        close(z[i] + P[i].grad.numpy(), B[k], "se " + k)


@pytest.mark.parametrize("gscale", [1.0, R.f32s(1 / 3)])
def test_loss_references_against_torch(gscale):
    pred, gt = R.loss_inputs(3076)
    pt = t(pred, True)
    loss = torch.sqrt((pt - t(gt)) ** 2 + R.CHARB_EPS).sum()
    (loss * gscale).backward()
    ref = R.charbonnier(pred, gt, gscale)
    close(loss.item(), ref["loss"], "charbonnier sum")
    close(pt.grad.numpy(), ref["grad"], "charbonnier gradient")
    assert float(ref["grad"][0][0]) == 0.0 and pred[0] == gt[0]                 # d = 0: gradient 0, term sqrt(eps)
    p2, g2 = (a.reshape(4, 769) for a in (pred, gt))
    p2 = p2.copy()
    p2[1] = g2[1]
    pt = t(p2, True)
    mse = ((pt - t(g2)) ** 2).mean(1)
    loss = 0.5 * 10.0 / math.log(10.0) * torch.log(mse + 1e-8).mean()
    loss.backward()
    ref = R.psnr_loss(p2, g2, 0.5)
    close(loss.item(), ref["loss"], "psnr loss")
    close((mse * 769).detach().numpy(), ref["sq"], "psnr sq")
    close(pt.grad.numpy(), ref["grad"], "psnr gradient")
    g = R.fp32(R.uni(1, 64))
    close(float((t(g) ** 2).sum()), R.sqnorm(g), "sqnorm")


@pytest.mark.parametrize("regime", ["clip", "noclip", "off"])
def test_adamw_reference_against_torch_optim(regime):
    """clip_grad_norm_ + torch.optim.AdamW in float64, three steps, against clip_adamw() with exact (float64) bias corrections."""
    h = R.ADAMW_HYPER
    p0 = R.fp32(R.uni(1, 64) + 0.25)
    pt = t(p0, True)
    opt = torch.optim.AdamW([pt], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"])
    p, m, v = p0, np.zeros(64), np.zeros(64)
    for step in (1, 2, 3):
        g = R.fp32(R.uni(10 + step, 64))
        norm = math.sqrt(float((g * g).sum()))
        max_norm = {"clip": 0.01 * norm, "noclip": 4 * norm, "off": 0.0}[regime]
        pt.grad = t(g)
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([pt], max_norm)
        opt.step()
        r = R.clip_adamw(p, g, m, v, norm * norm, max_norm=max_norm, gscale=1.0, lr=h["lr"], bc1=1 - h["b1"] ** step,
                         bc2s=math.sqrt(1 - h["b2"] ** step), b1=h["b1"], b2=h["b2"], eps=h["eps"], wd=h["wd"])
        assert float(np.abs(pt.detach().numpy() - r["p"][0]).max()) <= 1e-13 * float(r["p"][1].max()), step
        p, m, v = r["p"][0], r["m"][0], r["v"][0]
        st = opt.state[pt]
        assert float(np.abs(st["exp_avg"].numpy() - m).max()) <= 1e-13 * float(r["m"][1].max())
        assert float(np.abs(st["exp_avg_sq"].numpy() - v).max()) <= 1e-13 * float(r["v"][1].max())


# ---- (2) the float32 restatements meet the bars; the constants follow the rule -------------------------------------------------
BE = R.Float32Backend()
WORST = {}


def _run(name):
    w = WORST.setdefault(name, {})
    if name == "hin":
        for cfg, fams in R.HIN_CASES:
            for fam in fams:
                R.compare_hin(BE, cfg, fam, w)
    elif name == "fac":
        for s, fams in R.FAC_CASES:
            for fam in fams:
                R.compare_fac(BE, s, fam, w)
    elif name == "ln":
        for s, fams in R.LN_FWD_CASES:
            for fam in fams:
                R.compare_ln_fwd(BE, s, fam, w)
        for s, fams in R.LN_BWD_CASES:
            for fam in fams:
                for mode in ("none", "res", "alias"):
                    R.compare_ln_bwd(BE, s, fam, mode, w)
    elif name == "dw":
        for s, fams in R.DW_CASES:
            for fam in fams:
                R.compare_dw(BE, s, fam, w)
    elif name == "reductions":
        for c in R.COLSUM_CASES:
            R.compare_colsum(BE, c, w)
        for s in R.GS_CASES:
            R.compare_gs(BE, s, w)
    elif name == "se":
        for C, parts in R.SE_CASES:
            R.compare_se(BE, C, parts, w)
    elif name == "loss":
        for n in R.LOSS_COUNTS:
            for gs in (1.0, R.f32s(1 / 3)):
                for want in (True, False):
                    R.compare_charbonnier(BE, n, gs, want, w)
            R.compare_sqnorm(BE, n, w)
        for c in R.PSNR_CASES:
            R.compare_psnr(BE, c, w)
    else:
        assert name == "adamw", name
        for c in R.ADAMW_CASES:
            R.compare_adamw(BE, c, w)
    return w


@pytest.mark.parametrize("name", ["hin", "fac", "ln", "dw", "reductions", "se", "loss", "adamw"])
def test_float32_restatement_meets_the_bars_and_fixes_the_constants(name):
    """Every case and family of the GPU file through the float32 restatement and the same check() with the same constants; then
    the rule: a derived constant equals the next power of two at or above twice the worst ratio measured here."""
    w = _run(name)
    assert w, name
    for k, r in sorted(w.items()):
        print(f"{k}: float32 restatement worst err / (2^-24 S) = {r:.3g}, constant {R.CONST[k]}")
        if k not in R.NOT_DERIVED:
            assert R.CONST[k] == R.next_pow2_of_twice(r), (k, r, R.CONST[k])


def test_every_constant_is_covered():
    keys = set()
    for name in ["hin", "fac", "ln", "dw", "reductions", "se", "loss", "adamw"]:
        keys |= set(WORST.get(name) or _run(name))
    assert keys == set(R.CONST), keys ^ set(R.CONST)


# ---- (3) teeth ---------------------------------------------------------------------------------------------------------------
def test_one_pass_variance_would_miss_the_hin_bound():
    """The data has teeth: the float32 restatement with the variance as E[x^2] - m^2, accumulated the way part_sums does (fp32 per
    thread, tree over the rows, parts in double), misses the HIN bar on offset32 at (1, 64, 64, 8): worst err / (2^-24 S) = 22.1
    against the constant 8, a factor 2.8 (the two-pass form: 0.42 on the same data)."""
    x = R.family("offset32", (1, 64, 64, 8), 11)
    gamma, beta = R.fp32(1.0 + 0.3 * R.uni(12, 8)), R.fp32(0.5 * R.uni(13, 8))
    ref, S = R.hin_fwd(x, gamma, beta, 8)
    two, _ = R.hin_fwd32(x, gamma, beta, 8)
    assert R.check(two, ref, S, R.CONST["hin_fwd/out"], "two-pass out") < 1.0
    one, _ = R.hin_fwd32(x, gamma, beta, 8, one_pass=True)
    with pytest.raises(AssertionError, match="one-pass out"):
        R.check(one, ref, S, R.CONST["hin_fwd/out"], "one-pass out")
    assert R.check(one, ref, S, float("inf"), "one-pass out") > 2.5 * R.CONST["hin_fwd/out"]
