"""float64 and float32 restatements of the kernels that are not GEMMs: HIN + LeakyReLU and FAC_bias (csrc/evhinet.hip), LayerNorm2d,
depthwise 3x3 + GELU, colsum, gs_reduce and squeeze-excite (csrc/egaca.hip), Charbonnier, PSNRLoss, squared norm and clip + AdamW
(csrc/train.hip).  Shared by test_nongemm_ref_host.py (CPU) and test_hip_nongemm_precision.py (GPU).

Everything is numpy on NHWC arrays.  The float64 functions are written out by hand (no autograd) so that every value comes with a
per-element error scale S; the gate is |got - ref| <= c 2^-24 S for every element (check()).  S is
  * for a sum, the sum of the absolute values of its terms (plus the starting value of an accumulating destination);
  * for a normalisation, T = |gamma| rstd (|x| + mean |x|) + |beta|, the scale test_hip_pw_precision.ln_ref uses: it dominates
    the value and carries the error of the mean; whatever consumes a normalised value x^ propagates Tx = rstd (|x| + mean |x|);
  * for AdamW, |p| + |update| for p and the sum of |terms| for m and v.
The float32 functions restate the same formulas in numpy float32.  Their sums are "strided": a fixed number of lanes, each adding
its terms in sequence, then a pairwise tree over the lanes -- the structure of every reduction kernel here (a thread's pixels in
order, then a fixed tree), though not bit for bit the kernel's order, which is not part of any contract.  For HIN the strided sum
follows part_sums: pixel chunks ("parts"), R = 256 / Q rows of threads per part, a tree over the rows, the parts added in double.

All inputs are float64 arrays that hold fp32 numbers (fp32()); scalars (eps, slope, lr, ...) are fp32 numbers too (f32s()).
"""
import math

import numpy as np

EPS = 2.0 ** -24
F32 = np.float32
HIN_EPS = float(F32(1e-5))
LN_EPS = float(F32(1e-6))
CHARB_EPS = float(F32(1e-12))
SLOPE = float(F32(0.2))
GELU_LIP = 1.13              # the project's constants (test_hip_pw_precision.py)
C_GELU = 8.0
SIG_MARGIN = 8.0
FAMILIES = ["uniform", "offset8", "offset32", "spread", "hot-pixel"]
NORM_FAMILIES = FAMILIES + ["const-channel"]


def fp32(a):
    return np.asarray(a, dtype=np.float64).astype(F32).astype(np.float64)


def f32s(v):
    return float(F32(v))


def check(got, ref, S, c, what):
    """Every element within c 2^-24 S; NaN / inf fail.  Returns the worst err / (2^-24 S)."""
    got, ref, S = (np.asarray(v, dtype=np.float64) for v in (got, ref, S))
    assert got.shape == ref.shape == S.shape, (what, got.shape, ref.shape, S.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(S > 0, err / (EPS * S), np.where(err > 0, np.inf, 0.0))
    ratio = np.where(np.isfinite(err), ratio, np.inf)
    worst = float(ratio.max()) if ratio.size else 0.0
    bad = ~(ratio <= c)
    if bad.any():
        i = np.unravel_index(int(np.flatnonzero(bad.reshape(-1))[0]), err.shape) if err.ndim else ()
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.size} elements outside c 2^-24 S (c = {c}); first at {tuple(int(v) for v in i)}: "
                             f"got {float(got[i]):.9e}, float64 {float(ref[i]):.9e}, error {float(err[i]):.3e}, S {float(S[i]):.3e}; "
                             f"worst error / (2^-24 S) = {worst:.3g}")
    return worst


def next_pow2_of_twice(r):
    """The rule for a constant: the next power of two at or above twice the float32 restatement's worst ratio."""
    return 2.0 ** math.ceil(math.log2(max(2.0 * r, 1.0)))


# ---- data ------------------------------------------------------------------------------------------------------------------
def uni(seed, *shape):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=shape)


def family(kind, shape, seed):
    """(N, H, W, C) float64 of fp32 numbers.  sigma = 3^-1/2, the standard deviation of a channel of `uniform`."""
    N, H, W, C = shape
    x = uni(seed, N, H, W, C)
    sd = 1.0 / math.sqrt(3.0)
    if kind == "offset8":
        x = x + 8 * sd
    elif kind == "offset32":
        x = x + 32 * sd
    elif kind == "spread":
        x = x * np.exp2(np.linspace(-10.0, 10.0, C))
    elif kind == "hot-pixel":
        x[:, 0, 0, :] = 1e3 * sd * np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
    elif kind == "const-channel":
        x[..., 1::4] = 100.0
    else:
        assert kind == "uniform", kind
    return fp32(x)


# ---- float32 sums ------------------------------------------------------------------------------------------------------------
def tree32(a):
    """Pairwise tree over axis 0 (length a power of two), float32."""
    a = np.asarray(a, dtype=F32)
    while a.shape[0] > 1:
        h = a.shape[0] // 2
        a = a[:h] + a[h:]
    return a[0]


def strided_sum32(t, lanes):
    """Sum over axis 0 in float32: `lanes` (a power of two) lanes add their terms i, i + lanes, ... in sequence, then a tree."""
    t = np.asarray(t, dtype=F32)
    n = t.shape[0]
    k = -(-n // lanes)
    pad = np.zeros((k * lanes - n,) + t.shape[1:], dtype=F32)
    t = np.concatenate([t, pad], 0).reshape((k, lanes) + t.shape[1:])
    acc = np.zeros(t.shape[1:], dtype=F32)
    for i in range(k):
        acc = acc + t[i]
    assert acc.dtype == F32
    return tree32(acc)


def lrelu(v, slope):
    return np.where(v > 0, v, v * slope)


# ---- HIN + LeakyReLU ---------------------------------------------------------------------------------------------------------
def hin_stats(x, ch, eps=HIN_EPS):
    xs = x[..., :ch]
    m = xs.mean((1, 2), keepdims=True)
    d = xs - m
    rstd = 1.0 / np.sqrt((d * d).mean((1, 2), keepdims=True) + eps)
    Tx = rstd * (np.abs(xs) + np.abs(xs).mean((1, 2), keepdims=True))
    return d * rstd, rstd, Tx


def hin_fwd(x, gamma, beta, ch, slope=SLOPE, eps=HIN_EPS):
    """(out, S): LeakyReLU([IN(x[..., :ch]) gamma + beta | x[..., ch:]]).  LeakyReLU is 1-Lipschitz: S is the pre-activation's."""
    pre, S = x.copy(), np.abs(x)
    if ch:
        xh, rstd, Tx = hin_stats(x, ch, eps)
        pre[..., :ch] = xh * gamma + beta
        S[..., :ch] = np.abs(gamma) * Tx + np.abs(beta)
    return lrelu(pre, slope), S


def hin_bwd(g, out, x, gamma, ch, dgamma0, dbeta0, slope=SLOPE, eps=HIN_EPS):
    """gx, dgamma, dbeta with their scales; the sign decisions are read from `out` (an input of the kernel)."""
    gy = g * np.where(out > 0, 1.0, slope)
    gx, Sgx = gy.copy(), np.abs(gy)
    if not ch:
        return dict(gx=(gx, Sgx))
    xh, rstd, Tx = hin_stats(x, ch, eps)
    gyc = gy[..., :ch]
    mean = lambda a: a.mean((1, 2), keepdims=True)                     # noqa: E731
    s1, s2 = mean(gyc), mean(gyc * xh)
    gx[..., :ch] = rstd * gamma * (gyc - s1 - xh * s2)
    Sgx[..., :ch] = rstd * np.abs(gamma) * (np.abs(gyc) + mean(np.abs(gyc)) + np.abs(xh) * mean(np.abs(gyc * xh))
                                            + Tx * np.abs(s2) + np.abs(xh) * mean(np.abs(gyc) * Tx))
    dg = dgamma0 + (gyc * xh).sum((0, 1, 2))
    Sdg = np.abs(dgamma0) + (np.abs(gyc) * Tx).sum((0, 1, 2))
    db = dbeta0 + gyc.sum((0, 1, 2))
    Sdb = np.abs(dbeta0) + np.abs(gyc).sum((0, 1, 2))
    return dict(gx=(gx, Sgx), dgamma=(dg, Sdg), dbeta=(db, Sdb))


def hin_parts(hw):
    return min(max(-(-hw // 1024), 1), 128)


def hin_part_sums32(a, Q):
    """sum over the pixels of a (HW, ch) float32 array the way part_sums does it: parts, R rows strided, tree, parts in double."""
    HW = a.shape[0]
    nparts, R = hin_parts(HW), 256 // Q
    chunk = -(-HW // nparts)
    tot = np.zeros(a.shape[1:], dtype=np.float64)
    for k in range(nparts):
        seg = a[k * chunk:min(HW, (k + 1) * chunk)]
        if seg.shape[0]:
            tot += strided_sum32(seg, R).astype(np.float64)
    return tot


def max_0(v):
    return np.maximum(v, 0.0)


def hin_fwd32(x, gamma, beta, ch, slope=SLOPE, eps=HIN_EPS, one_pass=False):
    """float32 restatement; one_pass=True forms the variance as E[x^2] - m^2 from fp32 partial sums (the rejected form)."""
    N, H, W, C = x.shape
    xf = x.astype(F32)
    pre = xf.copy()
    stats = np.zeros((N, 2, ch), dtype=F32)
    for n in range(N):
        if not ch:
            break
        a = xf[n, :, :, :ch].reshape(H * W, ch)
        s = hin_part_sums32(a, ch // 4)
        if one_pass:
            m = s / (H * W)
            var = max_0(hin_part_sums32(a * a, ch // 4) / (H * W) - m * m)
        else:
            d = a - (s / (H * W)).astype(F32)
            dm = hin_part_sums32(d, ch // 4) / (H * W)
            var = max_0(hin_part_sums32(d * d, ch // 4) / (H * W) - dm * dm)
            m = (s / (H * W)).astype(F32).astype(np.float64) + dm
        stats[n, 0] = m.astype(F32)
        stats[n, 1] = (1.0 / np.sqrt(var + eps)).astype(F32)
        pre[n, :, :, :ch] = (xf[n, :, :, :ch] - stats[n, 0]) * stats[n, 1] * gamma.astype(F32) + beta.astype(F32)
    out = np.where(pre > 0, pre, pre * F32(slope))
    assert out.dtype == F32
    return out, stats


def hin_bwd32(g, out, x, gamma, stats, ch, dgamma0, dbeta0, slope=SLOPE):
    N, H, W, C = x.shape
    gy = g.astype(F32) * np.where(out > 0, F32(1), F32(slope))
    gx = gy.copy()
    dg, db = np.zeros(ch), np.zeros(ch)
    inv = F32(1) / F32(H * W)
    for n in range(N):
        if not ch:
            break
        xh = (x[n, :, :, :ch].astype(F32) - stats[n, 0]) * stats[n, 1]
        gyc = gy[n, :, :, :ch]
        s1 = hin_part_sums32(gyc.reshape(H * W, ch), ch // 4)
        s2 = hin_part_sums32((gyc * xh).reshape(H * W, ch), ch // 4)
        db += s1
        dg += s2
        gx[n, :, :, :ch] = stats[n, 1] * gamma.astype(F32) * (gyc - s1.astype(F32) * inv - xh * (s2.astype(F32) * inv))
    assert gx.dtype == F32
    r = dict(gx=gx)
    if ch:
        r["dgamma"] = dgamma0.astype(F32) + dg.astype(F32)
        r["dbeta"] = dbeta0.astype(F32) + db.astype(F32)
    return r


# ---- FAC_bias ----------------------------------------------------------------------------------------------------------------
def fac_fwd(feat, filt):
    C = feat.shape[-1]
    return feat * filt[..., :C] + filt[..., C:], np.abs(feat * filt[..., :C]) + np.abs(filt[..., C:])


def fac_bwd(g, feat, filt):
    C = feat.shape[-1]
    gfilt = np.concatenate([g * feat, g], -1)
    return dict(gfeat=(g * filt[..., :C], np.abs(g * filt[..., :C])), gfilt=(gfilt, np.abs(gfilt)))


def fac_fwd32(feat, filt):
    C = feat.shape[-1]
    f = filt.astype(F32)
    return feat.astype(F32) * f[..., :C] + f[..., C:]


def fac_bwd32(g, feat, filt):
    C = feat.shape[-1]
    g32 = g.astype(F32)
    return dict(gfeat=g32 * filt.astype(F32)[..., :C], gfilt=np.concatenate([g32 * feat.astype(F32), g32], -1))


# ---- LayerNorm2d -------------------------------------------------------------------------------------------------------------
def ln_stats(x, eps=LN_EPS):
    mu = x.mean(-1, keepdims=True)
    d = x - mu
    rstd = 1.0 / np.sqrt((d * d).mean(-1, keepdims=True) + eps)
    return d * rstd, rstd, rstd * (np.abs(x) + np.abs(x).mean(-1, keepdims=True))


def ln_fwd(x, w, b, eps=LN_EPS):
    y, rstd, Ty = ln_stats(x, eps)
    return y * w + b, np.abs(w) * Ty + np.abs(b)


def ln_bwd(g, x, w, res, dw0, db0, eps=LN_EPS):
    """gx = rstd (g w - y mean(g w y) - mean(g w)) + res ; dw = dw0 + sum g y ; db = db0 + sum g."""
    y, rstd, Ty = ln_stats(x, eps)
    gh = g * w
    mean = lambda a: a.mean(-1, keepdims=True)                         # noqa: E731
    m1, m2 = mean(gh), mean(gh * y)
    r = 0.0 if res is None else res
    gx = (gh - y * m2 - m1) * rstd + r
    Sgx = rstd * (np.abs(gh) + np.abs(y) * mean(np.abs(gh * y)) + mean(np.abs(gh)) + Ty * np.abs(m2) + np.abs(y) * mean(np.abs(gh) * Ty)) \
        + np.abs(r)
    ax = tuple(range(x.ndim - 1))
    dw = dw0 + (g * y).sum(ax)
    db = db0 + g.sum(ax)
    return dict(gx=(gx, Sgx), dw=(dw, np.abs(dw0) + (np.abs(g) * Ty).sum(ax)), db=(db, np.abs(db0) + np.abs(g).sum(ax)))


def _group_sum32(v):
    """Sum over the last axis (C channels = C / 4 lanes of 4): in-lane sequential, then a tree over the lanes."""
    C = v.shape[-1]
    q = v.reshape(v.shape[:-1] + (C // 4, 4))
    lane = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
    return tree32(np.moveaxis(lane, -1, 0))[..., None]


def ln_fwd32(x, w, b, eps=LN_EPS):
    xf, C = x.astype(F32), x.shape[-1]
    mu = _group_sum32(xf) * (F32(1) / F32(C))
    d = xf - mu
    var = _group_sum32(d * d) * (F32(1) / F32(C))
    rstd = F32(1) / np.sqrt(var + F32(eps))
    out = w.astype(F32) * (d * rstd) + b.astype(F32)
    assert out.dtype == F32
    return out


def ln_bwd32(g, x, w, res, dw0, db0, eps=LN_EPS, lanes=4096):
    xf, gf, wf, C = x.astype(F32), g.astype(F32), w.astype(F32), x.shape[-1]
    ic = F32(1) / F32(C)
    mu = _group_sum32(xf) * ic
    d = xf - mu
    rstd = F32(1) / np.sqrt(_group_sum32(d * d) * ic + F32(eps))
    y = d * rstd
    gh = gf * wf
    m1, m2 = _group_sum32(gh) * ic, _group_sum32(gh * y) * ic
    gx = (gh - y * m2 - m1) * rstd + (F32(0) if res is None else res.astype(F32))
    assert gx.dtype == F32
    dw = dw0.astype(F32) + strided_sum32((gf * y).reshape(-1, C), lanes)
    db = db0.astype(F32) + strided_sum32(gf.reshape(-1, C), lanes)
    return dict(gx=gx, dw=dw, db=db)


# ---- depthwise 3x3 + GELU ----------------------------------------------------------------------------------------------------
def _erf(v):
    return np.vectorize(math.erf, otypes=[np.float64])(v)


def gelu(v):
    return 0.5 * v * (1.0 + _erf(v / math.sqrt(2.0)))


def _shifts(x):
    """The nine zero-padded neighbour planes x[y + dy - 1][x + dx - 1], tap order dy * 3 + dx."""
    N, H, W, C = x.shape
    p = np.zeros((N, H + 2, W + 2, C), dtype=x.dtype)
    p[:, 1:-1, 1:-1] = x
    return [p[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)]


def dw_fwd(x, w, b, c_const):
    """pre, act, pool sums (N, C) with scales; w (C, 9).  act's scale is in units of the constant c_const of `pre`."""
    sh = _shifts(x)
    pre = b + sum(sh[t] * w[:, t] for t in range(9))
    Spre = np.abs(b) + sum(np.abs(sh[t] * w[:, t]) for t in range(9))
    act = gelu(pre)
    Sact = GELU_LIP * Spre + (C_GELU / c_const) * (np.abs(pre) + np.abs(act))
    return dict(pre=(pre, Spre), act=(act, Sact), pool=(act.sum((1, 2)), (Sact + np.abs(act)).sum((1, 2))))


def dw_bwd(gd, x, w, dw0, db0):
    """gin[y][x] = sum_t gd[y - dy + 1][x - dx + 1] w[t] ; dw[c][t] = dw0 + sum gd in(shifted) ; db = db0 + sum gd."""
    gs, sh = _shifts(gd), _shifts(x)
    gin = sum(gs[8 - t] * w[:, t] for t in range(9))
    Sgin = sum(np.abs(gs[8 - t] * w[:, t]) for t in range(9))
    dw = dw0 + np.stack([(gd * sh[t]).sum((0, 1, 2)) for t in range(9)], -1)
    Sdw = np.abs(dw0) + np.stack([np.abs(gd * sh[t]).sum((0, 1, 2)) for t in range(9)], -1)
    return dict(gin=(gin, Sgin), dw=(dw, Sdw), db=(db0 + gd.sum((0, 1, 2)), np.abs(db0) + np.abs(gd).sum((0, 1, 2))))


def gelu32(v):
    v = v.astype(F32)
    out = F32(0.5) * v * (F32(1) + _erf(v * F32(0.70710678118654752440)).astype(F32))
    assert out.dtype == F32
    return out


def dw_fwd32(x, w, b, lanes=256):
    sh, wf = _shifts(x.astype(F32)), w.astype(F32)
    pre = np.broadcast_to(b.astype(F32), x.shape).copy()
    for t in range(9):
        pre = pre + sh[t] * wf[:, t]
    act = gelu32(pre)
    N, H, W, C = x.shape
    pool = np.stack([strided_sum32(act[n].reshape(H * W, C), lanes) for n in range(N)])
    assert pre.dtype == F32 and pool.dtype == F32
    return dict(pre=pre, act=act, pool=pool)


def dw_bwd32(gd, x, w, dw0, db0, lanes=256):
    g32, wf = gd.astype(F32), w.astype(F32)
    gs, sh = _shifts(g32), _shifts(x.astype(F32))
    gin = np.zeros(x.shape, dtype=F32)
    for t in range(9):
        gin = gin + gs[8 - t] * wf[:, t]
    C = x.shape[-1]
    dw = dw0.astype(F32) + np.stack([strided_sum32((g32 * sh[t]).reshape(-1, C), lanes) for t in range(9)], -1)
    db = db0.astype(F32) + strided_sum32(g32.reshape(-1, C), lanes)
    return dict(gin=gin, dw=dw, db=db)


# ---- colsum, gs_reduce -------------------------------------------------------------------------------------------------------
def colsum(g, db0):
    C = g.shape[-1]
    return db0 + g.reshape(-1, C).sum(0), np.abs(db0) + np.abs(g).reshape(-1, C).sum(0)


def colsum32(g, db0, lanes=256):
    return db0.astype(F32) + strided_sum32(g.astype(F32).reshape(-1, g.shape[-1]), lanes)


def gs_reduce(gxs, xi, xe):
    C = xi.shape[-1]
    a, b = gxs[..., :C] * xi, gxs[..., C:] * xe
    return (a + b).sum((1, 2)), (np.abs(a) + np.abs(b)).sum((1, 2))


def gs_reduce32(gxs, xi, xe, lanes=256):
    C = xi.shape[-1]
    g = gxs.astype(F32)
    t = g[..., :C] * xi.astype(F32) + g[..., C:] * xe.astype(F32)
    return np.stack([strided_sum32(t[n].reshape(-1, C), lanes) for n in range(t.shape[0])])


# ---- squeeze-excite ----------------------------------------------------------------------------------------------------------
def sigmoid32(v):
    s = F32(1) / (F32(1) + np.exp(-np.asarray(v, dtype=F32)))
    assert s.dtype == F32
    return s


def se_fwd(pool, inv_hw, W1, b1, W2, b2):
    """m, pre-activation z1p, z1, s from pool partials (N, parts, C), each with its scale in units of 2^-24: the sequential-sum
    bounds of test_hip_pw_precision.se_ref ((n + 2) sum |terms|, earlier stages propagated through |W|; ReLU 1-Lipschitz, sigmoid
    1/4-Lipschitz) and SIG_MARGIN times numpy float32's own sigmoid error on the same arguments."""
    N, parts, C = pool.shape
    m = pool.sum(1) * inv_hw
    Sm = (parts + 2) * np.abs(pool).sum(1) * inv_hw
    z1p = m @ W1.T + b1
    Sz = (C + 2) * (np.abs(m) @ np.abs(W1).T + np.abs(b1)) + Sm @ np.abs(W1).T
    z1 = np.maximum(z1p, 0.0)
    v = z1 @ W2.T + b2
    Sv = (C // 2 + 2) * (np.abs(z1) @ np.abs(W2).T + np.abs(b2)) + Sz @ np.abs(W2).T
    s = 1.0 / (1.0 + np.exp(-v))
    e_sig = float(np.abs(sigmoid32(v).astype(np.float64) - s).max())
    return dict(m=(m, Sm), z1p=z1p, z1=(z1, Sz), s=(s, 0.25 * Sv + SIG_MARGIN * e_sig / EPS))


def se_fwd32(pool, inv_hw, W1, b1, W2, b2):
    N, parts, C = pool.shape
    nseg = 256 // C
    m = strided_sum32(np.moveaxis(pool.astype(F32), 1, 0), 1 << (4 * nseg - 1).bit_length()) * F32(inv_hw)
    f = lambda a: a.astype(F32)                                        # noqa: E731
    z1 = np.maximum(np.stack([strided_sum32(f(W1).T * m[n][:, None], 64) for n in range(N)]) + f(b1), F32(0))
    v = np.stack([strided_sum32(f(W2).T * z1[n][:, None], 64) for n in range(N)]) + f(b2)
    assert v.dtype == F32
    return dict(m=m, z1=z1, s=sigmoid32(v))


def se_bwd(gs, s, z1, m, W1, W2, dW1_0, db1_0, dW2_0, db2_0):
    """s, z1, m are the kernel's inputs (the forward's fp32 outputs); the ReLU mask is z1 > 0."""
    d2 = gs * s * (1.0 - s)
    Sd2 = np.abs(d2) * 3.0
    mask = z1 > 0
    d1 = np.where(mask, d2 @ W2, 0.0)
    Sd1 = np.where(mask, Sd2 @ np.abs(W2), 0.0)
    return dict(gm=(d1 @ W1, Sd1 @ np.abs(W1)),
                dW2=(dW2_0 + d2.T @ z1, np.abs(dW2_0) + Sd2.T @ np.abs(z1)),
                dW1=(dW1_0 + d1.T @ m, np.abs(dW1_0) + Sd1.T @ np.abs(m)),
                db2=(db2_0 + d2.sum(0), np.abs(db2_0) + Sd2.sum(0)),
                db1=(db1_0 + d1.sum(0), np.abs(db1_0) + Sd1.sum(0)))


def _seq32(t):
    """Plain sequential float32 sum over axis 0."""
    acc = np.zeros(t.shape[1:], dtype=F32)
    for i in range(t.shape[0]):
        acc = acc + t[i].astype(F32)
    return acc


def se_bwd32(gs, s, z1, m, W1, W2, dW1_0, db1_0, dW2_0, db2_0):
    f = lambda a: a.astype(F32)                                        # noqa: E731
    sf = f(s)
    d2 = f(gs) * sf * (F32(1) - sf)
    N = gs.shape[0]
    d1 = np.stack([np.where(z1[n] > 0, _seq32(f(W2) * d2[n][:, None]), F32(0)) for n in range(N)])
    gm = np.stack([_seq32(f(W1) * d1[n][:, None]) for n in range(N)])
    assert gm.dtype == F32
    return dict(gm=gm,
                dW2=f(dW2_0) + _seq32(d2[:, :, None] * f(z1)[:, None, :]),
                dW1=f(dW1_0) + _seq32(d1[:, :, None] * f(m)[:, None, :]),
                db2=f(db2_0) + _seq32(d2), db1=f(db1_0) + _seq32(d1))


# ---- losses, norm, AdamW -----------------------------------------------------------------------------------------------------
GRID_THREADS = 2048 * 256


def _thread_sums32(t, threads=GRID_THREADS):
    """Per-thread float32 sums of a flat float32 array read as f32x4 by a grid-stride loop; the threads' sums are added in double."""
    n4 = t.size // 4
    threads = min(threads, -(-n4 // 256) * 256)
    k = -(-n4 // threads)
    q = np.zeros((k * threads, 4), dtype=F32)
    q[:n4] = t.reshape(n4, 4)
    q = q.reshape(k, threads, 4)
    acc = np.zeros(threads, dtype=F32)
    return k, q, acc


def charbonnier(pred, gt, gscale, eps=CHARB_EPS):
    d = pred - gt
    r = np.sqrt(d * d + eps)
    g = d / r * gscale
    return dict(loss=(np.float64(r.sum()), np.float64(r.sum())), grad=(g, np.abs(g)))


def charbonnier32(pred, gt, gscale, eps=CHARB_EPS):
    d = pred.astype(F32) - gt.astype(F32)
    r = np.sqrt(d * d + F32(eps))
    g = d / r * F32(gscale)
    assert g.dtype == F32
    k, q, acc = _thread_sums32(r)
    for i in range(k):
        for j in range(4):
            acc = acc + q[i, :, j]
    return dict(loss=acc.astype(np.float64).sum(), grad=g)


def sqnorm(g):
    s = np.float64((g * g).sum())
    return s, s


def sqnorm32(g, threads=GRID_THREADS):
    k, q, acc = _thread_sums32(g.astype(F32), threads)
    for i in range(k):
        acc = acc + (((q[i, :, 0] * q[i, :, 0] + q[i, :, 1] * q[i, :, 1]) + q[i, :, 2] * q[i, :, 2]) + q[i, :, 3] * q[i, :, 3])
    assert acc.dtype == F32
    return acc.astype(np.float64).sum()


PSNR_SCALE = 10.0 / math.log(10.0)


def psnr_loss(pred, gt, weight):
    """pred, gt (B, per).  loss = w 10/ln10 mean_b log(mse_b + 1e-8); sq_b = sum d^2; grad = d 2 w scale / (per B (mse_b + 1e-8)).
    The loss moves with sq_b by w scale / B * (sq_b / per) / (mse_b + 1e-8) per unit of relative error: that sum is its scale."""
    B, per = pred.shape
    d = pred - gt
    sq = (d * d).sum(1)
    mse = sq / per
    loss = weight * PSNR_SCALE * np.log(mse + 1e-8).mean()
    Sloss = weight * PSNR_SCALE * (mse / (mse + 1e-8)).mean() + abs(loss) * 2.0 ** -26
    grad = d * (weight * PSNR_SCALE * 2.0 / (per * B) / (mse + 1e-8))[:, None]
    return dict(loss=(np.float64(loss), np.float64(Sloss)), sq=(sq, sq), grad=(grad, np.abs(grad)))


def psnr_loss32(pred, gt, weight):
    B, per = pred.shape
    d = pred.astype(F32) - gt.astype(F32)
    sq = np.array([sqnorm32(d[b], 256 * 256) for b in range(B)])          # psnr_blocks: 256 workgroups per sample
    mse = sq / per
    coef = (weight * PSNR_SCALE * 2.0 / (per * B) / (mse + 1e-8)).astype(F32)
    grad = d * coef[:, None]
    assert grad.dtype == F32
    return dict(loss=weight * PSNR_SCALE * np.log(mse + 1e-8).mean(), sq=sq, grad=grad)


def adamw_scalars(lr, b1, b2, step):
    """(lr, bc1, sqrt(bc2)) as the launcher forms them: fp32 betas promoted to double, the results rounded to fp32."""
    return f32s(lr), f32s(1.0 - f32s(b1) ** step), f32s(math.sqrt(1.0 - f32s(b2) ** step))


def clip_coef(sq, max_norm, gscale):
    if max_norm <= 0:
        return gscale
    return min(max_norm / (math.sqrt(sq) * gscale + f32s(1e-6)), 1.0) * gscale


def clip_adamw(p, g, m, v, sq, *, max_norm, gscale, lr, bc1, bc2s, b1, b2, eps, wd):
    """One step in float64 from fp32 state; every scalar is an fp32 number (adamw_scalars).  Scales: |p| + |update| for p,
    the sums of |terms| for m and v."""
    gc = g * clip_coef(sq, max_norm, gscale)
    m1 = m * b1 + gc * (1.0 - b1)
    v1 = v * b2 + gc * gc * (1.0 - b2)
    upd = (lr / bc1) * m1 / (np.sqrt(v1) / bc2s + eps)
    pd = p * (1.0 - lr * wd)
    Sm = np.abs(m * b1) + np.abs(gc * (1.0 - b1))
    # p is gated twice: against |p| + |update| (a momentum that cancels, m b1 ~ -g (1 - b1), next to p ~ 0 leaves that scale far
    # below the rounding of the update's own terms: the restatement's worst ratio is in the hundreds) and, as "p_terms", against
    # |p| + the update with its momentum terms in absolute value, which fp32 meets with a constant of ordinary size
    return dict(p=(pd - upd, np.abs(pd) + np.abs(upd)), p_terms=(pd - upd, np.abs(pd) + (lr / bc1) * Sm / (np.sqrt(v1) / bc2s + eps)),
                m=(m1, Sm), v=(v1, v1))


def clip_adamw32(p, g, m, v, sq, *, max_norm, gscale, lr, bc1, bc2s, b1, b2, eps, wd):
    f = lambda a: np.asarray(a, dtype=F32)                             # noqa: E731
    coef = F32(1)
    if max_norm > 0:
        c = F32(max_norm) / (F32(math.sqrt(sq)) * F32(gscale) + F32(1e-6))
        coef = c if c < 1 else F32(1)
    coef = coef * F32(gscale)
    step = F32(lr) / F32(bc1)
    gv = f(g) * coef
    pv = f(p) * (F32(1) - F32(lr) * F32(wd))
    mv = f(m) * F32(b1) + gv * (F32(1) - F32(b1))
    vv = f(v) * F32(b2) + gv * gv * (F32(1) - F32(b2))
    pv = pv - step * mv / (np.sqrt(vv) / F32(bc2s) + F32(eps))
    assert pv.dtype == F32 and mv.dtype == F32 and vv.dtype == F32
    return dict(p=pv, m=mv, v=vv)


# ---- the float32 restatement as a backend ------------------------------------------------------------------------------------
class Float32Backend:
    """The restatements above behind the interface the comparisons below drive; the GPU test file has the same interface over
    refid_amd.ops.  Arrays in are float64 of fp32 numbers, arrays out are whatever the backend computes in (read as float64)."""

    def hin_fwd(self, x, gamma, beta, ch):
        return hin_fwd32(x, gamma, beta, ch)

    def hin_bwd(self, g, out, x, gamma, stats, ch, dg0, db0):
        return hin_bwd32(g, out, x, gamma, stats, ch, dg0, db0)

    def fac_fwd(self, feat, filt):
        return fac_fwd32(feat, filt)

    def fac_bwd(self, g, feat, filt):
        return fac_bwd32(g, feat, filt)

    def ln_fwd(self, x, w, b):
        return ln_fwd32(x, w, b)

    def ln_bwd(self, g, x, w, res, dw0, db0, alias=False):
        return ln_bwd32(g, x, w, res, dw0, db0)

    def dw_fwd(self, x, w, b):
        return dw_fwd32(x, w, b)

    def dw_bwd(self, gd, x, w, dw0, db0):
        return dw_bwd32(gd, x, w, dw0, db0)

    def colsum(self, g, db0):
        return colsum32(g, db0)

    def gs_reduce(self, gxs, xi, xe):
        return gs_reduce32(gxs, xi, xe)

    def se_fwd(self, pool, inv_hw, W1, b1, W2, b2):
        return se_fwd32(pool, inv_hw, W1, b1, W2, b2)

    def se_bwd(self, *a):
        return se_bwd32(*a)

    def charbonnier(self, pred, gt, gscale, want_grad=True):
        return charbonnier32(pred, gt, gscale)

    def sqnorm(self, g):
        return sqnorm32(g)

    def psnr_loss(self, pred, gt, weight):
        return psnr_loss32(pred, gt, weight)

    def clip_adamw(self, p, g, m, v, sq, step=None, **kw):
        return clip_adamw32(p, g, m, v, sq if sq is not None else 0.0, **kw)


# ---- constants ---------------------------------------------------------------------------------------------------------------
# C_LN / C_GELU / GELU_LIP / SIG_MARGIN are the project's (test_hip_pw_precision.py): LayerNorm forward uses C_LN, the GELU
# output carries GELU_LIP and C_GELU inside its scale, the squeeze-excite forward's scales are absolute bounds (constant 1) with
# SIG_MARGIN inside.  Every other constant is the next power of two at or above twice the float32 restatement's worst
# err / (2^-24 S) over all cases below (test_nongemm_ref_host.py measures it and asserts this rule); the kernels' own ratios
# are never an input.
C_LN = 16.0
CONST = {
    # float32 restatement's worst ratio (CPU) in the comment; the kernels' ratios on the MI355X are in test_hip_nongemm_precision.py
    "hin_fwd/out": 8.0,          # 3.27
    "hin_bwd/gx": 8.0,           # 3.46
    "hin_bwd/dgamma": 8.0,       # 2.15
    "hin_bwd/dbeta": 8.0,        # 2.41
    "fac/out": 4.0,              # 1.89
    "fac/gfeat": 2.0,            # 1.00
    "fac/gfilt": 2.0,            # 1.00
    "ln_fwd/out": C_LN,          # 4.87 (the project's constant; the rule gives the same 16)
    "ln_bwd/gx": 8.0,            # 3.30
    "ln_bwd/dw": 1.0,            # 0.33
    "ln_bwd/db": 1.0,            # 0.33
    "dw_fwd/pre": 16.0,          # 5.62
    "dw_fwd/act": 16.0,          # not derived: the GELU output is gated in the units of `pre` (gelu_bound's convention)
    "dw_fwd/pool": 2.0,          # 0.54
    "dw_bwd/gin": 8.0,           # 3.73
    "dw_bwd/dw": 8.0,            # 2.69
    "dw_bwd/db": 2.0,            # 0.63
    "colsum/db": 4.0,            # 1.24
    "gs_reduce/gs": 2.0,         # 0.59
    "se_fwd/m": 1.0, "se_fwd/z1": 1.0, "se_fwd/s": 1.0,          # absolute bounds (se_ref's), constant 1
    "se_bwd/gm": 1.0,            # 0.33
    "se_bwd/dW2": 4.0,           # 1.14
    "se_bwd/dW1": 2.0,           # 0.76
    "se_bwd/db2": 2.0,           # 0.87
    "se_bwd/db1": 1.0,           # 0.49
    "charbonnier/loss": 4.0,     # 1.98
    "charbonnier/grad": 8.0,     # 3.46
    "sqnorm/sq": 2.0,            # 0.54
    "psnr/loss": 1.0,            # 0.49
    "psnr/sq": 2.0,              # 0.59
    "psnr/grad": 8.0,            # 2.39
    "adamw/p": 1024.0,           # 457: against |p| + |update| (see clip_adamw)
    "adamw/p_terms": 16.0,       # 4.99: against |p| + the update's terms
    "adamw/m": 8.0,              # 2.99
    "adamw/v": 16.0,             # 5.14
}
NOT_DERIVED = ("ln_fwd/out", "dw_fwd/act", "se_fwd/m", "se_fwd/z1", "se_fwd/s")


# ---- cases: the smallest shapes that reach each branch -----------------------------------------------------------------------
HIN_CASES = [
    # (N, H, W, C, ch), families
    ((2, 5, 7, 8, 4), ["uniform"]),                    # Q = 1
    ((1, 33, 31, 16, 8), NORM_FAMILIES),               # HW = 1023: one part
    ((2, 41, 25, 64, 32), NORM_FAMILIES),              # HW = 1025: two ragged parts, 513 + 512
    ((1, 8, 8, 1024, 1024), ["uniform"]),              # R = 1: no tree
    ((1, 363, 362, 8, 8), ["uniform"]),                # HW = 131 406 > 131 072: parts capped at 128
    ((1, 257, 257, 16, 0), ["uniform"]),               # ch = 0
]
FAC_CASES = [((2, 9, 11, 16), FAMILIES), ((1, 257, 257, 64), ["uniform"])]      # the second wraps ew_blocks (4096 x 256)
LN_FWD_CASES = [((1, 5, 7, c), NORM_FAMILIES) for c in (16, 32, 64, 128)] + [((1, 131, 127, 128), NORM_FAMILIES)]
LN_BWD_CASES = [
    ((1, 83, 61, 128), ["uniform", "offset32"]),       # 5063 pixels: u = 1 partly valid, u >= 2 clamped
    ((1, 131, 127, 128), ["uniform"]),                 # 16 637 > 4 x 4096: the outer loop wraps
    ((1, 97, 89, 64), ["uniform", "hot-pixel"]),       # 8633 > 8192
    ((3, 5, 7, 16), NORM_FAMILIES),
]
DW_CASES = [
    ((2, 23, 23, 128), ["uniform"]),                   # 529 > 64 x 8
    ((2, 37, 29, 64), FAMILIES),                       # 1073 > 1024
    ((2, 67, 63, 16), ["uniform"]),                    # 4221 > 4096
    ((2, 1, 7, 32), ["uniform"]), ((2, 5, 1, 32), ["uniform"]),
]
COLSUM_CASES = [((1, 12, 25, 1024), 1024), ((1, 1, 4133, 64), 64), ((1, 7, 11, 64), 8)]      # (shape of the buffer, C summed)
GS_CASES = [(3, 47, 45, 64), (1, 33, 32, 128), (2, 5, 7, 16)]
SE_CASES = [(c, parts) for c in (16, 32, 64, 128) for parts in (1, 3, 16, 17, 64)]
LOSS_COUNTS = [4, 3076, 2097152 + 1036]
PSNR_CASES = [(3, 16), (3, 262144 + 308)]
ADAMW_BIG = 2097152 + 1036                             # above 2048 blocks x 1024 elements, ragged final wrap
# (count, clip regime, grad_scale, |p|): the full product at count = 4; at the large count, where only the grid-stride wrap is
# new, four cases that hold every regime, both grad_scales and both |p| at least once
ADAMW_CASES = [(4, regime, gs, ps) for regime in ("clip", "noclip", "off") for gs in (1.0, 0.125) for ps in (1.0, 1e-3)] + \
    [(ADAMW_BIG, "clip", 1.0, 1.0), (ADAMW_BIG, "noclip", 0.125, 1e-3), (ADAMW_BIG, "off", 1.0, 1e-3), (ADAMW_BIG, "clip", 0.125, 1e-3)]
ADAMW_STEPS = (1, 2, 1000)
ADAMW_HYPER = dict(lr=f32s(2e-4), b1=f32s(0.9), b2=f32s(0.99), eps=f32s(1e-8), wd=f32s(1e-4))


def _keys(worst, name, got, ref, c, what):
    """check every output of a kernel; record the worst ratio per output in `worst`."""
    for k, (r, S) in ref.items():
        w = check(got[k], r, S, c if c is not None else CONST[f"{name}/{k}"], f"{what}: {k}")
        worst[f"{name}/{k}"] = max(worst.get(f"{name}/{k}", 0.0), w)


def compare_hin(be, cfg, fam, worst, c=None):
    N, H, W, C, ch = cfg
    x = family(fam, (N, H, W, C), 11)
    gamma = fp32(1.0 + 0.3 * uni(12, ch)) if ch else None
    beta = fp32(0.5 * uni(13, ch)) if ch else None
    out, stats = be.hin_fwd(x, gamma, beta, ch)
    out = np.asarray(out, dtype=np.float64)
    ref, S = hin_fwd(x, gamma, beta, ch)
    what = f"hin_lrelu {cfg} {fam}"
    _keys(worst, "hin_fwd", dict(out=out), dict(out=(ref, S)), c, what + " forward")
    g = fp32(uni(14, N, H, W, C))
    dg0, db0 = (fp32(uni(15, ch)), fp32(uni(16, ch))) if ch else (None, None)
    got = be.hin_bwd(g, out, x, gamma, stats, ch, dg0, db0)
    _keys(worst, "hin_bwd", got, hin_bwd(g, out, x, gamma, ch, dg0, db0), c, what + " backward")


def compare_fac(be, shape, fam, worst, c=None):
    N, H, W, C = shape
    feat, filt, g = family(fam, shape, 21), family(fam, (N, H, W, 2 * C), 22), fp32(uni(23, *shape))
    what = f"fac {shape} {fam}"
    ref, S = fac_fwd(feat, filt)
    _keys(worst, "fac", dict(out=be.fac_fwd(feat, filt)), dict(out=(ref, S)), c, what)
    _keys(worst, "fac", be.fac_bwd(g, feat, filt), fac_bwd(g, feat, filt), c, what)


def ln_inputs(shape, fam):
    C = shape[-1]
    return (family(fam, shape, 31), fp32(1.0 + 0.3 * uni(32, C)), fp32(uni(33, C)), fp32(uni(34, *shape)), fp32(uni(35, *shape)),
            fp32(uni(36, C)), fp32(uni(37, C)))


def compare_ln_fwd(be, shape, fam, worst, c=None):
    x, w, b = ln_inputs(shape, fam)[:3]
    ref, S = ln_fwd(x, w, b)
    _keys(worst, "ln_fwd", dict(out=be.ln_fwd(x, w, b)), dict(out=(ref, S)), c, f"layernorm2d_fwd {shape} {fam}")


def compare_ln_bwd(be, shape, fam, mode, worst, c=None):
    """mode: 'none' (no residual), 'res' (a separate residual), 'alias' (the residual is gx's own content)."""
    x, w, b, g, res, dw0, db0 = ln_inputs(shape, fam)
    res = None if mode == "none" else res
    got = be.ln_bwd(g, x, w, res, dw0, db0, alias=mode == "alias")
    _keys(worst, "ln_bwd", got, ln_bwd(g, x, w, res, dw0, db0), c, f"layernorm2d_bwd {shape} {fam} res={mode}")
    return got


def dw_inputs(shape, fam):
    C = shape[-1]
    return (family(fam, shape, 41), fp32(uni(42, C, 9) / 3.0), fp32(0.1 * uni(43, C)), fp32(uni(44, *shape)), fp32(uni(45, C, 9)),
            fp32(uni(46, C)))


def compare_dw(be, shape, fam, worst, c=None):
    x, w, b, gd, dw0, db0 = dw_inputs(shape, fam)
    what = f"dwconv3x3 {shape} {fam}"
    got = be.dw_fwd(x, w, b)
    _keys(worst, "dw_fwd", got, dw_fwd(x, w, b, CONST["dw_fwd/pre"]), c, what + " forward")
    gotb = be.dw_bwd(gd, x, w, dw0, db0)
    _keys(worst, "dw_bwd", gotb, dw_bwd(gd, x, w, dw0, db0), c, what + " backward")
    return got, gotb


def compare_colsum(be, case, worst, c=None):
    shape, C = case
    buf = fp32(uni(51, *shape) + 0.25)
    db0 = fp32(uni(52, C))
    g = buf[..., 8:8 + C] if C < shape[-1] else buf
    ref, S = colsum(g, db0)
    _keys(worst, "colsum", dict(db=be.colsum(g, db0)), dict(db=(ref, S)), c, f"colsum {case}")


def compare_gs(be, shape, worst, c=None):
    N, H, W, C = shape
    gxs, xi, xe = fp32(uni(61, N, H, W, 2 * C)), fp32(uni(62, *shape) + 0.5), fp32(uni(63, *shape))
    ref, S = gs_reduce(gxs, xi, xe)
    _keys(worst, "gs_reduce", dict(gs=be.gs_reduce(gxs, xi, xe)), dict(gs=(ref, S)), c, f"egaca_gs_reduce {shape}")


def se_inputs(C, parts, N=3):
    Ch, hw = C // 2, 64 * parts
    lev = np.array([-1.0, 0.3, 1.6])[:N, None, None]
    pool = fp32((lev + 0.3 * uni(71, N, 1, C) + 0.5 * uni(72, N, parts, C)) * (hw / parts))
    W1, b1 = fp32(uni(73, Ch, C) / math.sqrt(C) * 2), fp32(0.3 * uni(74, Ch))
    W2, b2 = fp32(uni(75, C, Ch) / math.sqrt(Ch) * 2), fp32(0.3 * uni(76, C))
    return pool, 1.0 / hw, W1, b1, W2, b2


def compare_se(be, C, parts, worst, c=None):
    pool, inv_hw, W1, b1, W2, b2 = se_inputs(C, parts)
    R = se_fwd(pool, inv_hw, W1, b1, W2, b2)
    assert (R["z1"][0] > 0).any() and (R["z1"][0] == 0).any(), "both sides of the ReLU must be exercised"
    got = {k: np.asarray(v, dtype=np.float64) for k, v in be.se_fwd(pool, inv_hw, W1, b1, W2, b2).items()}
    what = f"squeeze-excite C = {C}, {parts} parts"
    _keys(worst, "se_fwd", got, {k: R[k] for k in ("m", "z1", "s")}, c, what + " forward")
    assert (got["z1"] > 0).any() and (got["z1"] == 0).any()
    Ch = C // 2
    gs = fp32(uni(77, 3, C))
    z = [fp32(uni(78 + i, *s)) for i, s in enumerate([(Ch, C), (Ch,), (C, Ch), (C,)])]
    gotb = be.se_bwd(gs, got["s"], got["z1"], got["m"], W1, W2, *z)
    _keys(worst, "se_bwd", gotb, se_bwd(gs, got["s"], got["z1"], got["m"], W1, W2, *z), c, what + " backward")


def loss_inputs(count, seed=81):
    """gt and pred = gt + d with |d| log-uniform over 1e-8 .. 10 (gt of d's own size on every other element, so that small d
    survive the rounding of pred) and pred == gt exactly on every seventh element."""
    u = uni(seed, count)
    d = np.sign(uni(seed + 1, count)) * np.exp(np.log(1e-8) + (np.log(10.0) - np.log(1e-8)) * 0.5 * (uni(seed + 2, count) + 1))
    gt = fp32(np.where(np.arange(count) % 2 == 0, u, 4.0 * u * np.abs(d)))
    pred = fp32(gt + d)
    pred[::7] = gt[::7]
    return pred, gt


def compare_charbonnier(be, count, gscale, want_grad, worst, c=None):
    pred, gt = loss_inputs(count)
    ref = charbonnier(pred, gt, gscale)
    got = be.charbonnier(pred, gt, gscale, want_grad)
    if not want_grad:
        ref = dict(loss=ref["loss"])
    assert count < 7 or ((ref["loss"][0] > 0) and (not want_grad or (ref["grad"][0][::7] == 0).all()))
    _keys(worst, "charbonnier", got, ref, c, f"charbonnier count = {count}, grad_scale = {gscale}, grad = {want_grad}")


def compare_sqnorm(be, count, worst, c=None):
    g = fp32(uni(91, count) * np.exp2(10 * uni(92, count)))
    ref, S = sqnorm(g)
    _keys(worst, "sqnorm", dict(sq=be.sqnorm(g)), dict(sq=(ref, S)), c, f"grad_sqnorm count = {count}")


def compare_psnr(be, case, worst, c=None):
    B, per = case
    pred, gt = (a.reshape(B, per) for a in loss_inputs(B * per, seed=101))
    pred = 0.1 * pred
    gt = 0.1 * gt
    pred, gt = fp32(pred), fp32(gt)
    pred[1] = gt[1]                                                    # mse = 0: the 1e-8 floor decides
    _keys(worst, "psnr", be.psnr_loss(pred, gt, 0.5), psnr_loss(pred, gt, 0.5), c, f"psnr_loss {case}")


def compare_adamw(be, case, worst, c=None, dev=None):
    """Steps 1, 2, 1000 in sequence, each from the backend's own fp32 state of the previous one.  `dev`, when given, runs the same
    step through the hyper-parameters-in-memory form on a copy of the state; the two must agree bit for bit."""
    count, regime, gscale, pscale = case
    h = ADAMW_HYPER
    p = fp32(pscale * (uni(111, count) + 0.25))
    m, v = np.zeros(count), np.zeros(count)
    for step in ADAMW_STEPS:
        g = fp32(uni(112 + step, count) * np.exp2(3 * uni(113, count)) / gscale)
        sq_true = float(((g * gscale) ** 2).sum())
        # the squared norm is an INPUT (of the unscaled gradients, as grad_sqnorm gives it); the regimes place max_norm around it
        sq = sq_true / gscale ** 2
        max_norm = {"clip": f32s(0.01 * math.sqrt(sq_true)), "noclip": f32s(4.0 * math.sqrt(sq_true)), "off": 0.0}[regime]
        lr, bc1, bc2s = adamw_scalars(h["lr"], h["b1"], h["b2"], step)
        kw = dict(max_norm=max_norm, gscale=f32s(gscale), lr=lr, bc1=bc1, bc2s=bc2s, b1=h["b1"], b2=h["b2"], eps=h["eps"], wd=h["wd"])
        ref = clip_adamw(p, g, m, v, sq, **kw)
        got = be.clip_adamw(p, g, m, v, None if regime == "off" else sq, step=step, **kw)
        got = {k: np.asarray(a, dtype=np.float64) for k, a in got.items()}
        got["p_terms"] = got["p"]
        if dev is not None:
            got2 = dev(p, g, m, v, None if regime == "off" else sq, step=step, **kw)
            for k in got2:
                assert np.array_equal(got[k], np.asarray(got2[k], dtype=np.float64)), f"clip_adamw_dev differs from clip_adamw: {k}, {case}, step {step}"
        _keys(worst, "adamw", got, ref, c, f"clip_adamw {case} step {step}")
        p, m, v = got["p"], got["m"], got["v"]
