"""Element-wise precision contract of the kernels that are not GEMMs against float64: HIN + LeakyReLU and FAC_bias
(csrc/evhinet.hip), LayerNorm2d, depthwise 3x3 + GELU, colsum, gs_reduce, squeeze-excite (csrc/egaca.hip), Charbonnier, PSNRLoss,
squared norm and clip + AdamW (csrc/train.hip).

For every output element the gate is |got - ref| <= c 2^-24 S, no aggregation, no element excluded (nongemm_ref.check).  ref and S
are the hand-written float64 restatements of nongemm_ref.py (cross-checked against torch autograd in test_nongemm_ref_host.py);
c is nongemm_ref.CONST, fixed on the CPU from the float32 restatement of the same formulas (the next power of two at or above
twice its worst ratio) or taken from test_hip_pw_precision.py (C_LN, C_GELU, GELU_LIP, SIG_MARGIN) -- never from a kernel.

The shapes are the smallest that cross each launcher's grid cap, so that every grid-stride loop wraps at least once, plus the
ragged and degenerate ones (nongemm_ref.*_CASES say what each reaches).  Operands and results are channel slices of wider buffers
wherever the wrapper takes a pitch; the unused channels keep their fill value.  Accumulating destinations start non-zero.  Where
the backward kernel takes a forward output as an input (HIN's `out`, squeeze-excite's z1) the reference takes its sign decisions
from the device's tensor.

HIN's statistics: the variance is taken from the sums of x - mean (two reductions).  The form before it, E[x^2] - mean^2 from fp32
partial sums, fails this file on the families with a DC offset (see MEASURED).

MEASURED, worst err / (2^-24 S) over every case of an output: constant | float32 restatement on the CPU | MI355X
  hin_fwd/out             8 |  3.27 | 3.24
  hin_bwd/gx              8 |  3.46 | 3.46
  hin_bwd/dgamma          8 |  2.15 | 2.15
  hin_bwd/dbeta           8 |  2.41 | 2.41
  fac/out                 4 |  1.89 | 1
  fac/gfeat               2 |  1.00 | 1
  fac/gfilt               2 |  1.00 | 1
  ln_fwd/out             16 |  4.87 | 4.52
  ln_bwd/gx               8 |  3.30 | 3.3
  ln_bwd/dw               1 |  0.33 | 0.512
  ln_bwd/db               1 |  0.33 | 0.245
  dw_fwd/pre             16 |  5.62 | 5.62
  dw_fwd/act             16 |  2.03 | 2.03
  dw_fwd/pool             2 |  0.54 | 0.69
  dw_bwd/gin              8 |  3.73 | 3.54
  dw_bwd/dw               8 |  2.69 | 2.01
  dw_bwd/db               2 |  0.63 | 0.635
  colsum/db               4 |  1.24 | 1.57
  gs_reduce/gs            2 |  0.59 | 0.399
  se_fwd/m                1 |  0.53 | 0.411
  se_fwd/z1               1 |  0.03 | 0.0374
  se_fwd/s                1 |  0.04 | 0.028
  se_bwd/gm               1 |  0.33 | 0.407
  se_bwd/dW2              4 |  1.14 | 1.14
  se_bwd/dW1              2 |  0.76 | 0.97
  se_bwd/db2              2 |  0.87 | 0.865
  se_bwd/db1              1 |  0.49 | 0.626
  charbonnier/loss        4 |  1.98 | 1.98
  charbonnier/grad        8 |  3.46 | 3.46
  sqnorm/sq               2 |  0.54 | 0.541
  psnr/loss               1 |  0.49 | 0.486
  psnr/sq                 2 |  0.59 | 0.585
  psnr/grad               8 |  2.39 | 2.39
  adamw/p              1024 |   457 | 276
  adamw/p_terms          16 |  4.99 | 5.4
  adamw/m                 8 |  2.99 | 2.99
  adamw/v                16 |  5.14 | 5.14
  (adamw/p is gated against |p| + |update| as well as, under p_terms, against |p| + the update's terms: nongemm_ref.clip_adamw.)
  HIN on the one-pass statistics this file replaced (the same tests, the library built from the commit before): offset8 forward
  9.07 at (2,41,25,64,32) and backward gx 47.1 at (1,33,31,16,8); offset32 forward 31.6 and 40.4 -- against c = 8.  uniform,
  spread, hot-pixel and const-channel pass there too: the hot pixel raises sigma, not mean / sigma, and 100 x 1024 and 100^2 x 1024
  are exact in fp32.  hot-pixel is there for a form with a fixed pivot at pixel 0.
"""
import numpy as np
import pytest
import torch

import nongemm_ref as R

pytestmark = pytest.mark.gpu
FILL = 7.0
PAD = 12                         # extra channels of a wide buffer; the slice starts at channel 4 (16-byte aligned)
WORST = {}


def _ops():
    from refid_amd import ops
    return ops


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda")


def host(tn):
    return tn.detach().double().cpu().numpy()


class Wide:
    """An NHWC operand or result as a channel slice of a wider buffer; everything outside the slice keeps FILL."""

    def __init__(self, a=None, shape=None, fill=float("nan"), pad=PAD):
        shape = tuple(a.shape if a is not None else shape)
        self.buf = torch.full(shape[:-1] + (shape[-1] + pad,), FILL, dtype=torch.float32, device="cuda")
        self.t = self.buf[..., 4:4 + shape[-1]]
        self.t[...] = dev(a) if a is not None else fill
        self.C = shape[-1]

    def get(self, what):
        assert bool((self.buf[..., :4] == FILL).all()) and bool((self.buf[..., 4 + self.C:] == FILL).all()), \
            f"{what}: channels outside the slice were written"
        return host(self.t)


class HipBackend:
    """nongemm_ref's backend interface over refid_amd.ops."""
    defer = False

    def hin_fwd(self, x, gamma, beta, ch):
        ops = _ops()
        xd, out = Wide(x), Wide(shape=x.shape)
        gd, bd = (dev(gamma), dev(beta)) if ch else (None, None)
        _, stats = ops.hin_lrelu_fwd(xd.t, gd, bd, R.SLOPE, R.HIN_EPS, out=out.t)
        xd.get("hin_lrelu_fwd x")
        return out.get("hin_lrelu_fwd out"), stats

    def hin_bwd(self, g, out, x, gamma, stats, ch, dg0, db0):
        ops = _ops()
        gd, od, xd, gx = Wide(g), Wide(out), Wide(x), Wide(shape=x.shape)
        dg, db = (dev(dg0), dev(db0)) if ch else (None, None)
        ops.hin_lrelu_bwd(gd.t, od.t, xd.t, dev(gamma) if ch else None, stats, dg, db, R.SLOPE, gx=gx.t)
        r = dict(gx=gx.get("hin_lrelu_bwd gx"))
        if ch:
            r.update(dgamma=host(dg), dbeta=host(db))
        return r

    def fac_fwd(self, feat, filt):
        out = Wide(shape=feat.shape)
        _ops().fac_fwd(Wide(feat).t, Wide(filt).t, out=out.t)
        return out.get("fac_fwd out")

    def fac_bwd(self, g, feat, filt):
        gfeat, gfilt = Wide(shape=feat.shape), Wide(shape=filt.shape)
        _ops().fac_bwd(Wide(g).t, Wide(feat).t, Wide(filt).t, gfeat=gfeat.t, gfilt=gfilt.t)
        return dict(gfeat=gfeat.get("fac_bwd gfeat"), gfilt=gfilt.get("fac_bwd gfilt"))

    def ln_fwd(self, x, w, b):
        out = Wide(shape=x.shape)
        _ops().layernorm2d_fwd(Wide(x).t, dev(w), dev(b), out=out.t, eps=R.LN_EPS)
        return out.get("layernorm2d_fwd out")

    def ln_bwd(self, g, x, w, res, dw0, db0, alias=False):
        ops = _ops()
        gx = Wide(res) if alias else Wide(shape=x.shape)
        dw, db = dev(dw0), dev(db0)
        rd = None if (alias or res is None) else Wide(res).t
        if self.defer:
            ops.rows_sum_defer()
        ops.layernorm2d_bwd(Wide(g).t, Wide(x).t, dev(w), gx.t, dw, db, accumulate=alias, res=rd, eps=R.LN_EPS)
        if self.defer:
            ops.rows_sum_flush()
        return dict(gx=gx.get("layernorm2d_bwd gx"), dw=host(dw), db=host(db))

    def dw_fwd(self, x, w, b):
        ops = _ops()
        xd, wd, bd = Wide(x), dev(w), dev(b)
        pre, act, pool = ops.dwconv3x3_gelu_fwd(xd.t, wd, bd, want_pool=True)
        assert pool.shape[1] == ops.dwconv_pool_parts(x.shape[1], x.shape[2], x.shape[3])
        again = ops.dwconv3x3_gelu_fwd(xd.t, wd, bd, want_pool=True)
        assert all(torch.equal(a, b_) for a, b_ in zip((pre, act, pool), again)), "dwconv3x3_gelu_fwd: a second run differs"
        return dict(pre=host(pre), act=host(act), pool=host(pool).sum(1))

    def dw_bwd(self, gd, x, w, dw0, db0):
        ops = _ops()
        xd, gdd, wd = Wide(x), dev(gd), dev(w)
        outs = []
        for _ in range(2):
            dw, db = dev(dw0), dev(db0)
            outs.append((ops.dwconv3x3_bwd(gdd, xd.t, wd, dw, db), dw, db))
        assert all(torch.equal(a, b_) for a, b_ in zip(*outs)), "dwconv3x3_bwd: a second run differs"
        return dict(gin=host(outs[0][0]), dw=host(outs[0][1]), db=host(outs[0][2]))

    def colsum(self, g, db0):
        db = dev(db0)
        _ops().colsum(Wide(g, pad=56 if g.shape[-1] == 8 else PAD).t, db)          # C = 8: a slice of a 64-wide tensor
        return host(db)

    def gs_reduce(self, gxs, xi, xe):
        return host(_ops().egaca_gs_reduce(dev(gxs), dev(xi), dev(xe)))

    def se_fwd(self, pool, inv_hw, W1, b1, W2, b2):
        m, z1, s = _ops().se_fwd(dev(pool), inv_hw, dev(W1), dev(b1), dev(W2), dev(b2))
        return dict(m=host(m), z1=host(z1), s=host(s))

    def se_bwd(self, gs, s, z1, m, W1, W2, dW1_0, db1_0, dW2_0, db2_0):
        d = [dev(a) for a in (dW1_0, db1_0, dW2_0, db2_0)]
        gm = _ops().se_bwd(dev(gs), dev(s), dev(z1), dev(m), dev(W1), dev(W2), *d)
        return dict(gm=host(gm), dW1=host(d[0]), db1=host(d[1]), dW2=host(d[2]), db2=host(d[3]))

    def charbonnier(self, pred, gt, gscale, want_grad=True):
        grad = torch.full((pred.size,), float("nan"), device="cuda") if want_grad else None
        loss = _ops().charbonnier(dev(pred), dev(gt), grad, eps=R.CHARB_EPS, grad_scale=gscale)
        r = dict(loss=np.float64(loss.item()))
        if want_grad:
            r["grad"] = host(grad)
        return r

    def sqnorm(self, g):
        return np.float64(_ops().grad_sqnorm(dev(g))[0].item())

    def psnr_loss(self, pred, gt, weight):
        grad = torch.full(pred.shape, float("nan"), device="cuda")
        loss, sq = _ops().psnr_loss(dev(pred), dev(gt), grad, weight=weight, want_sq=True)
        return dict(loss=np.float64(loss.item()), sq=sq.cpu().numpy(), grad=host(grad))

    @staticmethod
    def _adamw_args(p, g, m, v, sq, kw):
        T = [dev(a) for a in (p, g, m, v)]
        sqd = torch.tensor([sq], dtype=torch.float64, device="cuda") if sq is not None else None
        common = dict(max_norm=kw["max_norm"], betas=(kw["b1"], kw["b2"]), eps=kw["eps"], weight_decay=kw["wd"], grad_scale=kw["gscale"])
        return T, sqd, common

    def clip_adamw(self, p, g, m, v, sq, step=None, **kw):
        T, sqd, common = self._adamw_args(p, g, m, v, sq, kw)
        _ops().clip_adamw(*T, sqd, lr=kw["lr"], step=step, **common)
        return dict(p=host(T[0]), m=host(T[2]), v=host(T[3]))

    def clip_adamw_dev(self, p, g, m, v, sq, step=None, **kw):
        T, sqd, common = self._adamw_args(p, g, m, v, sq, kw)
        hyper = torch.tensor([kw["lr"], kw["bc1"], kw["bc2s"]], dtype=torch.float32, device="cuda")
        _ops().clip_adamw_dev(*T, sqd, hyper, **common)
        return dict(p=host(T[0]), m=host(T[2]), v=host(T[3]))


BE = HipBackend()


def _w(name):
    return WORST.setdefault(name, {})


def _report(name):
    print("; ".join(f"{k} {v:.3g} (c = {R.CONST[k]:g})" for k, v in sorted(_w(name).items())))


def _ids(cases):
    return ["x".join(str(v) for v in c[0]) + "-" + fam for c in cases for fam in c[1]]


def _flat(cases):
    return [(c[0], fam) for c in cases for fam in c[1]]


@pytest.mark.parametrize("cfg,fam", _flat(R.HIN_CASES), ids=_ids(R.HIN_CASES))
def test_hin_lrelu_forward_and_backward_elementwise_against_float64(cfg, fam):
    R.compare_hin(BE, cfg, fam, _w("hin"))
    _report("hin")


@pytest.mark.parametrize("shape,fam", _flat(R.FAC_CASES), ids=_ids(R.FAC_CASES))
def test_fac_bias_forward_and_backward_elementwise_against_float64(shape, fam):
    R.compare_fac(BE, shape, fam, _w("fac"))
    _report("fac")


@pytest.mark.parametrize("shape,fam", _flat(R.LN_FWD_CASES), ids=_ids(R.LN_FWD_CASES))
def test_layernorm2d_forward_elementwise_against_float64(shape, fam):
    R.compare_ln_fwd(BE, shape, fam, _w("ln_fwd"))
    _report("ln_fwd")


@pytest.mark.parametrize("mode", ["none", "res", "alias"])
@pytest.mark.parametrize("shape,fam", _flat(R.LN_BWD_CASES), ids=_ids(R.LN_BWD_CASES))
def test_layernorm2d_backward_elementwise_against_float64(shape, fam, mode):
    R.compare_ln_bwd(BE, shape, fam, mode, _w("ln_bwd"))
    _report("ln_bwd")


@pytest.mark.parametrize("shape", [(1, 83, 61, 128), (3, 5, 7, 16)], ids=lambda s: "x".join(map(str, s)))
def test_layernorm2d_backward_deferred_sums_are_bit_identical(shape):
    """The same call between rows_sum_defer() and rows_sum_flush(): the queued per-channel sums give the immediate form's bits."""
    a = R.compare_ln_bwd(BE, shape, "uniform", "res", {})
    be = HipBackend()
    be.defer = True
    b = R.compare_ln_bwd(be, shape, "uniform", "res", {})
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("shape,fam", _flat(R.DW_CASES), ids=_ids(R.DW_CASES))
def test_depthwise_gelu_forward_and_backward_elementwise_against_float64(shape, fam):
    """Both directions run twice (HipBackend): the second run's bits are the first's."""
    R.compare_dw(BE, shape, fam, _w("dw"))
    _report("dw")


@pytest.mark.parametrize("case", R.COLSUM_CASES, ids=lambda c: "x".join(map(str, c[0])) + f"-c{c[1]}")
def test_colsum_elementwise_against_float64(case):
    R.compare_colsum(BE, case, _w("colsum"))
    _report("colsum")


@pytest.mark.parametrize("shape", R.GS_CASES, ids=lambda s: "x".join(map(str, s)))
def test_gs_reduce_elementwise_against_float64(shape):
    R.compare_gs(BE, shape, _w("gs"))
    _report("gs")


@pytest.mark.parametrize("C,parts", R.SE_CASES)
def test_squeeze_excite_forward_and_backward_elementwise_against_float64(C, parts):
    R.compare_se(BE, C, parts, _w("se"))
    _report("se")


@pytest.mark.parametrize("want_grad", [True, False], ids=["grad", "nograd"])
@pytest.mark.parametrize("gscale", [1.0, R.f32s(1 / 3)], ids=["gs1", "gs3rd"])
@pytest.mark.parametrize("count", R.LOSS_COUNTS)
def test_charbonnier_elementwise_against_float64(count, gscale, want_grad):
    R.compare_charbonnier(BE, count, gscale, want_grad, _w("charbonnier"))
    _report("charbonnier")


@pytest.mark.parametrize("count", R.LOSS_COUNTS)
def test_grad_sqnorm_against_float64(count):
    R.compare_sqnorm(BE, count, _w("sqnorm"))
    _report("sqnorm")


@pytest.mark.parametrize("case", R.PSNR_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_psnr_loss_elementwise_against_float64(case):
    R.compare_psnr(BE, case, _w("psnr"))
    _report("psnr")


@pytest.mark.parametrize("case", R.ADAMW_CASES, ids=lambda c: f"n{c[0]}-{c[1]}-gs{c[2]:g}-p{c[3]:g}")
def test_clip_adamw_elementwise_against_float64_and_the_device_hyper_form(case):
    """Steps 1, 2 and 1000, each from the device's own fp32 state; clip_adamw_dev with hyper = [lr, bc1, sqrt(bc2)] on a copy of
    the same state must give clip_adamw's bits."""
    R.compare_adamw(BE, case, _w("adamw"), dev=BE.clip_adamw_dev)
    _report("adamw")
