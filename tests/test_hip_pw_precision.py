"""Element-wise precision contract of the register-operand pointwise tile (csrc/conv_pw.hip) and its EGACA fusions against float64.

For every output element o the gate is

    |got_o - ref_o| <= c * 2^-24 * S_o                       (test_hip_precision.check: first offender, worst ratio, NaN / inf fail)

with ref the float64 torch op on the CPU and S_o the float64 sum of the absolute values of the terms that meet in o: for a 1x1 conv
|x| conv |w| + |bias_o| + |res_o| (+ |res2_o|).  LeakyReLU is 1-Lipschitz, so S is taken at the pre-activation and a sign decision
that differs next to zero stays inside the bound; the mask factor (1 or slope_mask) multiplies value and error alike, so it
multiplies S.  Mask values keep 1e-3 away from zero, slopes are fp32 numbers: the reference makes the kernel's decisions on the
kernel's numbers.  Every tensor handed to a kernel is _fp32()-rounded first.

c = C_DOWN_FWD = 32, the project's constant for direct fp32-class forms at K = 512 .. 2048 (the pointwise K is at most 512).  The
six-bf16-product form (mfma_terms 6) claims the fp32 tile's distance from float64 and meets the same c.  A float32 restatement on
the CPU -- products rounded to fp32, strictly sequential fp32 accumulation along K, the same epilogue; for the LayerNorm chain a
two-pass fp32 mean / variance with sequential sums -- runs on the same data through the same check() with the same constants in
the tests WITHOUT the gpu marker: the bound describes fp32 arithmetic wherever `-m "not gpu"` runs.

Data families (a 1x1 conv mixes no pixels and fp32 is invariant under powers of two, so per-pixel and per-channel-compensated
scales give the ratios of (a) bit for bit -- they are not repeated here):
  (a) uniform O(1);
  (m) per-ELEMENT log-uniform magnitudes over 2^-20 .. 2^20: every K sum mixes magnitudes;
  (d) 95 % exact zeros, isolated values over 2^-10 .. 2^10;
  (t) family (a) times 2^-100 (bias and residual too): bf16 planes share fp32's exponent range.

Parts:
  1  the plain tile in every form the engine issues: forward and input gradient (transposed packing, co_base row ranges), fp32 and
     six products, full epilogue, channel-sliced operands (pitch != width, the untouched columns keep their fill value), the GELU'
     mask epilogue, ConvTranspose2d forward (pixel-shuffle store) and input gradient (patch GEMM with mask and second output);
  2  the fusions one at a time: LayerNorm prologue (+ ln_out, + GELU second output), squeeze-excite inside conv3;
  3  the EGACA block at the width that takes the fused path, forward and backward through the engine, against float64 autograd.

Bounds of part 2 (derived, not measured on the kernel):
  LayerNorm: T_k = |gamma_k| rstd (|x_k| + mean_j |x_j|) + |beta_k| dominates |LN(x)_k| and carries the error of the mean;
     ln_out within C_LN = 16 x 2^-24 T_k, the conv within 32 x 2^-24 (sum_k |w_ok| T_k + |b_o|);  GELU second output within
     1.13 x (the first output's bound) + 8 x 2^-24 (|v| + |GELU(v)|)   (1.13 > max |GELU'|).
  Squeeze-excite: sequential-sum bounds (n + 2) 2^-24 sum|terms| for the pooled mean (n = parts), z1 (n = C) and the sigmoid's
     argument (n = C / 2), each earlier stage's bound propagated through |W| (ReLU and sigmoid are 1- and 1/4-Lipschitz).  The
     sigmoid's own error: the kernel uses the hardware exponential, which has no project number; the allowance is SIG_MARGIN = 8
     times the worst error of numpy float32 1 / (1 + exp(-v)) against float64 on the SAME arguments (measured in the test:
     6.0e-8 .. 7.7e-8 on these cases, so the allowance is 4.8e-7 .. 6.1e-7 absolute on s in (0, 1)).  xs_out and the conv carry
     |x_k| ds + 2^-24 |x_k s_k| per operand, the conv the c = 32 product bound on top.
  GELU' mask epilogue: S |GELU'(m)| plus 8 x 2^-24 |v| for the derivative's own evaluation (v = the unmasked float64 result).

Part 3 is per tensor and max-normalised (autograd gives no per-element scale): the same block in torch float32 on the CPU sets the
unit, the HIP path may be at most E2E_MARGIN = 4 times its error against float64 plus 2^-22 (reductions over up to 8192 pixels
in another order).

MEASURED (worst err / (2^-24 S) over every case of a test)
  float32 restatement on the CPU: plain product 10.7 (family m, 80 channels); two-pass LayerNorm 11.7 against T (one channel hot,
  C = 64), conv after it 5.0, GELU output 3.8 (of c = 32).
  MI355X: forward 12.7 (fp32 products) / 13.1 (six products); input gradient 12.2 / 11.7; with the GELU' mask
  8.0 / 8.1; ConvTranspose2d forward 13.0, input gradient 12.2, its second output 11.7 -- all on family m, at most 3.5 on (a);
  LayerNorm ln_out 7.5 against T (one channel hot), conv after it 4.8, GELU output 3.9; squeeze-excite: m, z1, s and xs_out use
  at most 0.25, 0.09, 0.03 and 0.04 of their bounds, the conv output 1.4.  EGACA block: the worst tensor against its bar is se_1.1.bias hip 2.659e-07 torch float32 1.114e-07
  (0.39 of 4 x float32 + 2^-22).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_hip_precision import C_DOWN_FWD, EPS, _fp32, _gen, check, nchw, nhwc

C_PW = C_DOWN_FWD            # 32: the project's constant for direct fp32-class forms
C_LN = 16.0                  # ln_out against T
GELU_LIP = 1.13              # > max |GELU'| = 1.1289
C_GELU = 8.0                 # evaluation of GELU / GELU' in fp32 (erff, __expf), in units of 2^-24 of the values it combines
SIG_MARGIN = 8.0             # kernel sigmoid (hardware exponential) vs numpy float32 sigmoid
E2E_MARGIN = 4.0
E2E_ABS = 2.0 ** -22
FAMILIES = ["a", "m", "d", "t"]
SL_PRE, SL_POST, SL_MASK = (float(np.float32(v)) for v in (0.2, 0.5, 0.3))
LN_EPS = float(np.float32(1e-6))
FILL = 7.0


def _ops():
    from refid_amd import ops
    return ops


def _cdiv(a, b):
    return -(-a // b)


def _uni(seed, *shape):
    return torch.rand(*shape, generator=_gen(seed, *shape), dtype=torch.float64) * 2 - 1


def lrelu(x, s):
    return torch.where(x > 0, x, x * s)


# ---- data ------------------------------------------------------------------------------------------------------------------
def family_scale(fam):
    """Magnitude of bias / residual next to the family's products (so they never drown the K sum)."""
    return {"a": 1.0, "m": 1.0, "d": 2.0 ** -6, "t": 2.0 ** -100}[fam]


def make_operand(fam, shape, seed):
    """NCHW float64 tensor of fp32 numbers: the conv's operand (activations, or the output gradient of an input gradient)."""
    x = _uni(seed + 1, *shape)
    if fam == "m":
        x = x * torch.exp2(torch.rand(*shape, generator=_gen(seed + 3, *shape), dtype=torch.float64) * 40 - 20)
    elif fam == "d":
        keep = torch.rand(*shape, generator=_gen(seed + 4, *shape), dtype=torch.float64) < 0.05
        r = torch.rand(*shape, generator=_gen(seed + 5, *shape), dtype=torch.float64) * 20 - 10
        x = torch.where(keep, x * torch.exp2(r), torch.zeros_like(x))
    elif fam == "t":
        x = x * 2.0 ** -100
    else:
        assert fam == "a", fam
    return _fp32(x)


def make_weight(co, ci, seed):
    return _fp32(_uni(seed + 2, co, ci) / math.sqrt(ci))


def make_mask(shape, seed):
    u = _uni(seed + 6, *shape)
    return _fp32(torch.where(u >= 0, u + 1e-3, u - 1e-3))          # no value within 1e-3 of zero


def conv1x1(x, w):
    return F.conv2d(x, w[:, :, None, None])


def epilogue_ref(v, S, b, r, m, sl=(1.0, 1.0, 1.0)):
    """float64 mask(post(pre(v + b) + r)) and its error scale (S at the pre-activation, times the mask factor)."""
    if b is not None:
        v, S = v + b.view(1, -1, 1, 1), S + b.abs().view(1, -1, 1, 1)
    v = lrelu(v, sl[0])
    if r is not None:
        v, S = v + r, S + r.abs()
    v = lrelu(v, sl[1])
    if m is not None:
        f = torch.where(m > 0, torch.ones_like(m), torch.full_like(m, sl[2]))
        v, S = v * f, S * f
    return v, S


# ---- float32 restatements on the CPU ---------------------------------------------------------------------------------------
def f32_matmul_seq(x, w):
    """NCHW x (fp32 numbers) times w (R, K): every product rounded to fp32, strictly sequential fp32 accumulation along K."""
    N, K, H, W = x.shape
    xf = x.permute(0, 2, 3, 1).reshape(-1, K).float()
    wf = w.float()
    acc = torch.zeros(xf.shape[0], wf.shape[0], dtype=torch.float32)
    for k in range(K):
        acc = acc + xf[:, k:k + 1] * wf[:, k].unsqueeze(0)
    return acc.view(N, H, W, -1).permute(0, 3, 1, 2)


def f32_epilogue(v, b, r, m, sl=(1.0, 1.0, 1.0)):
    one = torch.ones((), dtype=torch.float32)
    if b is not None:
        v = v + b.float().view(1, -1, 1, 1)
    v = torch.where(v > 0, v, v * torch.tensor(sl[0], dtype=torch.float32))
    if r is not None:
        v = v + r.float()
    v = torch.where(v > 0, v, v * torch.tensor(sl[1], dtype=torch.float32))
    if m is not None:
        v = v * torch.where(m.float() > 0, one, torch.tensor(sl[2], dtype=torch.float32))
    assert v.dtype == torch.float32
    return v.double()


def f32_layernorm_two_pass(x, g, b):
    """fp32 LayerNorm over the channel axis of NCHW x: sequential sums, mean first, variance of the differences."""
    xf = x.float()
    C = x.shape[1]
    s1 = torch.zeros_like(xf[:, 0])
    for k in range(C):
        s1 = s1 + xf[:, k]
    mu = (s1 / C).unsqueeze(1)
    d = xf - mu
    s2 = torch.zeros_like(s1)
    for k in range(C):
        s2 = s2 + d[:, k] * d[:, k]
    rstd = (1.0 / torch.sqrt(s2 / C + torch.tensor(LN_EPS, dtype=torch.float32))).unsqueeze(1)
    y = d * rstd * g.float().view(1, -1, 1, 1) + b.float().view(1, -1, 1, 1)
    assert y.dtype == torch.float32
    return y


# ---- device helpers --------------------------------------------------------------------------------------------------------
class Dev:
    """An NCHW float64 tensor as an NHWC float32 device tensor; wide: as a channel slice [lead, lead + C) of a buffer that is
    8 channels wider (C % 4 != 0: padded up to a multiple of 4), the other columns holding `fill`."""

    def __init__(self, t=None, wide=False, fill=float("nan"), shape=None):
        d = nhwc(t) if t is not None else torch.full(shape, fill, device="cuda")
        N, H, W, C = d.shape
        self.buf, self.fill, self.C = None, fill, C
        if C % 4:
            wide, lead, total = True, 0, _cdiv(C, 4) * 4
        else:
            lead, total = 4, C + 8
        if wide:
            self.buf = torch.full((N, H, W, total), fill, device="cuda")
            self.lead = lead
            self.t = self.buf[..., lead:lead + C]
            self.t.copy_(d)
        else:
            self.t = d

    def get(self):
        return nchw(self.t)

    def assert_untouched(self, what):
        if self.buf is None:
            return
        side = torch.cat([self.buf[..., :self.lead], self.buf[..., self.lead + self.C:]], -1)
        same = torch.isnan(side) if math.isnan(self.fill) else side == self.fill
        assert bool(same.all()), f"{what}: columns outside the channel slice were written"


def _t(d):
    return d.t if d is not None else None


def run_tile(x, w, *, role="fwd", form="fp32", ca=None, rows=None, bias=None, res=None, mask=None, sl=(1.0, 1.0, 1.0),
             mask_mode=0, wide=False, pw=None):
    """The pointwise tile (refid_conv2d algo 3).  role fwd: out = w [x_a | x_b]; role dgrad: x is the output gradient, the rows
    [base, base + cnt) of w^T are computed.  Returns the NCHW float64 result."""
    ops = _ops()
    co, ci = w.shape
    w4 = w.float().view(co, ci, 1, 1).cuda().contiguous()
    r = ops.ROLE_FWD if role == "fwd" else ops.ROLE_DGRAD
    nrows = co if role == "fwd" else ci
    wp = ops.pack_conv_weights_split(w4, r, 32, 1, 1, co, ci, planes=3) if form == "six" else \
        ops.pack_conv_weights(w4, r, 32, 8, 1, 1, co, ci)
    base, cnt = rows if rows is not None else (0, nrows)
    N, C, H, W = x.shape
    ca = ca or C
    xa = Dev(x[:, :ca], wide)
    xb = Dev(x[:, ca:], wide) if ca < C else None
    out = Dev(shape=(N, H, W, cnt), wide=wide, fill=FILL)
    rd = Dev(res, wide) if res is not None else None
    md = Dev(mask, wide) if mask is not None else None
    ops.conv2d(xa.t, wp, out.t, kh=1, kw=1, cout=cnt, cout_pad=_cdiv(nrows, 32) * 32, co_base=base, algo=3,
               terms=6 if form == "six" else 0, in_b=_t(xb), bias=bias.float().cuda() if bias is not None else None, res=_t(rd),
               mask=_t(md), slope_pre=sl[0], slope_post=sl[1], slope_mask=sl[2], mask_mode=mask_mode, pw=pw)
    torch.cuda.synchronize()
    out.assert_untouched(f"pointwise {role} {form}")
    return out.get()


def six_ok(ctot, ca, cout):
    """conv_pw.hip's argument rule for mfma_terms 6: channel counts multiples of 16, more than 32 outputs."""
    return ctot % 16 == 0 and (ca == ctot or ca % 16 == 0) and cout > 32


# ---- (1) the plain tile ----------------------------------------------------------------------------------------------------
PLAIN_CASES = [
    # (N, H, W, Ca, Cb, Co, wide)
    (1, 4, 8, 8, 0, 64, False),            # one wave, one 8-channel chunk
    (3, 5, 7, 72, 0, 48, True),            # 105 pixels: partial wave / workgroup across samples; 9 chunks: the ring of 8 wraps by one
    (2, 16, 16, 40, 24, 80, True),         # the source switches inside a ring turn; two column tiles, the second partial
    (1, 9, 11, 256, 256, 256, False),      # K = 512: eight ring turns, four column tiles
    (2, 16, 24, 136, 0, 32, False),        # the <1, 8> instantiation (Cout <= 32): its 16-chunk ring wraps by one
    (2, 9, 13, 32, 0, 3, False),           # pred's width: the scalar (non-16-byte) epilogue, pitch 4
    (3, 5, 7, 80, 0, 48, True),            # six-product twin of the 72-channel case: 10 chunks, the ring wraps by a chunk pair
    (2, 16, 16, 48, 16, 80, False),        # six-product twin of the 40 | 24 case: the source switches inside a ring turn
    (2, 128, 128, 64, 64, 64, False),      # configs[1] level 1 (fuse_two_dir) at its real size: 256 workgroups
    (2, 64, 64, 128, 0, 128, False),       # level 2
]


def _case_id(c):
    return "%dx%dx%d-%d+%dto%d%s" % (c[0], c[1], c[2], c[3], c[4], c[5], "-sliced" if len(c) > 6 and c[6] else "")


def plain_data(case, family, seed=41):
    N, H, W, Ca, Cb, Co = case[:6]
    Ci = Ca + Cb
    e = family_scale(family)
    x = make_operand(family, (N, Ci, H, W), seed)
    w = make_weight(Co, Ci, seed)
    b = _fp32(_uni(seed + 7, Co) * e)
    r = _fp32(_uni(seed + 8, N, Co, H, W) * e)
    m = make_mask((N, Co, H, W), seed)
    return x, w, b, r, m


def plain_ref(x, w, b, r, m, sl):
    return epilogue_ref(conv1x1(x, w), conv1x1(x.abs(), w.abs()), b, r, m, sl)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", PLAIN_CASES, ids=_case_id)
def test_pointwise_forward_elementwise_against_float64(case, family):
    N, H, W, Ca, Cb, Co, wide = case
    sl = (SL_PRE, SL_POST, SL_MASK)
    x, w, b, r, m = plain_data(case, family)
    ref, S = plain_ref(x, w, b, r, m, sl)
    for form in ["fp32"] + (["six"] if six_ok(Ca + Cb, Ca, Co) else []):
        got = run_tile(x, w, form=form, ca=Ca, bias=b, res=r, mask=m, sl=sl, wide=wide)
        worst = check(got, ref, S, C_PW, f"pointwise forward {form} {_case_id(case)} family {family}")
        print(f"pw fwd {form} {_case_id(case)} {family}: worst {worst:.3g}")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", PLAIN_CASES, ids=_case_id)
def test_float32_restatement_of_the_product_meets_the_bound(case, family):
    """Products rounded to fp32, sequential fp32 accumulation along K, the tile's epilogue -- on the GPU test's data (the first
    2048 pixels of the two train-size cases), through the same check() with the same c."""
    sl = (SL_PRE, SL_POST, SL_MASK)
    x, w, b, r, m = plain_data(case, family)
    if x.shape[0] * x.shape[2] * x.shape[3] > 2048:
        rows = 2048 // x.shape[3]
        x, r, m = x[:1, :, :rows], r[:1, :, :rows], m[:1, :, :rows]
    ref, S = plain_ref(x, w, b, r, m, sl)
    got = f32_epilogue(f32_matmul_seq(x, w), b, r, m, sl)
    worst = check(got, ref, S, C_PW, f"float32 restatement {_case_id(case)} family {family}")
    print(f"pw restatement {_case_id(case)} {family}: worst {worst:.3g}")


DGRAD_CASES = [
    (3, 5, 7, 72, 0, 48, True),
    (2, 16, 16, 40, 24, 80, True),         # both halves; the second (24 rows from row 40) on the <1, 8> instantiation
    (1, 9, 11, 256, 256, 256, False),
    (2, 128, 128, 64, 64, 64, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", DGRAD_CASES, ids=_case_id)
def test_pointwise_input_gradient_elementwise_against_float64(case, family):
    """The transposed packing issued as co_base row ranges (both halves of a two-source conv), with residual and mask."""
    N, H, W, Ca, Cb, Co, wide = case
    Ci = Ca + Cb
    e = family_scale(family)
    g = make_operand(family, (N, Co, H, W), 51)
    w = make_weight(Co, Ci, 51)
    xin = torch.zeros(N, Ci, H, W, dtype=torch.float64, requires_grad=True)
    conv1x1(xin, w).backward(g)                             # reference: autograd of the float64 conv
    full, fullS = xin.grad, conv1x1(g.abs(), w.abs().t().contiguous())
    for base, cnt in [(0, Ca)] + ([(Ca, Cb)] if Cb else []):
        r = _fp32(_uni(58 + base, N, cnt, H, W) * e)
        m = make_mask((N, cnt, H, W), 51 + base)
        ref, S = epilogue_ref(full[:, base:base + cnt], fullS[:, base:base + cnt], None, r, m, (1.0, 1.0, SL_MASK))
        for form in ["fp32"] + (["six"] if six_ok(Co, Co, cnt) else []):
            got = run_tile(g, w, role="dgrad", form=form, rows=(base, cnt), res=r, mask=m, sl=(1.0, 1.0, SL_MASK), wide=wide)
            worst = check(got, ref, S, C_PW, f"pointwise input gradient {form} rows {base}+{cnt} {_case_id(case)} family {family}")
            print(f"pw dgrad {form} rows {base}+{cnt} {_case_id(case)} {family}: worst {worst:.3g}")


def gelu_d(m):
    return 0.5 * (1.0 + torch.erf(m / math.sqrt(2.0))) + m * torch.exp(-0.5 * m * m) / math.sqrt(2.0 * math.pi)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", [(3, 5, 7, 72, 48), (2, 64, 64, 128, 64)], ids=lambda c: "%dx%dx%d-%dfrom%d" % c)
def test_pointwise_input_gradient_gelu_mask_elementwise_against_float64(case, family):
    """mask_mode 1: the input gradient times GELU'(stashed pre-activation), mask values spread over [-6, 6] (conv5's input
    gradient in EGACA).  S |GELU'(m)| + (C_GELU / c) |v|: the second term is the derivative's own fp32 evaluation."""
    N, H, W, Ci, Co = case
    g = make_operand(family, (N, Co, H, W), 61)
    w = make_weight(Co, Ci, 61)
    m = _fp32(_uni(66, N, Ci, H, W) * 6.0)
    v = conv1x1(g, w.t().contiguous())
    d = gelu_d(m)
    ref = v * d
    S = conv1x1(g.abs(), w.abs().t().contiguous()) * d.abs() + (C_GELU / C_PW) * v.abs()
    for form in ["fp32"] + (["six"] if six_ok(Co, Co, Ci) else []):
        got = run_tile(g, w, role="dgrad", form=form, mask=m, mask_mode=1)
        worst = check(got, ref, S, C_PW, f"pointwise input gradient x GELU' {form} family {family}")
        print(f"pw dgrad gelu {form} {case} {family}: worst {worst:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", [(2, 64, 64, 128, 64), (2, 5, 20, 128, 64)], ids=lambda c: "%dx%dx%d-%dto%d" % c)
def test_conv_transpose_on_the_pointwise_tile_elementwise_against_float64(case, family):
    """ConvTranspose2d(2, 2): forward as the pixel-shuffle store (mode 1: bias per real channel, residual, slope_post), input
    gradient as one patch GEMM with mask and second output -- against F.conv_transpose2d and its autograd in float64."""
    ops = _ops()
    N, H, W, Ci, Co = case
    e = family_scale(family)
    x = make_operand(family, (N, Ci, H, W), 71).requires_grad_(True)
    w = _fp32(_uni(72, Ci, Co, 2, 2) / math.sqrt(Ci))
    b = _fp32(_uni(73, Co) * e)
    r = _fp32(_uni(74, N, Co, 2 * H, 2 * W) * e)
    y = F.conv_transpose2d(x, w, None, stride=2)
    S = F.conv_transpose2d(x.detach().abs(), w.abs(), None, stride=2)
    ref, S = epilogue_ref(y.detach(), S, b, r, None, (1.0, SL_PRE, 1.0))
    wc = w.float().cuda().contiguous()
    wq = ops.pack_conv_weights(wc, ops.ROLE_CONVT, 32, 8, 2, 2, Co, Ci)
    out = torch.full((N, 2 * H, 2 * W, Co), float("nan"), device="cuda")
    ops.conv2d(nhwc(x.detach()), wq, out, kh=1, kw=1, stride=1, pad=0, mode=1, cout=4 * Co, cout_pad=_cdiv(4 * Co, 32) * 32,
               bias=b.float().cuda(), res=nhwc(r), slope_post=SL_PRE, algo=3)
    worst = check(nchw(out), ref, S, C_PW, f"ConvTranspose2d forward on the pointwise tile, family {family}")
    print(f"convT fwd {case} {family}: worst {worst:.3g}")
    # input gradient: the operand is the high-resolution output gradient
    g = make_operand(family, (N, Co, 2 * H, 2 * W), 75)
    y.backward(g)
    m = make_mask((N, Ci, H, W), 76)
    plus = _fp32(_uni(77, N, Ci, H, W) * e)
    Sg = F.conv2d(g.abs(), w.abs(), None, stride=2)
    ref, Sg = epilogue_ref(x.grad, Sg, None, None, m, (1.0, 1.0, SL_MASK))
    wq = ops.pack_conv_weights(wc, ops.ROLE_CONVT_DGRAD_PW, 32, 8, 2, 2, Co, Ci)
    dx = torch.full((N, H, W, Ci), float("nan"), device="cuda")
    o2 = torch.full((N, H, W, Ci), float("nan"), device="cuda")
    ops.conv2d(nhwc(g), wq, dx, kh=2, kw=2, stride=2, pad=0, cout=Ci, cout_pad=_cdiv(Ci, 32) * 32, algo=3, mask=nhwc(m),
               slope_mask=SL_MASK, add2=nhwc(plus), out2=o2)
    worst = check(nchw(dx), ref, Sg, C_PW, f"ConvTranspose2d input gradient (patch GEMM), family {family}")
    worst2 = check(nchw(o2), ref + plus, Sg + plus.abs(), C_PW, f"ConvTranspose2d input gradient, second output, family {family}")
    print(f"convT dgrad {case} {family}: worst {worst:.3g}, second output {worst2:.3g}")


# ---- (2) LayerNorm prologue ------------------------------------------------------------------------------------------------
LN_KINDS = ["uniform", "mean100", "mean1e4", "spread1e-5", "3+1e-4u", "logmag", "hot-channel"]
LN_SHAPES = [(3, 5, 7), (2, 64, 64)]


def ln_data(kind, N, C, H, W, seed=81):
    u = _uni(seed, N, C, H, W)
    if kind == "uniform":
        x = u
    elif kind == "mean100":
        x = 100.0 + u                          # a one-pass variance E[x^2] - mu^2 loses 4 digits here ...
    elif kind == "mean1e4":
        x = 1e4 + u                            # ... and everything here
    elif kind == "spread1e-5":
        x = 1e-5 * u                           # variance far below eps: rstd ~ 1000
    elif kind == "3+1e-4u":
        x = 3.0 + 1e-4 * u
    elif kind == "logmag":
        x = u * torch.exp2(torch.rand(N, 1, H, W, generator=_gen(seed + 1, N, H, W), dtype=torch.float64) * 20 - 10)
    else:
        assert kind == "hot-channel", kind
        x = u.clone()
        x[:, C // 3] *= 1e4
    return _fp32(x)


def ln_case(kind, shape, C, Co):
    N, H, W = shape
    x = ln_data(kind, N, C, H, W)
    gam = _fp32(1.0 + 0.3 * _uni(82, C))
    bet = _fp32(_uni(83, C))
    w = make_weight(Co, C, 84)
    b = _fp32(_uni(85, Co))
    return x, gam, bet, w, b


def ln_ref(x, gam, bet, w, b):
    """float64 LN(x), conv(LN(x)) + b and their error scales T, sum_k |w_ok| T_k + |b_o|."""
    mu = x.mean(1, keepdim=True)
    d = x - mu
    rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + LN_EPS)
    y = d * rstd * gam.view(1, -1, 1, 1) + bet.view(1, -1, 1, 1)
    T = gam.abs().view(1, -1, 1, 1) * rstd * (x.abs() + x.abs().mean(1, keepdim=True)) + bet.abs().view(1, -1, 1, 1)
    return y, T, conv1x1(y, w) + b.view(1, -1, 1, 1), conv1x1(T, w.abs()) + b.abs().view(1, -1, 1, 1)


def gelu_bound(v, Sv):
    """float64 GELU(v) and its scale in units of C_PW 2^-24: GELU_LIP Sv + (C_GELU / C_PW) (|v| + |GELU(v)|)."""
    gl = F.gelu(v)
    return gl, GELU_LIP * Sv + (C_GELU / C_PW) * (v.abs() + gl.abs())


def run_ln(x, gam, bet, w, b, form, want_gelu):
    N, C, H, W = x.shape
    ln_out = Dev(shape=(N, H, W, C), wide=True, fill=float("nan"))
    pw = dict(ln_gamma=gam.float().cuda(), ln_beta=bet.float().cuda(), ln_eps=LN_EPS, ln_out=ln_out.t)
    out2 = None
    if want_gelu:
        out2 = torch.full((N, H, W, w.shape[0]), float("nan"), device="cuda")
        pw["out2"] = out2
    out = run_tile(x, w, form=form, bias=b, pw=pw, wide=True)
    ln_out.assert_untouched("ln_out")
    return out, ln_out.get(), nchw(out2) if want_gelu else None


@pytest.mark.gpu
@pytest.mark.parametrize("kind", LN_KINDS)
@pytest.mark.parametrize("C,Co", [(40, 64), (40, 128), (64, 64), (64, 128)])
@pytest.mark.parametrize("shape", LN_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_layernorm_prologue_elementwise_against_float64(shape, C, Co, kind):
    """conv(LN(x)) with the normalised tensor as a side output (conv1 / conv1_e of EGACA)."""
    x, gam, bet, w, b = ln_case(kind, shape, C, Co)
    y, T, ref, S = ln_ref(x, gam, bet, w, b)
    for form in ["fp32"] + (["six"] if six_ok(C, C, Co) else []):
        out, ln_out, _ = run_ln(x, gam, bet, w, b, form, False)
        w1 = check(ln_out, y, T, C_LN, f"LayerNorm prologue {form}: ln_out, {kind}, C = {C}")
        w2 = check(out, ref, S, C_PW, f"LayerNorm prologue {form}: conv(LN(x)), {kind}, {C} -> {Co}")
        print(f"ln {form} {shape} {C}->{Co} {kind}: ln_out {w1:.3g}, conv {w2:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", LN_KINDS)
@pytest.mark.parametrize("shape", LN_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_layernorm_prologue_with_gelu_second_output_against_float64(shape, kind):
    """conv4's form: LayerNorm prologue, out = conv(LN(x)) + b, out2 = GELU(out)."""
    C, Co = 64, 128
    x, gam, bet, w, b = ln_case(kind, shape, C, Co)
    y, T, ref, S = ln_ref(x, gam, bet, w, b)
    gl, Sg = gelu_bound(ref, S)
    out, ln_out, out2 = run_ln(x, gam, bet, w, b, "fp32", True)
    w1 = check(ln_out, y, T, C_LN, f"LayerNorm + GELU output: ln_out, {kind}")
    w2 = check(out, ref, S, C_PW, f"LayerNorm + GELU output: conv(LN(x)), {kind}")
    w3 = check(out2, gl, Sg, C_PW, f"LayerNorm + GELU output: GELU(conv(LN(x))), {kind}")
    print(f"ln+gelu {shape} {kind}: ln_out {w1:.3g}, conv {w2:.3g}, gelu {w3:.3g}")


@pytest.mark.parametrize("kind", LN_KINDS)
@pytest.mark.parametrize("C,Co", [(40, 64), (64, 128)])
@pytest.mark.parametrize("shape", LN_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_float32_restatement_of_the_layernorm_chain_meets_the_bounds(shape, C, Co, kind):
    """Two-pass fp32 LayerNorm, sequential fp32 conv, fp32 GELU on the GPU tests' data (the first 2048 pixels of the large
    shape): the bounds of the LayerNorm tests describe fp32 arithmetic."""
    x, gam, bet, w, b = ln_case(kind, shape, C, Co)
    if x.shape[0] * x.shape[2] * x.shape[3] > 2048:
        x = x[:1, :, :2048 // x.shape[3]]
    y, T, ref, S = ln_ref(x, gam, bet, w, b)
    gl, Sg = gelu_bound(ref, S)
    y32 = f32_layernorm_two_pass(x, gam, bet)
    o32 = f32_matmul_seq(y32.double(), w) + b.float().view(1, -1, 1, 1)
    assert o32.dtype == torch.float32
    w1 = check(y32.double(), y, T, C_LN, f"float32 two-pass LayerNorm, {kind}, C = {C}")
    w2 = check(o32.double(), ref, S, C_PW, f"float32 conv(LN(x)), {kind}, {C} -> {Co}")
    w3 = check(F.gelu(o32).double(), gl, Sg, C_PW, f"float32 GELU(conv(LN(x))), {kind}")
    print(f"ln restatement {shape} {C}->{Co} {kind}: ln_out {w1:.3g}, conv {w2:.3g}, gelu {w3:.3g}")


def test_one_pass_variance_would_miss_the_layernorm_bound():
    """The data has teeth: the same fp32 restatement with the variance as E[x^2] - mu^2 misses C_LN on the mean-1e4 case."""
    x, gam, bet, w, b = ln_case("mean1e4", (3, 5, 7), 64, 64)
    y, T, _, _ = ln_ref(x, gam, bet, w, b)
    xf = x.float()
    mu = xf.mean(1, keepdim=True)
    var = (xf * xf).mean(1, keepdim=True) - mu * mu
    y32 = (xf - mu) / torch.sqrt(var.clamp_min(0) + LN_EPS) * gam.float().view(1, -1, 1, 1) + bet.float().view(1, -1, 1, 1)
    with pytest.raises(AssertionError, match="ln_out"):
        check(y32.double(), y, T, C_LN, "one-pass ln_out")


# ---- (2) squeeze-excite inside conv3 ---------------------------------------------------------------------------------------
SE_C = 64
SE_LEVELS = (-1.0, 0.3, 1.6)                 # pooled means of the samples: O(1) apart
SE_CASES = [
    # (N, H, W, parts): parts "real" = the partials of ops.dwconv3x3_gelu_fwd(..., want_pool=True)
    (3, 8, 16, 1), (3, 8, 16, 7), (3, 8, 16, 256), (2, 128, 128, 7), (2, 128, 128, "real"),
]


def se_weights(seed=91):
    """W1 > 0 and W2 of one sign per output channel, so the sigmoid's argument moves with the pooled mean in every channel."""
    C, Ch = SE_C, SE_C // 2
    W1 = _fp32((_uni(seed, Ch, C).abs() + 0.1) / (0.6 * C))
    b1 = _fp32(_uni(seed + 1, Ch) * 0.5)
    sgn = torch.where(_uni(seed + 2, C, 1) >= 0, 1.0, -1.0).double()
    W2 = _fp32(sgn * (_uni(seed + 3, C, Ch).abs() + 0.1) / (0.15 * Ch))
    b2 = _fp32(_uni(seed + 4, C) * 0.5)
    return W1, b1, W2, b2


def se_ref(pool, hw, W1, b1, W2, b2):
    """float64 m, z1, s of the squeeze-excite branch from pool partials (N, parts, C), with their error bounds (absolute)."""
    N, parts, C = pool.shape
    m = pool.sum(1) / hw
    dm = (parts + 2) * EPS * pool.abs().sum(1) / hw
    z1p = m @ W1.t() + b1
    dz = (C + 2) * EPS * (m.abs() @ W1.abs().t() + b1.abs()) + dm @ W1.abs().t()
    z1 = F.relu(z1p)
    v = z1 @ W2.t() + b2
    dv = (C // 2 + 2) * EPS * (z1.abs() @ W2.abs().t() + b2.abs()) + dz @ W2.abs().t()
    s = torch.sigmoid(v)
    v32 = v.numpy().astype(np.float32)
    s32 = np.float32(1.0) / (np.float32(1.0) + np.exp(-v32))
    assert s32.dtype == np.float32
    e_sig = float(np.abs(s32.astype(np.float64) - s.numpy()).max())
    ds = 0.25 * dv + SIG_MARGIN * e_sig
    return dict(m=m, dm=dm, z1p=z1p, z1=z1, dz=dz, v=v, s=s, ds=ds, e_sig=e_sig)


def se_inputs(case):
    """(xi, xe, pool partials (N, parts, C) float64 of fp32 numbers); the 'real' case runs the depthwise kernel for xe and pool."""
    N, H, W, parts = case
    C = SE_C
    xi = _fp32(_uni(101, N, C, H, W))
    lev = torch.tensor(SE_LEVELS[:N] if N == 3 else (SE_LEVELS[0], SE_LEVELS[2]), dtype=torch.float64)
    if parts == "real":
        ops = _ops()
        c1e = _fp32(_uni(102, N, C, H, W) + 1.5 * lev.view(N, 1, 1, 1))
        wd = _fp32((_uni(103, C, 1, 3, 3).abs() + 0.2) / 6.0)
        bd = _fp32(_uni(104, C) * 0.1)
        _, act, pool = ops.dwconv3x3_gelu_fwd(nhwc(c1e), wd.float().cuda(), bd.float().cuda(), want_pool=True)
        assert pool.shape[1] == ops.dwconv_pool_parts(H, W, C) <= 256
        return xi, nchw(act), pool.double().cpu()
    xe = _fp32(_uni(105, N, C, H, W))
    base = lev.view(N, 1, 1) + 0.3 * _uni(106, N, 1, C)
    pool = _fp32((base + 0.5 * _uni(107, N, parts, C)) * (H * W / parts))
    return xi, xe, pool


@pytest.mark.gpu
@pytest.mark.parametrize("case", SE_CASES, ids=lambda c: "%dx%dx%d-%s-parts" % c)
def test_squeeze_excite_inside_conv3_elementwise_against_float64(case):
    """y = res + res2 + conv3([xi s | xe s]) + b with s computed per workgroup from the pool partials of ITS sample; the side
    outputs the backward pass reads (m, z1, s, the scaled operand) are NaN before the launch and complete after it."""
    ops = _ops()
    N, H, W, parts = case
    C, hw = SE_C, H * W
    xi, xe, pool = se_inputs(case)
    W1, b1, W2, b2 = se_weights()
    R = se_ref(pool, hw, W1, b1, W2, b2)
    # conditions on the INPUT, checked on the float64 reference: the ReLU kink is not within 1e-3 of any pre-activation, and
    # every channel of s differs by more than 0.1 between any two samples (a workgroup that read a neighbour's s must fail)
    assert float(R["z1p"].abs().min()) >= 1e-3, float(R["z1p"].abs().min())
    gaps = [float((R["s"][i] - R["s"][j]).abs().min()) for i in range(N) for j in range(i)]
    assert min(gaps) > 0.1, gaps
    assert bool((R["z1"] > 0).any()) and bool((R["z1"] == 0).any())      # both sides of the ReLU are exercised
    w = make_weight(C, 2 * C, 111)
    b = _fp32(_uni(112, C))
    ev = _fp32(_uni(113, N, C, H, W))
    img = _fp32(_uni(114, N, C, H, W))
    sv = R["s"].view(N, C, 1, 1)
    x = torch.cat([xi, xe], 1)
    xs = torch.cat([xi * sv, xe * sv], 1)
    ds = R["ds"].view(N, C, 1, 1).repeat(1, 2, 1, 1)
    exs = x.abs() * ds + EPS * xs.abs()                               # error of one scaled operand
    ref = conv1x1(xs, w) + b.view(1, -1, 1, 1) + ev + img
    S = conv1x1(xs.abs(), w.abs()) + b.abs().view(1, -1, 1, 1) + ev.abs() + img.abs() + conv1x1(exs, w.abs()) / (C_PW * EPS)
    dev = lambda t: t.float().cuda().contiguous()                     # noqa: E731
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")       # noqa: E731
    se_m, se_z1, se_s = nan(N, C), nan(N, C // 2), nan(N, C)
    xs_out = Dev(shape=(N, H, W, 2 * C), wide=True, fill=float("nan"))
    res2 = Dev(img, wide=True)
    pw = dict(pool=dev(pool), hw=hw, se_w1=dev(W1), se_b1=dev(b1), se_w2=dev(W2), se_b2=dev(b2), se_m=se_m, se_z1=se_z1,
              se_s=se_s, xs_out=xs_out.t, res2=res2.t)
    got = run_tile(x, w, ca=C, bias=b, res=ev, pw=pw)
    what = f"squeeze-excite in conv3, {N} x {H} x {W}, {parts} parts"
    wm = check(se_m.double().cpu(), R["m"], R["dm"] / EPS, 1.0, what + ": se_m")
    wz = check(se_z1.double().cpu(), R["z1"], R["dz"] / EPS, 1.0, what + ": se_z1")
    ws = check(se_s.double().cpu(), R["s"], R["ds"] / EPS, 1.0, what + ": se_s")
    wx = check(xs_out.get(), xs, exs / EPS, 1.0, what + ": xs_out")
    xs_out.assert_untouched("xs_out")
    wo = check(got, ref, S, C_PW, what + ": output")
    print(f"se {case}: numpy float32 sigmoid error {R['e_sig']:.3g}; fraction of the bound used: m {wm:.3g}, z1 {wz:.3g}, "
          f"s {ws:.3g}, xs_out {wx:.3g}; output worst / (2^-24 S) {wo:.3g}")


# ---- (3) the EGACA block through the engine, forward and backward ----------------------------------------------------------
EGACA_PREFIX = "encoders_forward.1.atten_fuse"


def _egaca_any_dtype(P, a, ev, img):
    """test_hip_egaca._egaca_ref with the parameters taken as they are (float32 or float64): the float32 yardstick."""
    g = lambda k: P[f"{a}.{k}"]                                                # noqa: E731

    def ln(x, n):
        mu = x.mean(1, keepdim=True)
        var = (x - mu).pow(2).mean(1, keepdim=True)
        return g(n + ".weight").view(1, -1, 1, 1) * ((x - mu) / (var + 1e-6).sqrt()) + g(n + ".bias").view(1, -1, 1, 1)

    c = ev.shape[1]
    xi = F.gelu(F.conv2d(F.conv2d(ln(img, "norm1"), g("conv1.weight"), g("conv1.bias")), g("conv2.weight"), g("conv2.bias"),
                         padding=1, groups=c))
    xe = F.gelu(F.conv2d(F.conv2d(ln(ev, "norm1_e"), g("conv1_e.weight"), g("conv1_e.bias")), g("conv2_e.weight"),
                         g("conv2_e.bias"), padding=1, groups=c))
    m = xe.mean((2, 3), keepdim=True)
    s = torch.sigmoid(F.conv2d(F.relu(F.conv2d(m, g("se_1.1.weight"), g("se_1.1.bias"))), g("se_1.3.weight"), g("se_1.3.bias")))
    zf = F.conv2d(torch.cat([xi * s, xe * s], 1), g("conv3.weight"), g("conv3.bias"))
    y = ev + img + zf * g("beta")
    ffn = F.conv2d(F.gelu(F.conv2d(ln(y, "norm2"), g("conv4.weight"), g("conv4.bias"))), g("conv5.weight"), g("conv5.bias"))
    return F.conv2d(y, g("conv_y_side.weight"), g("conv_y_side.bias")) + ffn * g("gamma")


_EGACA = {}


def _egaca_engine():
    """The full-width network (built once per session) with released-checkpoint-like weights, and its level-1 EGACA block."""
    if not _EGACA:
        from oracle import refid_oracle as O
        from refid_amd.archs import define_network
        torch.manual_seed(5)
        P = O.make_params(26, mode="init", seed=5)
        for k in P:
            if k.endswith((".beta", ".gamma")):
                P[k] = torch.randn_like(P[k]) * 0.1
        net = define_network(dict(type="FinalBidirectionAttenfusion", img_chn=26, ev_chn=2, num_encoders=3,
                                  base_num_channels=32, num_block=1, num_residual_blocks=2))
        net.load_state_dict(P, strict=True)
        net = net.cuda()
        net.engine.repack()
        _EGACA.update(P=P, net=net)
    return _EGACA["P"], _EGACA["net"].engine


def _egaca_cpu(P, ev, img, gout, dtype):
    """(output, {name: gradient}) of the block in `dtype` on the CPU; names: 'ev', 'img' and the block's parameters."""
    a = EGACA_PREFIX
    Q = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in P.items() if k.startswith(a + ".")}
    e, i = ev.to(dtype).clone().requires_grad_(True), img.to(dtype).clone().requires_grad_(True)
    if dtype == torch.float64:
        from test_hip_egaca import _egaca_ref
        out = _egaca_ref(Q, a, e, i)
        assert torch.equal(out, _egaca_any_dtype(Q, a, e, i))         # the float32 yardstick below is the same formula
    else:
        out = _egaca_any_dtype(Q, a, e, i)
    out.backward(gout.to(dtype))
    grads = {k[len(a) + 1:]: (Q[k].grad if Q[k].grad is not None else torch.zeros_like(Q[k])).double() for k in Q}
    grads.update(ev=e.grad.double(), img=i.grad.double())
    return out.detach().double(), grads


def _egaca_hip(eng, ev, img, gout, fused):
    """The engine's calls of one EGACA step: image path, forward with a stash, backward, image-path backward, weight-gradient
    finish, fold back.  Returns (output, gradients as _egaca_cpu, names of the ops calls of _egaca_fwd)."""
    from refid_amd import engine as E, ops
    A = eng.enc_f[1].att
    a = EGACA_PREFIX
    evd, imgd, gd = nhwc(ev), nhwc(img), nhwc(gout)
    names = ("conv2d", "layernorm2d_fwd", "dwconv3x3_gelu_fwd", "se_fwd", "scale_cat", "add", "gelu_fwd")
    saved = {k: getattr(ops, k) for k in names}
    old, E.EGACA_FUSED = E.EGACA_FUSED, fused
    calls = []
    for o in eng.all_ops:
        o.w_calls, o.w_last, o.w_pend = 0, None, []
    eng.fold_scratch.zero_()
    eng.zero_grad()
    eng._set_wgrad_groups(1)
    try:
        ip = eng._egaca_img_path(A, imgd)
        for k in names:
            setattr(ops, k, (lambda f, k: (lambda *aa, **kw: (calls.append(k), f(*aa, **kw))[1]))(saved[k], k))
        st = {}
        out = eng._egaca_fwd(A, evd, imgd, ip, st)
        for k in names:
            setattr(ops, k, saved[k])
        img_grad = torch.zeros_like(imgd)
        g_ev = eng._egaca_bwd(A, gd, img_grad, ip, st)
        eng._egaca_img_bwd(A, imgd, img_grad, ip)
        E.finish_wgrads(A.ops())
        eng._egaca_fold_back(A)
        torch.cuda.synchronize()
    finally:
        for k in names:
            setattr(ops, k, saved[k])
        E.EGACA_FUSED = old
    grads = {k[len(a) + 1:]: eng.arena.g(k).double().cpu() for k in eng.arena.shapes if k.startswith(a + ".")}
    grads.update(ev=nchw(g_ev), img=nchw(img_grad))
    return nchw(out), grads, calls


_EGACA_REF = {}


def _egaca_reference(shape):
    """Inputs and the two CPU runs (float64, float32) of a leg, computed once and shared by its fused / unfused tests."""
    if shape not in _EGACA_REF:
        n, h, w = shape
        P, _ = _egaca_engine()
        ev, img = (_fp32(_uni(121 + i, n, 64, h, w)) for i in range(2))
        gout = _fp32(_uni(123, n, P[EGACA_PREFIX + ".conv5.weight"].shape[0], h, w))
        r64 = _egaca_cpu(P, ev, img, gout, torch.float64)
        r32 = _egaca_cpu(P, ev, img, gout, torch.float32)
        _EGACA_REF[shape] = (ev, img, gout, r64, r32)
    return _EGACA_REF[shape]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,fused", [((3, 8, 16), True), ((3, 8, 16), False), ((2, 64, 64), True), ((2, 64, 64), False),
                                         ((1, 24, 20), True)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("fused" if v else "unfused"))
def test_egaca_block_forward_and_backward_against_float64_autograd(shape, fused):
    """Output, input gradients and every parameter gradient of the c = 64 EGACA block through the engine's own calls.  Per
    tensor, max-normalised: at most E2E_MARGIN times the error of torch float32 on the CPU, plus 2^-22.  (1, 24, 20): h w is no
    multiple of 128, so the forward must take the one-kernel-per-op route with the switch on."""
    P, eng = _egaca_engine()
    A = eng.enc_f[1].att
    ev, img, gout, (o64, g64), (o32, g32) = _egaca_reference(shape)
    out, grads, calls = _egaca_hip(eng, ev, img, gout, fused)
    takes_fused = fused and (shape[1] * shape[2]) % 128 == 0
    assert len(calls) == ((5 if A.wp_cat is not None else 6) if takes_fused else 12), calls
    assert set(grads) == set(g64), sorted(set(grads) ^ set(g64))
    rows, bad = [], []
    for name in ["out", "ev", "img"] + sorted(k for k in g64 if k not in ("ev", "img")):
        got, r64, r32 = (out, o64, o32) if name == "out" else (grads[name], g64[name], g32[name])
        got = got.reshape(r64.shape)
        assert bool(torch.isfinite(got).all()), name
        scale = float(r64.abs().max())
        if name.startswith("se_2."):
            assert scale == 0.0 and float(got.abs().max()) == 0.0, f"{name}: unused parameters must receive exactly zero"
            continue
        assert scale > 0.0, name
        e_hip, e_f32 = float((got - r64).abs().max()) / scale, float((r32 - r64).abs().max()) / scale
        rows.append(f"{name:24s} hip {e_hip:.3e}   torch float32 {e_f32:.3e}")
        if not e_hip <= E2E_MARGIN * e_f32 + E2E_ABS:
            bad.append(rows[-1])
    print("\n".join(rows))
    assert not bad, f"EGACA block {shape}, fused {fused}: max-normalised error against float64 above {E2E_MARGIN} x torch float32 + " \
                    f"2^-22:\n" + "\n".join(bad) + "\nall tensors:\n" + "\n".join(rows)
