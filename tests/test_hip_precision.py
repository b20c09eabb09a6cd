"""Element-wise precision contract of the fp32-class conv forms against float64.

For every output element o the gate is

    |got_o - ref_o| <= c * 2^-24 * S_o

with ref the float64 torch convolution on the CPU (forward or input gradient, no epilogue) and S_o the error scale of o:

  * direct forms (conv_down 4x4 / stride 2 forward and its input gradient): S_o = sum of |x| |w| over o's own window,
    the float64 convolution of |x| with |w|;
  * Winograd F(2x2,3x3) forms: the fp32 tile's error already depends on the whole 4x4 input patch of o's 2x2 output tile
    (its transforms add patch elements before any product), so S_o = sum over ci of max_patch |x_ci| * sum_taps |w_co,ci|.

One constant c per role (C_DOWN_FWD ...).  The strict fp32 forms are the calibration and meet the same bound with the same c on
the same data in the same test: the fp32 MFMA tiles (conv_down: algo 0, what REFID_DOWN_SPLIT=0 selects; 3x3: Winograd algo 1) and
the exact three-plane bf16 forms (six products: algo 4 terms 6, algo 5 terms 0).  So the bound describes fp32 arithmetic, and a
form that meets it is per element as good as fp32.

Data families, each checked per element:
  (a) O(1) uniform data;
  (b) hot pixels: one per 16 x 64 input block (inside one conv_down workgroup of either tile height, inside one Winograd patch),
      on bands of 8 columns whose magnitudes are 2^-12, 2^-20 and 2^-30 of it -- so most windows miss the hot pixel entirely;
  (c) log-uniform per-pixel magnitudes over 2^-20 .. 2^20;
  (d) sparse: 95 % exact zeros, isolated values over 2^-10 .. 2^10 (a masked LeakyReLU input gradient);
  (e) channel-compensated scales x_c 2^s_c with w_c 2^-s_c, s_c rising from -s to s along K (every K step also grows the data,
      so the online rescale of the fp16 forms runs).

The three-fp16-product forms (conv_down mfma_terms 19, Winograd mfma_terms 3) bridge fp16's range with power-of-two scales: the
weights per tensor; the activations per Winograd tile (= the bound's patch) or per conv_down WORKGROUP (8 or 4 x 32 output
pixels x all of K), both online along K.  A value far below its scale block's largest has a subnormal low plane: its error is
then ~2^-33 of the block's largest instead of 2^-24 of itself.  Hence:
  * the Winograd fp16 form meets the bound on (a)-(d) (its block is the patch);
  * the conv_down fp16 form meets it on (a) only; on (b)-(d) it is held to the design's absolute bound
    c * 2^-24 * S_o + C_ABS * 2^-33 * (max|x| sum_window |w_o| + max|w| sum_window |x|);
  * on (e) both fp16 forms meet the bound up to |s| = S_ENV_DOWN / S_ENV_WINO (the envelope: beyond it the weight plane of the
    channels at one end and the activation plane of the other end go subnormal), and the absolute bound at |s| = 20;
  * the conv_down form the engine uses by default (engine.DOWN_SPLIT) meets the bound on every family.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
# c per role, set by the strict fp32 forms: their largest err / (2^-24 S) over these cases is 18.8 (conv_down forward: fp32 tile,
# family c), 14.3 (its input gradient: six bf16 products, family d) and 2.3 (Winograd forward / input gradient, family d) -- the
# Winograd scale is a patch maximum, hence the smaller constant
C_DOWN_FWD = 32.0
C_DOWN_DGRAD = 24.0
C_WINO_FWD = 4.0
C_WINO_DGRAD = 4.0
C_ABS = 64.0               # the fp16 forms' absolute term, in units of 2^-33 of the tensors' largest entries
# family (e) envelope: the largest |s| at which the fp16 forms still meet c.  Measured worst err / (2^-24 S):
# conv_down 3.3 (|s| <= 9), 7.7 (|s| = 10), 52-120 (|s| = 12); Winograd 0.8 (|s| <= 8), 1.9 (|s| = 9), 2.6-7.1 (|s| = 10)
S_ENV_DOWN = 10
S_ENV_WINO = 9
FAMILIES = ["a", "b", "c", "d", "e_env", "e20"]


def _ops():
    from refid_amd import ops
    return ops


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().cuda()


def nchw(t):
    return t.permute(0, 3, 1, 2).double().cpu()


def _gen(seed, *shape):
    return torch.Generator().manual_seed(seed * 1000003 + sum(shape) * 7919 + len(shape))


def _uni(seed, *shape):
    return torch.rand(*shape, generator=_gen(seed, *shape), dtype=torch.float64) * 2 - 1


def _fp32(t):
    return t.float().double()                      # what the kernels are given: fp32 numbers, exactly


# ---- data families ---------------------------------------------------------------------------------------------------------
def _ramp(C, s):
    """s_c rising from -s to s over C channels (integers)."""
    return torch.tensor([round(s * (2.0 * c / (C - 1) - 1.0)) if C > 1 else 0 for c in range(C)], dtype=torch.float64)


def make_data(family, xshape, wshape, kaxis, seed=0, hot=(16, 64, 7, 33)):
    """(x, w) as float64 tensors holding fp32 numbers.  x: the conv's operand (input, or output gradient for an input gradient);
    kaxis: the weight axis that runs along x's channels (1 for a forward conv, 0 for an input gradient); hot = (py, px, ry, rx):
    hot pixels of family (b) at rows ry mod py, columns rx mod px."""
    N, C, H, W = xshape
    x = _uni(seed + 1, *xshape)
    w = _uni(seed + 2, *wshape) / math.sqrt(C * wshape[2] * wshape[3])
    if family == "b":
        py, px, ry, rx = hot
        cls = (torch.arange(W) // 8) % 3
        mag = torch.tensor([2.0 ** -12, 2.0 ** -20, 2.0 ** -30], dtype=torch.float64)[cls].view(1, 1, 1, W).expand(N, 1, H, W).clone()
        mag[:, :, ry::py, rx::px] = 1.0
        x = x * mag
    elif family == "c":
        r = torch.rand(N, 1, H, W, generator=_gen(seed + 3, N, H, W), dtype=torch.float64) * 40 - 20
        x = x * torch.exp2(r)
    elif family == "d":
        keep = torch.rand(*xshape, generator=_gen(seed + 4, *xshape), dtype=torch.float64) < 0.05
        r = torch.rand(*xshape, generator=_gen(seed + 5, *xshape), dtype=torch.float64) * 20 - 10
        x = torch.where(keep, x * torch.exp2(r), torch.zeros_like(x))
    elif family.startswith("e"):
        s = _ramp(C, int(family[1:]))
        x = x * torch.exp2(s).view(1, C, 1, 1)
        shp = [1, 1, 1, 1]
        shp[kaxis] = C
        w = w * torch.exp2(-s).view(shp)
    else:
        assert family == "a", family
    return _fp32(x), _fp32(w)


def _family(fam, s_env):
    return {"e_env": "e%d" % s_env, "e20": "e20"}.get(fam, fam)


# ---- float64 references and error scales -----------------------------------------------------------------------------------
def ref_down_fwd(x, w):
    ax, aw = x.abs(), w.abs()
    ones = torch.ones(1, *w.shape[1:], dtype=torch.float64)
    ref = F.conv2d(x, w, None, 2, 1)
    S = F.conv2d(ax, aw, None, 2, 1)
    absb = float(ax.max()) * aw.sum((1, 2, 3)).view(1, -1, 1, 1) + float(aw.max()) * F.conv2d(ax, ones, None, 2, 1)
    return ref, S, absb


def ref_down_dgrad(g, w):
    ag, aw = g.abs(), w.abs()
    ones = torch.ones(w.shape[0], 1, *w.shape[2:], dtype=torch.float64)
    ref = F.conv_transpose2d(g, w, None, 2, 1)
    S = F.conv_transpose2d(ag, aw, None, 2, 1)
    absb = float(ag.max()) * aw.sum((0, 2, 3)).view(1, -1, 1, 1) + float(aw.max()) * F.conv_transpose2d(ag, ones, None, 2, 1)
    return ref, S, absb


def _patch_max(a):
    """max |x| over the 4x4 input patch of every 2x2 output tile of a 3x3 / pad 1 conv: (N, C, ceil(H/2), ceil(W/2))."""
    return F.max_pool2d(F.pad(a, (1, 2, 1, 2)), 4, 2)


def _per_tile(t, H, W):
    return t.repeat_interleave(2, 2).repeat_interleave(2, 3)[:, :, :H, :W]


def ref_wino(x, w, dgrad):
    """forward: x (N, Ci, H, W), w (Co, Ci, 3, 3); input gradient: x = the output gradient (N, Co, H, W), same w."""
    H, W = x.shape[2:]
    if dgrad:
        ref = F.conv_transpose2d(x, w, None, 1, 1)
        wk = w.abs().sum((2, 3)).t()                          # (Ci, Co): [out channel of this conv, x channel]
    else:
        ref = F.conv2d(x, w, None, 1, 1)
        wk = w.abs().sum((2, 3))
    pm = _patch_max(x.abs())
    S = _per_tile(F.conv2d(pm, wk[:, :, None, None]), H, W)
    X1 = _per_tile(16.0 * pm.sum(1, keepdim=True), H, W)
    absb = 2.25 * float(x.abs().max()) * wk.sum(1).view(1, -1, 1, 1) + 2.25 * float(w.abs().max()) * 9 * X1
    return ref, S, absb


def check(got, ref, S, c, what, absb=None):
    """Every element within c 2^-24 S (+ C_ABS 2^-33 absb when given); NaN / inf fail.  Returns the worst err / (2^-24 S)."""
    err = (got - ref).abs()
    bound = c * EPS * S
    if absb is not None:
        bound = bound + C_ABS * 2.0 ** -33 * absb
    ok = err <= bound
    ratio = torch.where(S > 0, err / (EPS * S), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), ratio)
    worst = float(ratio.max())
    if not bool(ok.all()):
        bad = (~ok).reshape(-1).nonzero()[:, 0]
        i = int(bad[0])
        idx = np.unravel_index(i, tuple(err.shape))
        raise AssertionError(
            f"{what}: {bad.numel()} of {err.numel()} elements outside {'c 2^-24 S + C_ABS 2^-33 M' if absb is not None else 'c 2^-24 S'} "
            f"(c = {c}); first at {tuple(int(v) for v in idx)}: got {float(got.reshape(-1)[i]):.9e}, float64 {float(ref.reshape(-1)[i]):.9e}, "
            f"error {float(err.reshape(-1)[i]):.3e}, bound {float(bound.reshape(-1)[i]):.3e}, S {float(S.reshape(-1)[i]):.3e}; "
            f"worst error / (2^-24 S) = {worst:.3g}")
    return worst


# ---- the kernels -----------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def run_down_fwd(x, w, form):
    """conv_down forward.  form 0: fp32 MFMA tile (algo 0); 6 / 19: split tile (algo 4) with that many mfma_terms."""
    ops = _ops()
    N, Ci, H, W = x.shape
    Co = w.shape[0]
    wc = w.float().cuda().contiguous()
    out = torch.full((N, H // 2, W // 2, Co), float("nan"), device="cuda")
    if form == 0:
        kc, bn = ops.conv_kc(4, 4, 2), ops.conv_bn(4, 4, 2, 0, Co)
        wp = ops.pack_conv_weights(wc, ops.ROLE_FWD, bn, kc, 4, 4, Co, Ci)
        ops.conv2d(nhwc(x), wp, out, kh=4, kw=4, stride=2, pad=1, cout=Co, cout_pad=_cdiv(Co, bn) * bn)
    else:
        bn = ops.conv_bn(4, 4, 2, 0, Co)
        wp = ops.pack_conv_weights_split(wc, ops.ROLE_FWD, bn, 4, 4, Co, Ci, planes=3 if form == 6 else 2, f16=form == 19)
        ops.conv2d(nhwc(x), wp, out, kh=4, kw=4, stride=2, pad=1, cout=Co, cout_pad=_cdiv(Co, bn) * bn, algo=4, terms=form)
    return nchw(out)


def run_down_dgrad(g, w, form):
    """conv_down input gradient (four parity classes, refid_conv2d mode 2); forms as run_down_fwd."""
    ops = _ops()
    N, Co, h, wd = g.shape
    Ci = w.shape[1]
    wc = w.float().cuda().contiguous()
    out = torch.full((N, 2 * h, 2 * wd, Ci), float("nan"), device="cuda")
    bn = ops.conv_bn(4, 4, 2, 2, Ci)
    if form == 0:
        wp = ops.pack_conv_weights(wc, ops.ROLE_DOWN_DGRAD, bn, ops.conv_kc(4, 4, 2, 2), 4, 4, Co, Ci)
        ops.conv2d(nhwc(g), wp, out, kh=4, kw=4, stride=2, pad=1, mode=2, cout=Ci, cout_pad=_cdiv(Ci, bn) * bn)
    else:
        wp = ops.pack_conv_weights_split(wc, ops.ROLE_DOWN_DGRAD, bn, 4, 4, Co, Ci, planes=3 if form == 6 else 2, f16=form == 19)
        ops.conv2d(nhwc(g), wp, out, kh=4, kw=4, stride=2, pad=1, mode=2, cout=Ci, cout_pad=_cdiv(Ci, bn) * bn, algo=4,
                   terms=form)
    return nchw(out)


WINO_FORMS = {"fp32": (1, 0), "bf16x6": (5, 0), "f16": (5, 3)}     # name -> (algo, mfma_terms)


def run_wino(x, w, form, dgrad=False, ca=None):
    """3x3 / pad 1 forward (two sources when ca < channels of x: in_a = x[:, :ca], in_b = the rest) or input gradient."""
    ops = _ops()
    algo, terms = WINO_FORMS[form]
    Co, Ci = w.shape[:2]
    rows, kdim = (Ci, Co) if dgrad else (Co, Ci)
    role = ops.ROLE_WINO_DGRAD if dgrad else ops.ROLE_WINO_FWD
    wc = w.float().cuda().contiguous()
    if algo == 5:
        wp = ops.pack_conv_weights_wino6(wc, role, Co, Ci, f16=terms == 3)
    else:
        wp = ops.pack_conv_weights(wc, role, 64, 8, 3, 3, Co, Ci)
    N, C, H, W = x.shape
    out = torch.full((N, H, W, rows), float("nan"), device="cuda")
    ca = ca or C
    ops.conv2d(nhwc(x[:, :ca]), wp, out, kh=3, kw=3, stride=1, pad=1, cout=rows, cout_pad=_cdiv(rows, 64) * 64, algo=algo,
               terms=terms, in_b=nhwc(x[:, ca:]) if ca < C else None)
    return nchw(out)


def _default_down_form():
    from refid_amd import engine
    return engine.DOWN_SPLIT


# ---- (1) conv_down forward / input gradient --------------------------------------------------------------------------------
DOWN_CASES = [
    # (role, N, Ci, Co, H, W): H, W of the conv's INPUT (forward) / of the input gradient
    ("fwd", 2, 32, 64, 256, 256),       # configs[1] level 0 -> 1
    ("fwd", 4, 64, 128, 128, 128),      # level 1 -> 2
    ("fwd", 3, 32, 64, 72, 100),        # partial tiles in both directions
    ("dgrad", 2, 32, 64, 256, 256),
    ("dgrad", 4, 64, 128, 128, 128),
]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", DOWN_CASES, ids=lambda c: "%s-%dx%d-%dto%d-%dx%d" % (c[0], c[1], 1, c[2], c[3], c[4], c[5]))
def test_conv_down_elementwise_against_float64(monkeypatch, case, family):
    role, N, Ci, Co, H, W = case
    fam = _family(family, S_ENV_DOWN)
    if role == "fwd":
        x, w = make_data(fam, (N, Ci, H, W), (Co, Ci, 4, 4), 1, seed=11, hot=(16, 64, 7, 33))
        ref, S, absb = ref_down_fwd(x, w)
        run, c = run_down_fwd, C_DOWN_FWD
    else:
        x, w = make_data(fam, (N, Co, H // 2, W // 2), (Co, Ci, 4, 4), 0, seed=12, hot=(8, 32, 3, 16))
        ref, S, absb = ref_down_dgrad(x, w)
        run, c = run_down_dgrad, C_DOWN_DGRAD
    ops = _ops()
    worst = {}
    for split in (0, 2):
        monkeypatch.setattr(ops, "WINO_SPLIT", split)
        for form in (0, 6):                                                 # the calibration: strict fp32-class forms
            worst[(form, split)] = check(run(x, w, form), ref, S, c, f"conv_down {role} form {form} split {split} family {fam}")
        f16 = run(x, w, 19)
        if fam in ("a", "e%d" % S_ENV_DOWN):
            worst[(19, split)] = check(f16, ref, S, c, f"conv_down {role} fp16 form split {split} family {fam}")
        else:                                                              # the block-scale design bound
            worst[(19, split)] = check(f16, ref, S, c, f"conv_down {role} fp16 form split {split} family {fam} (absolute bound)", absb)
        d = _default_down_form()
        if d not in (0, 6):                                                 # the engine's default form meets the bound everywhere
            check(f16 if d == 19 else run(x, w, d), ref, S, c, f"conv_down {role} DEFAULT form (DOWN_SPLIT={d}) split {split} family {fam}")


# ---- (1) Winograd forward / input gradient ---------------------------------------------------------------------------------
WINO_CASES = [
    # (role, N, Ca, Cb, Co, H, W)
    ("fwd", 2, 64, 0, 64, 128, 128),    # trunk 64 -> 64
    ("fwd", 2, 128, 0, 128, 64, 64),    # trunk 128 -> 128
    ("fwd", 1, 64, 64, 64, 61, 93),     # two sources (trunk main.0), ragged
    ("fwd", 1, 128, 0, 128, 16, 24),    # small grid: split-K under WINO_SPLIT 2
    ("dgrad", 2, 64, 0, 64, 128, 128),
    ("dgrad", 1, 128, 0, 128, 20, 36),  # small grid, ragged tiles
]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", WINO_CASES, ids=lambda c: "%s-%d-%d+%dto%d-%dx%d" % c)
def test_winograd_elementwise_against_float64(monkeypatch, case, family):
    role, N, Ca, Cb, Co, H, W = case
    Ci = Ca + Cb
    fam = _family(family, S_ENV_WINO)
    dgrad = role == "dgrad"
    if dgrad:
        x, w = make_data(fam, (N, Co, H, W), (Co, Ci, 3, 3), 0, seed=21, hot=(8, 32, 5, 13))
        c = C_WINO_DGRAD
    else:
        x, w = make_data(fam, (N, Ci, H, W), (Co, Ci, 3, 3), 1, seed=22, hot=(8, 32, 5, 13))
        c = C_WINO_FWD
    ref, S, absb = ref_wino(x, w, dgrad)
    ops = _ops()
    for split in (0, 2):
        monkeypatch.setattr(ops, "WINO_SPLIT", split)
        for form in ("fp32", "bf16x6"):                                     # the calibration
            check(run_wino(x, w, form, dgrad, None if dgrad else Ca), ref, S, c, f"Winograd {role} {form} split {split} family {fam}")
        got = run_wino(x, w, "f16", dgrad, None if dgrad else Ca)
        if fam == "e20":
            check(got, ref, S, c, f"Winograd {role} fp16 form split {split} family {fam} (absolute bound)", absb)
        else:                                                              # per-tile scale = the bound's patch
            check(got, ref, S, c, f"Winograd {role} fp16 form split {split} family {fam}")


# ---- (3) a sample's bits do not depend on the batch it is in ---------------------------------------------------------------
@pytest.mark.parametrize("split", [0, 1, 2])
def test_fp16_forms_give_a_sample_the_same_bits_in_any_batch(monkeypatch, split):
    """Sample 0's result BITS at B = 1, 2 and 8: conv_down forward and input gradient on three fp16 products, Winograd forward
    and input gradient on three fp16 products, under every split policy (ops.WINO_SPLIT).  With the fp16 forms a scale block's
    largest value sets the rounding of the small values in it, so the blocks must not follow the batch: conv_down's data has
    its hot pixels in the upper half of every 8-row workgroup only, so a 4-row and an 8-row tile (the choice the batch used to make,
    conv_split.hip) scale the lower half differently.  Winograd scales per tile (batch independent); under policy 2 ("auto") its
    split-K factor follows the total grid by design -- a different order of additions for every form, fp32 included -- so there
    only the shapes whose grid never splits are compared (128 -> 128 at 64^2 splits K at B = 1, 2 and not at 8)."""
    ops = _ops()
    monkeypatch.setattr(ops, "WINO_SPLIT", split)
    x, wd = make_data("b", (8, 32, 256, 256), (64, 32, 4, 4), 1, seed=31, hot=(16, 64, 1, 33))
    g, _ = make_data("b", (8, 64, 128, 128), (64, 32, 4, 4), 0, seed=32, hot=(8, 32, 1, 16))
    xw, ww = make_data("c", (8, 64, 128, 128), (64, 64, 3, 3), 1, seed=33)
    xw2, ww2 = make_data("c", (8, 128, 64, 64), (128, 128, 3, 3), 1, seed=34)
    jobs = {
        "conv_down fwd": lambda B: run_down_fwd(x[:B], wd, 19),
        "conv_down dgrad": lambda B: run_down_dgrad(g[:B], wd, 19),
        "Winograd fwd 64": lambda B: run_wino(xw[:B], ww, "f16"),
        "Winograd dgrad 64": lambda B: run_wino(xw[:B], ww, "f16", dgrad=True),
    }
    if split != 2:
        jobs["Winograd fwd 128"] = lambda B: run_wino(xw2[:B], ww2, "f16")
        jobs["Winograd dgrad 128"] = lambda B: run_wino(xw2[:B], ww2, "f16", dgrad=True)
    bad = []
    for name, job in jobs.items():
        base = job(1)[:1]
        assert bool(torch.isfinite(base).all()), name
        for B in (2, 8):
            got = job(B)[:1]
            if not torch.equal(got, base):
                bad.append((name, B, int((got != base).sum()), float((got - base).abs().max())))
    assert not bad, f"sample 0 differs from its B=1 bits (name, B, elements, largest difference): {bad}"
