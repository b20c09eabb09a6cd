"""Element-wise precision contract of the weight / bias gradients against float64.

Reference: float64 on the CPU, one GEMM per tap over padded NHWC views, dW[o,i,t] = sum_p g[p,o] x[p+t,i], summed over the time
steps a launch (or a pass) holds.  Error scales per element:

  * direct:   S[o,i,t]   = sum_p |g[p,o]| |x[p+t,i]|                          (the same GEMM on |g|, |x|);
  * Winograd: S^W[o,i]   = sum_T (sum_{p in T} |g[p,o]|) max_{q in patch(T)} |x[q,i]|, T = the form's own gradient tiles (2x2 for
              algo 1, 2x4 for algo 5, 2x4 per parity phase of the input for algo 7), patch(T) = the input window the tile reads;
              one value for all taps of (o, i), because the transforms mix them;
  * bias:     db[o] = sum_p g[p,o], scale sum_p |g[p,o]|.

Gate per element: |got - ref| <= c * 2^-24 * S, on (f) c * 2^-24 * sqrt(L) * S with L the form's longest serial run (pixels per
split plus the slab count of the fold, split_plan).  c is set by the direct fp32 tile (algo 0), which runs on the same data in the
same test; the 2x2 Winograd form meets the same c against S^W, the 2x4 forms (algos 5 / 7) their own measured constant against S^W
(the {1,2,4,8} rows of the gradient transform on sparse gradients), and every Winograd form its own constant against S.

Families (a)-(e) are test_hip_precision's (make_data) applied to the activations x and the output gradient g:
  (a) O(1) both; (b) hot pixels in x; (c) log-uniform magnitudes in both; (d) 95 % zeros in g; (e) channel scales 2^s, |s| <= 20,
  on x's AND g's channels, so rows and columns of dW span 2^+-40;
  (f) biased: x > 0 (after LeakyReLU), g of one sign per channel (a smooth loss): the sums grow with the run length;
  (g) exact: integers times 2^s per channel (|s| <= 20; |x| <= 1, g sparse: 1/128), sized so that R * S^W < 2^24 units (R = 160: the largest
      |Z| x |V| factor of the 2x4 transforms; asserted): every partial sum, in every order, is an integer below 2^24 units.  Then
      the dyadic forms (algo 0, 1, 8, the 1x1 streaming tile, the thin tiles, every bias gradient) are BIT-EXACT, and algos 5 / 7
      differ only by the rounding of their final inverse transform (1/6, 1/12, 1/24).  A lost or doubled tile, group, slab or fold
      piece fails this family at any length.

Measured worst err / (2^-24 S) over every case here, short and train-step length (DESIGN.md 3.4 has them per form and family;
on (f) the ratio is err / (2^-24 sqrt(L) S)):
  direct tiles, every form, (a)-(f): 6.5 (family b); bias gradients, every form: 2.3 (d)           -> C_DIRECT = 8
  algo 1 against S^W, (a)-(f): 1.9 (d)                                                             -> the same C_DIRECT
  algos 5 / 7 against S^W, (a)-(f): 12.5 / 2.2 (both family d)                                     -> C_W24_SW = 16
  Winograd against S (their own constant): algo 1 27.5 (b), algo 5 48.6 (b), algo 7 27.8 (c)      -> C_WINO_S = 64
  (g): algos 5 / 7 against S^W: 1.28 / 0.31; every other form and every bias gradient: bit-exact   -> C_EXACT_W24 = 2
"""
import math

import pytest
import torch
import torch.nn.functional as F

from test_hip_precision import _fp32, _gen, _ramp, check, make_data

pytestmark = pytest.mark.gpu

C_DIRECT = 8.0
C_W24_SW = 16.0              # algos 5 / 7 against S^W: sparse gradients (d) meet the 2x4 transform's {1,2,4,8} rows alone
C_WINO_S = 64.0
C_EXACT_W24 = 2.0
R_W24 = 160.0                # |Z| <= 8 sum_T |g| (Gy x Gx entries <= 8), |V| <= 20 max_patch |x| (By, Bx row sums 2 and 10)
FAMILIES = ["a", "b", "c", "d", "e", "f", "g"]
WINO = (1, 5, 7)


def _ops():
    from refid_amd import ops
    return ops


def _cdiv(a, b):
    return -(-a // b)


# ---- data ------------------------------------------------------------------------------------------------------------------
def fam_tensor(fam, role, shape, seed):
    """NHWC float64 tensor of fp32 numbers: role 'x' (activations) or 'g' (output gradient) of family fam."""
    N, H, W, C = shape
    if fam == "f":
        u = torch.rand(N, H, W, C, generator=_gen(seed, N, H, W, C), dtype=torch.float64)
        if role == "x":
            return _fp32(u + 2.0 ** -8)
        sgn = torch.where(torch.rand(C, generator=_gen(seed + 7, C), dtype=torch.float64) < 0.5, -1.0, 1.0)
        return _fp32(u * sgn * 2.0 ** -10)
    if fam == "g":
        gen = _gen(seed, N, H, W, C)
        s = _ramp(C, 20) if role == "x" else -_ramp(C, 20)
        if role == "x":
            v = torch.randint(-1, 2, (N, H, W, C), generator=gen).double()
        else:
            v = torch.randint(1, 3, (N, H, W, C), generator=gen).double() * torch.where(
                torch.rand(N, H, W, C, generator=gen, dtype=torch.float64) < 0.5, -1.0, 1.0)
            v = torch.where(torch.rand(N, H, W, C, generator=gen, dtype=torch.float64) < 1.0 / 128, v, torch.zeros_like(v))
        return v * torch.exp2(s)
    pick = {"a": "a", "b": "b" if role == "x" else "a", "c": "c", "d": "d" if role == "g" else "a", "e": "e20"}[fam]
    t, _ = make_data(pick, (N, C, H, W), (1, C, 1, 1), 1, seed=seed)
    return t.permute(0, 2, 3, 1).contiguous()


def unit(role, C):
    """Family (g): the per-channel power of two every value of channel c is an integer multiple of."""
    return torch.exp2(_ramp(C, 20) if role == "x" else -_ramp(C, 20))


def form_units(name):
    """Family (g): units of the rows (output channels) and columns (input channels) of a form's weight gradient."""
    k, s, p, co, ca, cb, algo, oreal = FORMS[name]
    if name == "convT":
        return unit("x", 64), unit("g", 32)
    if name == "iblock":
        return unit("g", 64)[:co], unit("x", 64)[32:64]
    if k == 4:
        return unit("g", 64)[:co], unit("x", 32)[:ca]
    return unit("g", 64)[:oreal or co], unit("x", 64)[:ca + cb]


# ---- float64 references and scales -----------------------------------------------------------------------------------------
def ref_direct(g, x, k, stride, pad):
    """g (N, Ho, Wo, Co), x (N, H, W, Ci) float64 -> dW, S (Co, Ci, k, k); db, Sb (Co)."""
    N, Ho, Wo, Co = g.shape
    Ci = x.shape[3]
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    G = g.reshape(-1, Co)
    Ga = G.abs()
    dW = torch.empty(Co, Ci, k, k, dtype=torch.float64)
    S = torch.empty_like(dW)
    for ky in range(k):
        for kx in range(k):
            xs = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :].reshape(-1, Ci)
            dW[:, :, ky, kx] = G.t() @ xs
            S[:, :, ky, kx] = Ga.t() @ xs.abs()
    return dW, S, G.sum(0), Ga.sum(0)


def _tile_scale(g, x, th, tw):
    """sum_T (sum_{p in T} |g|) max_{patch(T)} |x| for th x tw gradient tiles of a 3x3 / pad-1 / stride-1 conv: (Co, Ci)."""
    N, Ho, Wo, Co = g.shape
    Ci = x.shape[3]
    ty, tx = _cdiv(Ho, th), _cdiv(Wo, tw)
    ga = F.pad(g.abs().permute(0, 3, 1, 2), (0, tx * tw - Wo, 0, ty * th - Ho))
    gs = ga.reshape(N, Co, ty, th, tx, tw).sum((3, 5)).permute(0, 2, 3, 1).reshape(-1, Co)
    xa = F.pad(x.abs().permute(0, 3, 1, 2), (1, tx * tw + 1 - x.shape[2], 1, ty * th + 1 - x.shape[1]))
    xm = F.max_pool2d(xa, (th + 2, tw + 2), (th, tw)).permute(0, 2, 3, 1).reshape(-1, Ci)
    return gs.t() @ xm


def wino_scale(g, x, algo):
    if algo == 1:
        return _tile_scale(g, x, 2, 2)
    if algo == 5:
        return _tile_scale(g, x, 2, 4)
    return sum(_tile_scale(g, x[:, p::2, q::2, :], 2, 4) for p in (0, 1) for q in (0, 1))      # algo 7: parity phases


# ---- the forms ---------------------------------------------------------------------------------------------------------------
# name: (k, stride, pad, co, ca, cb, algo, o_real); 'convT': algo 8 on (low-res input as "g", high-res gradient as "in_a");
# 'head': thin-input tile (c_a = 4); 'pred': thin-output tile (3 real output channels, gradient padded to 4); 'iblock': one-shot
# column block i_base = 32 of a 96-column gradient
FORMS = {
    "w3_direct": (3, 1, 1, 64, 64, 0, 0, None),
    "w3_narrow": (3, 1, 1, 32, 16, 0, 0, None),
    "w3_2src_direct": (3, 1, 1, 64, 40, 24, 0, None),
    "wino22": (3, 1, 1, 64, 64, 0, 1, None),
    "wino24": (3, 1, 1, 64, 64, 0, 5, None),
    "wino24_2src": (3, 1, 1, 64, 32, 32, 5, None),
    "wino24_co32": (3, 1, 1, 32, 32, 0, 5, None),
    "down_w24": (4, 2, 1, 64, 32, 0, 7, None),
    "down_direct": (4, 2, 1, 64, 32, 0, 0, None),
    "convT": (2, 2, 0, 64, 32, 0, 8, None),
    "pw": (1, 1, 0, 64, 64, 0, 0, None),
    "pw_2src": (1, 1, 0, 64, 32, 32, 0, None),
    "pred": (3, 1, 1, 4, 32, 0, 0, 3),
    "head": (5, 1, 2, 32, 4, 0, 0, None),
    "iblock": (1, 1, 0, 64, 64, 0, 0, None),
}
LONG_E = ["w3_direct", "wino22", "wino24", "wino24_2src", "wino24_co32", "down_w24", "down_direct"]


def split_plan(name, n, ho, wo):
    """(nsplit, slab floats, workspace bytes) of a form's launch -- a mirror of refid_wgrad_split (wgrad_args.h) with each
    family's tile constants (plan_of in conv_wgrad.hip, pws_plan in wgrad_pws.hip), of thin_nsplit and of refid_slab_fold_count,
    for the phased calls (ci = i_total)."""
    k, s, p, co, ca, cb, algo, _ = FORMS[name]
    ci = ca + cb
    ntaps = k * k
    fold = True

    def pws(co, ca, cb, ci, npix):
        ow = 4 if co >= 128 else 2
        wi = 4 if ci >= 128 else (2 if ci >= 64 else 1)
        while cb and wi > 1 and ca % (32 * wi):
            wi //= 2
        if ow == 4 and wi == 1:
            wi = 2
        pb = 32 if ow + wi <= 4 else 16
        ncot, ncit = _cdiv(co, 32 * ow), _cdiv(ci, 32 * wi)
        want = _cdiv(512, ncot * ncit)
        want = want // 8 * 8 if want >= 8 else want
        return max(1, min(want, _cdiv(npix, pb))), ncot * 32 * ow, ncit * 32 * wi

    if name == "head":
        ns = min(_cdiv(wo, 32) * _cdiv(ho, 4) * n, 768)
        return ns, None, ns * 4 * (4 * 1024 + 32) * 4
    if algo == 8:
        ns, cop, cip = pws(co, 2 * ca, 2 * ca, 4 * ca, n * ho * wo)
        ntaps = 1
    elif k == 1:
        ns, cop, cip = pws(co, ca, cb, ci, n * ho * wo)
    elif algo in (5, 7):
        ot = 64 if co > 32 else 32
        ncot, ncit = _cdiv(co, ot), _cdiv(ci, 32)
        want = _cdiv(512 * 3 // 2 if ot == 32 else 512, ncot * ncit * (4 if algo == 7 else 1))
        want = want // 8 * 8 if want >= 8 else want
        # K tiles of 4 x 16 gradient pixels and 24 planes; conv_down (F(2,3) x F(2,4)): 6 x 16 pixels, four phases of 20 planes
        ns = max(1, min(want, _cdiv(wo, 16) * _cdiv(ho, 6 if algo == 7 else 4) * n))
        cop, cip, ntaps = ncot * ot, ncit * 32, (4 * 20 if algo == 7 else 24)
    else:
        if algo == 1:
            cot, cit, th, tw, ntaps, fold = 64, 32, 4, 32, 16, False
        elif k == 3:
            cot = 32 if co <= 32 else 64
            cit = 32 if ci <= 32 else 64
            th, tw = 2, 32
        else:                                               # 4x4 stride 2
            cot, cit, th, tw = 64, 32, 2, 16
        ncot, ncit = _cdiv(co, cot), _cdiv(ci, cit)
        ns = max(1, min(_cdiv(512, ncot * ncit), _cdiv(wo, tw) * _cdiv(ho, th) * n))
        cop, cip = ncot * cot, ncit * cit
    slab = ntaps * cop * cip
    return ns, slab, (ns * slab + ns * cop + (fold_count(slab, ns) if fold else 0) * slab) * 4


def fold_count(slab, ns):
    if ns < 2:
        return 0
    pieces = (slab // 4 + 255) // 256
    S = min(16, _cdiv(2048, pieces))
    if S >= ns:
        S = ns // 2
    return max(S, 1)


def form_dims(D, name):
    """(n, ho, wo) of the gradient a form reduces over (the low-res layer input for the ConvTranspose form)."""
    if name == "convT":
        return tuple(D.xl[0].shape[:3])
    return tuple(D.g[0].shape[:3])


def serial_length(name, n, ho, wo, steps):
    """L: the longest serial run of additions into one accumulator -- pixels per split over all steps, plus the slabs."""
    ns = split_plan(name, n, ho, wo)[0]
    if name == "head":
        ns *= 4                                             # one slab per wave
    return _cdiv(steps * n * ho * wo, ns) + ns


class Data:
    """The float64 operands of one family at one size, and their fp32 GPU copies, per time step."""

    def __init__(self, fam, T, N, H, W, seed):
        self.fam, self.T = fam, T
        # kept as fp32 (every value is an fp32 number): promoted to float64 per step by the reference
        self.x = [fam_tensor(fam, "x", (N, H, W, 64), seed + 10 * t).float() for t in range(T)]
        self.g = [fam_tensor(fam, "g", (N, H, W, 64), seed + 10 * t + 1).float() for t in range(T)]
        # conv_down (4x4 / stride 2): its output gradient is g itself, at (H, W), its input is (2H, 2W)
        self.xd = [fam_tensor(fam, "x", (N, 2 * H, 2 * W, 32), seed + 10 * t + 2).float() for t in range(T)]
        # ConvTranspose2d(64 -> 32, 2, 2): low-res input (the weight gradient's "g"), high-res output gradient ("in_a"); its
        # width a multiple of 32 pixels (the patch form's ring buffers)
        hl, wl = H, _cdiv(W, 32) * 32
        self.xl = [fam_tensor(fam, "x", (N, hl, wl, 64), seed + 10 * t + 3).float() for t in range(T)]
        self.gh = [fam_tensor(fam, "g", (N, 2 * hl, 2 * wl, 32), seed + 10 * t + 4).float() for t in range(T)]
        self._gpu = {}
        self.refs = {}

    def gpu(self, key, t):
        if (key, t) not in self._gpu:
            self._gpu[(key, t)] = getattr(self, key)[t].cuda()
        return self._gpu[(key, t)]

    def operands(self, name, t):
        """(g, x) float64 as the form's weight gradient sees them: x holds all of the form's input channels."""
        k, s, p, co, ca, cb, algo, oreal = FORMS[name]
        if name == "convT":
            return self.xl[t].double(), self.gh[t].double()
        if k == 4:
            return self.g[t][..., :co].double(), self.xd[t][..., :ca].double()
        g = self.g[t][..., :co].double()
        if oreal is not None:
            g[..., oreal:] = 0
        return g, self.x[t][..., :ca + cb].double()


def reference(D, name, steps, no_b=()):
    """Sum over `steps` of the float64 gradient, scales and Winograd scale; `no_b`: steps whose second source is missing."""
    k, s, p, co, ca, cb, algo, oreal = FORMS[name]
    key = (k, s, p, co, ca, cb, oreal, name == "convT", tuple(steps), tuple(no_b), algo if algo in WINO else 0)
    if key not in D.refs:                                   # forms on the same operands share the float64 work
        dkey = key[:-1]
        acc, accw = D.refs.get(dkey), None
        for t in steps:
            g, x = D.operands(name, t)
            if t in no_b:
                x[..., ca:] = 0
            if dkey not in D.refs:
                parts = list(ref_direct(g, x, k, s, p))
                if name == "convT":                         # the bias is the layer's: colsum of the high-res output gradient
                    parts[2], parts[3] = x.reshape(-1, x.shape[3]).sum(0), x.reshape(-1, x.shape[3]).abs().sum(0)
                acc = parts if t == steps[0] else [a + b for a, b in zip(acc, parts)]
            if algo in WINO:
                sw = wino_scale(g, x, algo)
                accw = sw if accw is None else accw + sw
        D.refs[dkey] = acc
        D.refs[key] = accw
    dW, S, db, Sb = D.refs[key[:-1]]
    SW = D.refs[key]
    o = oreal or co
    if name == "iblock":
        return dW[:o, 32:], S[:o, 32:], None, None, None
    return dW[:o], S[:o], db[:o], Sb[:o], SW[:o] if SW is not None else None


def run_form(D, name, groups, no_b=(), phase4=True):
    """Issue the form's weight gradient over the time steps in `groups` (each group ONE launch, `more=`; phase 1 then 2, the
    reduction as phase 4 + wgrad_finish_flush), or one-shot per step (groups=None).  Returns (dW, db, slab floats)."""
    ops = _ops()
    k, s, p, co, ca, cb, algo, oreal = FORMS[name]
    o = oreal or co

    def args(t):
        if name == "convT":
            return D.gpu("xl", t), D.gpu("gh", t), None
        if k == 4:
            return D.gpu("g", t)[..., :co], D.gpu("xd", t)[..., :ca], None
        g = D.gpu("g", t)[..., :co]
        if oreal is not None:
            g = g.clone()
            g[..., oreal:] = 0
        xa = D.gpu("x", t)
        if name == "iblock":
            return g, xa[..., 32:64], None
        return g, xa[..., :ca], (xa[..., ca:ca + cb] if cb and t not in no_b else None)

    ci = 4 * 8 if name == "convT" else ca + cb
    if name == "convT":
        dw = torch.zeros(64, 32, 2, 2, device="cuda")
        db = torch.zeros(32, device="cuda")
        geo = dict(kh=2, kw=2, stride=2, pad=0, algo=8)
    elif name == "iblock":
        dw = torch.zeros(o, 96, k, k, device="cuda")
        db = None
        geo = dict(kh=k, kw=k, stride=s, pad=p, i_base=32, i_total=96, algo=0)
    else:
        dw = torch.zeros(o, ci, k, k, device="cuda")
        db = torch.zeros(o, device="cuda")
        geo = dict(kh=k, kw=k, stride=s, pad=p, i_total=ci, algo=algo)
    wdb = None if name == "convT" else db
    slabs, nfl = None, 0
    if groups is None or name == "iblock":
        for grp in (groups or [[0]]):
            for t in grp:
                g, a, b = args(t)
                ops.conv2d_wgrad(g, a, dw, in_b=b, db=wdb, **geo)
                if name == "convT":
                    ops.colsum(D.gpu("gh", t), db)
    else:
        first = True
        for grp in groups:
            (g, a, b), more = args(grp[0]), [args(t) for t in grp[1:]]
            slabs = ops.conv2d_wgrad(g, a, dw, in_b=b, db=wdb, phase=1 if first else 2, slabs=slabs, more=more, **geo)
            if first:
                nfl = slabs.numel()
            first = False
            if name == "convT":
                for t in grp:
                    ops.colsum(D.gpu("gh", t), db)
        g, a, b = args(groups[-1][0])
        ops.conv2d_wgrad(g, a, dw, in_b=b, db=wdb, phase=4 if phase4 else 3, slabs=slabs, **geo)
        if phase4:
            ops.wgrad_finish_flush()
    torch.cuda.synchronize()
    dW = dw.double().cpu()
    if name == "iblock":
        dW = dW[:, 32:64]
    return dW, (db.double().cpu() if db is not None else None), nfl


def check_form(D, name, groups, steps, no_b, L, worst, fails):
    """Run one form and hold it to the family's gate; failures are collected (every form is checked)."""
    k, s, p, co, ca, cb, algo, oreal = FORMS[name]
    ref, S, db_ref, Sb, SW = reference(D, name, steps, no_b)
    got, db, _ = run_form(D, name, groups, no_b)
    fam = D.fam
    what = f"{name} (algo {algo}) family {fam} over {len(steps)} steps"
    tol = math.sqrt(L) if fam == "f" else 1.0
    try:
        if fam == "g":
            uo, ui = form_units(name)
            unit_w = uo.view(-1, 1, 1, 1) * ui.view(1, -1, 1, 1)
            bound = ((R_W24 if algo != 1 else 4.0) * SW.view(*SW.shape, 1, 1) if algo in WINO else S) / unit_w
            assert float(bound.max()) < 2.0 ** 24, f"{what}: family (g) data not exact (bound {float(bound.max()):.3g} units)"
            if algo in (5, 7):
                worst[(name, "SW")] = check(got, ref, SW.view(*SW.shape, 1, 1).expand_as(ref), C_EXACT_W24, what + " vs S^W")
            else:
                bad = got != ref
                assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from float64, first at "
                                             f"{tuple(int(v) for v in bad.nonzero()[0])} (got {float(got[bad][0]):.9e}, float64 "
                                             f"{float(ref[bad][0]):.9e})")
            if db is not None:
                assert torch.equal(db, db_ref), f"{what}: bias gradient differs from float64 (max {float((db - db_ref).abs().max()):.3e})"
            return
        if algo in WINO:
            worst[(name, "SW")] = check(got, ref, tol * SW.view(*SW.shape, 1, 1).expand_as(ref), C_DIRECT if algo == 1 else C_W24_SW,
                                        what + " vs S^W")
            worst[(name, "S")] = check(got, ref, tol * S, C_WINO_S, what + " vs S")
        else:
            worst[(name, "S")] = check(got, ref, tol * S, C_DIRECT, what)
        if db is not None:
            worst[(name, "db")] = check(db, db_ref, tol * Sb, C_DIRECT, what + " bias")
    except AssertionError as e:
        fails.append(str(e))


# ---- (1) every form and family at a short length: one step, one launch -------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_wgrad_forms_elementwise_short(family):
    """One time step (N = 2, 37 x 53: odd, so the last 2x2 / 2x4 Winograd tile row and column and the last macro tile of every
    form are partial) through the one-shot call."""
    D = Data(family, 1, 2, 37, 53, seed=101)
    worst, fails = {}, []
    for name in FORMS:
        n, ho, wo = form_dims(D, name)
        check_form(D, name, None, [0], (), serial_length(name, n, ho, wo, 1), worst, fails)
    print(f"\nworst err / (2^-24 S), family {family}, short:", {f"{a}/{b}": round(v, 3) for (a, b), v in worst.items()})
    assert not fails, "\n".join(fails)


# ---- (1) train-step lengths: 26 steps x B = 2 x 145 x 151 gradient pixels (1.14e6 per weight; conv_down's input 290 x 302) -----
# conv_down's direct tile (2 x 16 pixels) holds 24 x 1460 = 35040 > 2^15 tiles per grouped launch
T_LONG, N_LONG, H_LONG, W_LONG = 26, 2, 145, 151


@pytest.fixture(scope="module")
def long_data():
    cache = {}

    def get(fam):
        if fam not in cache:
            cache.clear()
            cache[fam] = Data(fam, T_LONG, N_LONG, H_LONG, W_LONG, seed=202)
        return cache[fam]
    yield get
    cache.clear()


def long_groups(name):
    """The engine's issue path: groups of 24 steps per launch (more=), phase 1 then 2; two-source forms start with a step that has
    no second source (the first recurrent step); the thin-input tile and the column block cannot group (one launch per step)."""
    if name in ("head", "iblock"):
        return [[t] for t in range(T_LONG)], ()
    if FORMS[name][5]:
        return [[0], list(range(1, 25)), [25]], (0,)
    return [list(range(24)), [24, 25]], ()


@pytest.mark.parametrize("family", ["e", "f", "g"])
def test_wgrad_forms_elementwise_train_length(long_data, family):
    D = long_data(family)
    worst, fails = {}, []
    names = LONG_E if family == "e" else list(FORMS)
    assert 24 * _cdiv(W_LONG, 16) * _cdiv(H_LONG, 2) * N_LONG > 2 ** 15     # (the direct conv_down tile's grouped launch)
    for name in names:
        n, ho, wo = form_dims(D, name)
        groups, no_b = long_groups(name)
        check_form(D, name, groups, list(range(T_LONG)), no_b, serial_length(name, n, ho, wo, T_LONG), worst, fails)
    print(f"\nworst err / (2^-24 S), family {family}, {T_LONG} steps:", {f"{a}/{b}": round(v, 3) for (a, b), v in worst.items()})
    assert not fails, "\n".join(fails)


def test_split_plan_mirrors_the_workspace_request():
    """split_plan (the split counts the sqrt(L) gate of family f uses) against the slab buffer ops.conv2d_wgrad requests for a
    phase-1 call, at the short and the train-step sizes; its split counts are not multiples of the fold count everywhere."""
    D = Data("a", 1, N_LONG, H_LONG, W_LONG, seed=303)
    odd = 0
    for name in FORMS:
        if name == "iblock":
            continue
        n, ho, wo = form_dims(D, name)
        ns, slab, nbytes = split_plan(name, n, ho, wo)
        _, _, nfl = run_form(D, name, [[0]])
        assert nfl == (nbytes + 3) // 4, (name, ns, nfl * 4, nbytes)
        if slab and fold_count(slab, ns) and ns % fold_count(slab, ns):
            odd += 1
    assert odd >= 2, "no form at these sizes folds a split count that is not a multiple of the fold count"


# ---- (2) the engine's issue path end to end: ConvOp.wgrad over T = 23 steps, engine.finish_wgrads ---------------------------
# name: (kind, weight shape, has bias, N, H, W of the gradient); "c3" runs two sources, a first step without the second source and a
# mid-pass change of the source split (32 | 32 -> 40 | 24 -> 32 | 32: algo 5 -> 0 -> 5, ConvOp._slab_layout); "pwi" adds the
# time-independent column block (i_base = 64) of a linearity split; "s00".."s41" queue 42 more phase-4 jobs than the rest,
# so the flush needs more than one launch of REFID_FINISH_BATCH = 40
E2E_OPS = {
    "c3": ("conv", (64, 64, 3, 3), True, 2, 37, 45),
    "c3s": ("conv", (64, 64, 3, 3), True, 1, 13, 15),
    "nar": ("conv", (32, 16, 3, 3), True, 1, 20, 36),
    "down": ("down", (64, 32, 4, 4), True, 2, 18, 20),
    "up": ("convT", (64, 32, 2, 2), True, 1, 10, 32),
    "pw": ("conv", (64, 64, 1, 1), True, 2, 9, 13),
    "pwi": ("conv", (64, 96, 1, 1), True, 1, 8, 12),
    "pred": ("conv", (3, 32, 3, 3), True, 1, 17, 40),
    "head": ("conv", (32, 4, 5, 5), True, 1, 20, 33),
}
E2E_OPS.update({"s%02d" % k: ("conv", (64, 32, 1, 1), True, 1, 4, 8) for k in range(42)})
T_E2E = 23


def _e2e_step(name, t, seed):
    """float64 (g, x) of one step of one op, family (g): g the gradient the weight gradient reads (the low-res layer input for
    ConvTranspose2d), x all of its input channels (the high-res output gradient for ConvTranspose2d)."""
    kind, (o, i, k, _), _, N, H, W = E2E_OPS[name]
    sd = seed + 1000 * t
    if kind == "convT":
        return fam_tensor("g", "x", (N, H, W, o), sd), fam_tensor("g", "g", (N, 2 * H, 2 * W, i), sd + 1)
    if kind == "down":
        return fam_tensor("g", "g", (N, H, W, o), sd), fam_tensor("g", "x", (N, 2 * H, 2 * W, i), sd + 1)
    g = fam_tensor("g", "g", (N, H, W, 4 if o == 3 else o), sd)
    if o == 3:
        g[..., 3:] = 0
    return g, fam_tensor("g", "x", (N, H, W, i), sd + 1)


@pytest.mark.parametrize("w_group", ["default", 8])
def test_convop_issue_path_end_to_end(w_group):
    from collections import OrderedDict
    from refid_amd import engine
    from refid_amd.engine import ConvOp, ParamArena
    ops = _ops()
    shapes = OrderedDict()
    for name, (kind, shp, bias, *_r) in E2E_OPS.items():
        shapes[name + ".weight"] = shp
        if bias:
            shapes[name + ".bias"] = (shp[1] if kind == "convT" else shp[0],)
    A = ParamArena(shapes, torch.device("cuda"))
    oplist = {name: ConvOp(A, name, kind=v[0], need_dgrad=False) for name, v in E2E_OPS.items()}
    group = min(engine.WGRAD_GROUP, T_E2E) if w_group == "default" else w_group
    for op in oplist.values():
        op.w_group = group
    refs = {}
    ops.rows_sum_defer()
    try:
        _e2e_pass(oplist, refs, ops)
    except BaseException:
        ops.rows_sum_flush()
        raise
    engine.finish_wgrads(list(oplist.values()))
    torch.cuda.synchronize()
    fails = []
    for name, (kind, shp, _, *_r) in E2E_OPS.items():
        dW, db, sw = refs[name]
        got, gotb = A.g(name + ".weight").double().cpu(), A.g(name + ".bias").double().cpu()
        if kind == "convT":
            dW = dW.reshape(shp)
        what = f"ConvOp {name} ({kind} {tuple(shp)}), w_group {group}, {T_E2E} steps"
        if sw is not None:                                  # algo 5 / 7 (and c3's algo-0 stretch added in fp32)
            try:
                check(got, dW, sw.view(*sw.shape, 1, 1).expand_as(dW), C_EXACT_W24 + 1, what + " vs S^W")
            except AssertionError as e:
                fails.append(str(e))
        elif not torch.equal(got, dW):
            bad = (got != dW).nonzero()[0]
            fails.append(f"{what}: {int((got != dW).sum())} elements differ from float64, first at {tuple(int(v) for v in bad)}: "
                         f"got {float(got[tuple(bad)]):.9e}, float64 {float(dW[tuple(bad)]):.9e}")
        if not torch.equal(gotb, db):
            fails.append(f"{what}: bias gradient differs from float64 (max {float((gotb - db).abs().max()):.3e})")
    assert not fails, "\n".join(fails)


def _e2e_pass(oplist, refs, ops):
    """One backward pass of E2E_OPS: T_E2E steps of every op through ConvOp.wgrad, float64 sums into refs[name]."""
    for t in range(T_E2E):
        for j, (name, op) in enumerate(oplist.items()):
            kind, (o, i, k, _), _, N, H, W = E2E_OPS[name]
            g, x = _e2e_step(name, t, seed=4000 + 97 * j)
            if name == "c3" and t == 0:
                x[..., 32:] = 0                               # the first recurrent step: no second source yet
            if kind == "convT":
                part = ref_direct(g, x, 2, 2, 0)
                bias = (x.reshape(-1, i).sum(0),)
                op.wgrad(x.float().cuda(), g.float().cuda())     # (output gradient, layer input): ConvOp swaps the roles
            else:
                part = ref_direct(g, x, k, 2 if kind == "down" else 1, 1 if kind == "down" else k // 2)
                bias = (part[2][:o],)
                gg, xx = g.float().cuda(), x.float().cuda()
                if name == "c3":
                    ca = 40 if 12 <= t < 18 else 32
                    op.wgrad(gg, xx[..., :ca].contiguous(), None if t == 0 else xx[..., ca:].contiguous())
                elif name == "pw":                            # two sources; the first step has none yet
                    if t == 0:
                        x[..., 32:] = 0
                        part = ref_direct(g, x, 1, 1, 0)
                    op.wgrad(gg, xx[..., :32].contiguous(), None if t == 0 else xx[..., 32:].contiguous())
                elif name == "pwi":
                    part = ref_direct(g, x[..., :64], k, 1, 0)
                    op.wgrad(gg, xx[..., :64].contiguous())
                else:
                    op.wgrad(gg, xx)
            sw = wino_scale(g, x, 5 if name == "c3" else 7) if name in ("c3", "down") else None
            new = [part[0][:o], bias[0], sw]
            refs[name] = new if name not in refs else [a + b if a is not None else None for a, b in zip(refs[name], new)]
    # the time-independent half of the linearity split: once per pass, straight into columns 64..95
    gsum, x32 = _e2e_step("pwi", 99, seed=5000)
    oplist["pwi"].wgrad(gsum.float().cuda(), x32[..., :32].float().cuda().contiguous(), None, bias=False, i_base=64)
    refs["pwi"][0] = torch.cat([refs["pwi"][0], ref_direct(gsum, x32[..., :32], 1, 1, 0)[0]], 1)


# ---- (3) the other parameter-gradient reductions over 2^20 pixels ------------------------------------------------------------
# measured worst err / (2^-24 S) over (a), (e) and (f) (on (f) / sqrt(L)): LayerNorm2d dw 0.009 / db 0.039, depthwise dw 0.033 /
# db 0.026, colsum 0.026
C_ROWS = 4.0


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("family", ["a", "e", "f"])
def test_channel_parameter_gradients_elementwise(family, deferred):
    """LayerNorm2d dw / db (refid_layernorm2d_bwd + its rows-sum), the depthwise 3x3 dw / db (dwconv3x3_bwd) and colsum over
    4 x 512 x 512 = 2^20 pixels of 32 channels, immediate and queued (rows_sum_defer / rows_sum_flush).  LayerNorm2d's scale is
    sum |g| (|x| + |mu|) rstd: the fp32 normalisation x * rstd - mu * rstd carries that error per pixel."""
    from refid_amd import _lib
    ops = _ops()
    N, H, W, C = 4, 512, 512, 32
    x = fam_tensor(family, "x", (N, H, W, C), 501)
    g = fam_tensor(family, "g", (N, H, W, C), 502)
    xg, gg = x.float().cuda(), g.float().cuda()
    npix = N * H * W
    w = torch.ones(C, device="cuda")
    # float64 references
    G, X = g.reshape(-1, C), x.reshape(-1, C)
    mu = X.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt((X - mu).pow(2).mean(1, keepdim=True) + 1e-6)
    ln_dw, ln_S = (G * (X - mu) * rstd).sum(0), (G.abs() * (X.abs() + mu.abs()) * rstd).sum(0)
    db, Sb = G.sum(0), G.abs().sum(0)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    dw_dw = torch.empty(C, 1, 3, 3, dtype=torch.float64)
    dw_S = torch.empty_like(dw_dw)
    for ky in range(3):
        for kx in range(3):
            xs = xp[:, ky:ky + H, kx:kx + W, :]
            dw_dw[:, 0, ky, kx] = (g * xs).sum((0, 1, 2))
            dw_S[:, 0, ky, kx] = (g.abs() * xs.abs()).sum((0, 1, 2))
    lib = _lib.lib()
    L = {"ln": lib.refid_layernorm2d_bwd_parts(npix, C), "dw": N * lib.refid_dwconv3x3_bwd_parts(H, W, C),
         "cs": lib.refid_colsum_parts(npix, C)}
    tol = {k: (math.sqrt(_cdiv(npix, v) + v) if family == "f" else 1.0) for k, v in L.items()}
    if deferred:
        ops.rows_sum_defer()
    dwl, dbl = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    gx = torch.empty_like(xg)
    ops.layernorm2d_bwd(gg, xg, w, gx, dwl, dbl)
    dwd, dbd = torch.zeros(C, 1, 3, 3, device="cuda"), torch.zeros(C, device="cuda")
    ops.dwconv3x3_bwd(gg, xg, torch.ones(C, 1, 3, 3, device="cuda"), dwd, dbd)
    dbc = torch.zeros(C, device="cuda")
    ops.colsum(gg, dbc)
    if deferred:
        ops.rows_sum_flush()
    torch.cuda.synchronize()
    worst = {}
    cpu = lambda t: t.double().cpu()
    worst["ln dw"] = check(cpu(dwl), ln_dw, tol["ln"] * ln_S, C_ROWS, f"LayerNorm2d dw family {family}")
    worst["ln db"] = check(cpu(dbl), db, tol["ln"] * Sb, C_ROWS, f"LayerNorm2d db family {family}")
    worst["dw dw"] = check(cpu(dwd), dw_dw, tol["dw"] * dw_S, C_ROWS, f"depthwise dw family {family}")
    worst["dw db"] = check(cpu(dbd), db, tol["dw"] * Sb, C_ROWS, f"depthwise db family {family}")
    worst["colsum"] = check(cpu(dbc), db, tol["cs"] * Sb, C_ROWS, f"colsum family {family}")
    print(f"\nworst err / (2^-24 S), family {family}, deferred {deferred}:", {k: round(v, 3) for k, v in worst.items()})
