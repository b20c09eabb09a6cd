"""Every element of every weight packing, padding included, against the layout's index formula restated on the host.

Each case is packed twice -- by its one-by-one call and as a record of ONE ops.PackPlan that holds all cases and a mul_vec
record (many kinds in one table: the batched kernel's binary search, the prepass of the fp16 forms) -- and the two must agree
byte for byte.

Non-Winograd forms are checked bit for bit: the value is one fp32 multiply w * oscale[ch] (or w), the planes are round-to-
nearest-even roundings of exact fp32 differences, the fp16 forms' exponent is clamp(12 - floor(log2 max |w s|), +-110) -- all of
it reproducible with numpy float32 and torch's CPU bf16 / fp16 casts.

Winograd forms: U = (G g G^T) s is a 9-term fp32 sum the compiler may contract into FMAs, so the bounds are derived, not
measured.  With A = sum |G_ia G_jb g_ab| |s| the fp32 U lies within 2^-20 A of the float64 U (at most 12 roundings of 2^-24:
8 additions, the multiply by s, and slack).  fp32 layout: that bound on every element.  Three bf16 planes: U32 = h + m + l is an
fp32 number with h = bf16(U32), m = bf16(U32 - h), l = U32 - h - m exactly and |U32 - U64| <= 2^-20 A.  fp16 planes, v = U64 2^eU
(eU exact): |h - v| <= 2^-11 |v| + 2^eU 2^-20 A + 2^-25 and |h + l - v| <= 2^-22 |v| + 2^eU 2^-20 A + 2^-25 (one rounding to 11
/ two to 22 bits, the fp32 U's error scaled, half an fp16 subnormal step)."""
from typing import NamedTuple, Optional

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F, D, CT, CTD, DD, WF, WD, CTP = range(8)       # ops.ROLE_*
HEADER = 64
G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64)


class Case(NamedTuple):
    fn: str                  # public function: pack / bf16 / split / wino6
    role: int
    o: int
    i: int
    k: int
    kc: int = 8
    bn: int = 32
    planes: int = 0
    f16: bool = False
    terms: Optional[int] = None
    scaled: bool = False
    nbytes: int = 0          # pinned size
    peak: bool = False       # the dedicated tensor whose largest value is 2^9

    @property
    def id(self):
        return "-".join(str(x) for x in (self.fn, "role%d" % self.role, "%dx%d" % (self.o, self.i), "k%d" % self.k, "kc%d" % self.kc,
                                         "p%d" % self.planes, "f16" if self.f16 else "", "t%s" % self.terms,
                                         "s" if self.scaled else "", "peak" if self.peak else "") if x != "")


def _cases():
    out = []
    for sc in (False, True):
        for role, nfl in ((F, 4608), (D, 6912)):                                     # 3x3, tile layout and split planes
            out.append(Case("pack", role, 20, 12, 3, scaled=sc, nbytes=4 * nfl))
            out.append(Case("bf16", role, 20, 12, 3, kc=16, scaled=sc, nbytes=2 * (4608 if role == F else 9216)))
            for pl in (1, 2, 3):
                out.append(Case("split", role, 20, 12, 3, planes=pl, scaled=sc, nbytes=pl * (10240 if role == F else 15360)))
                out.append(Case("split", role, 20, 24, 1, planes=pl, scaled=sc, nbytes=pl * 2048))          # 1x1 planes (kind 2)
            out.append(Case("split", role, 20, 12, 3, planes=2, f16=True, scaled=sc, nbytes=20544 if role == F else 30784))
        for pl in (1, 2, 3):                                                           # 4x4 stride 2 forward
            out.append(Case("split", F, 24, 20, 4, planes=pl, scaled=sc, nbytes=pl * 24576))
        out.append(Case("split", F, 24, 20, 4, planes=2, f16=True, scaled=sc, nbytes=49216))
        for role, nfl in ((WF, 24576), (WD, 40960)):                                   # Winograd
            out.append(Case("pack", role, 40, 24, 3, bn=64, scaled=sc, nbytes=4 * nfl))
            for terms, nb in ((0, (196608, 294912)), (3, (131136, 196672)), (1, (65600, 98368))):
                out.append(Case("wino6", role, 40, 24, 3, kc=16, bn=64, terms=terms, scaled=sc, nbytes=nb[role == WD]))
            if not sc:
                out.append(Case("wino6", role, 40, 24, 3, kc=16, bn=64, terms=1, nbytes=(65600, 98368)[role == WD], peak=True))
    for pl in (1, 2, 3):                                                               # conv_down's input gradient
        out.append(Case("split", DD, 24, 20, 4, planes=pl, nbytes=pl * 24576))
    out.append(Case("split", DD, 24, 20, 4, planes=2, f16=True, nbytes=49216))
    out.append(Case("pack", DD, 24, 20, 4, nbytes=4 * 12288))
    out.append(Case("bf16", DD, 24, 20, 4, kc=16, nbytes=2 * 16384))
    for role, nfl in ((CT, 1536), (CTD, 2048), (CTP, 1536)):                           # ConvTranspose2d(2, 2)
        out.append(Case("pack", role, 12, 24, 2, nbytes=4 * nfl))
    return out


CASES = _cases()


def _mixed(shape, seed, lo=-6, hi=6):
    """normal x 2^U(lo, hi): mixed magnitudes, no zeros"""
    g = np.random.default_rng(seed)
    w = g.standard_normal(shape) * np.exp2(g.uniform(lo, hi, shape))
    w[np.abs(w) < 1e-30] = 1.0
    return w.astype(np.float32)


def _weights(c):
    shape = (c.i, c.o, 2, 2) if c.role in (CT, CTD, CTP) else (c.o, c.i, c.k, c.k)
    if c.peak:
        w = _mixed(shape, 11, -24, 0)
        w *= np.float32(256.0) / np.abs(w).max()
        w.flat[5] = 512.0                                     # largest value 2^9: eU = 3, the low values land in fp16's subnormals
        return w
    return _mixed(shape, 7 + c.k)


def _scale(c):
    return _mixed((c.o,), 23, -2, 2) if c.scaled else None


# ---- the layouts, restated ------------------------------------------------------------------------------------------------------
def _logical(c, w, s):
    """(value[cls][tap][row][k], A or None): fp32 values of the non-Winograd roles; float64 U and its bound's A for Winograd."""
    o, i, kk = c.o, c.i, c.k * c.k
    if c.role in (WF, WD):
        g = w.astype(np.float64)
        if c.role == WD:
            g = g[:, :, ::-1, ::-1]                           # flipped taps
        s64 = np.ones(o) if s is None else s.astype(np.float64)
        u = np.einsum("xa,oiab,yb->xyoi", G, g, G).reshape(16, o, i) * s64[None, :, None]
        a = np.einsum("xa,oiab,yb->xyoi", np.abs(G), np.abs(g), np.abs(G)).reshape(16, o, i) * np.abs(s64)[None, :, None]
        if c.role == WD:                                      # rows = i, k = o
            u, a = u.transpose(0, 2, 1), a.transpose(0, 2, 1)
        return u[None], a[None]
    ws = w if s is None else w * s[:, None, None, None]       # ONE fp32 multiply
    if c.role == F:                                           # rows = o, k = i
        v = ws.reshape(o, i, kk).transpose(2, 0, 1)[None]
    elif c.role == D:                                         # rows = i, k = o, flipped taps
        v = ws.reshape(o, i, kk)[:, :, ::-1].transpose(2, 1, 0)[None]
    elif c.role == CT:                                        # W (ci, co, 2, 2): rows = (q, co), k = ci
        v = w.reshape(i, o, 4).transpose(2, 1, 0).reshape(1, 1, 4 * o, i)
    elif c.role == CTD:                                       # rows = ci, k = co, tap = q
        v = w.reshape(i, o, 4).transpose(2, 0, 1)[None]
    elif c.role == CTP:                                       # rows = ci, k = (q, co)
        v = w.reshape(i, o, 4).transpose(0, 2, 1).reshape(1, 1, i, 4 * o)
    else:                                                     # DD: W (o, i, 4, 4): class (py, px), tap (ta, tb); rows = i, k = o
        v = np.zeros((4, 4, i, o), np.float32)
        for cls in range(4):
            for tap in range(4):
                py, px, ta, tb = cls >> 1, cls & 1, tap >> 1, tap & 1
                ky = ((2 if py else 1) if ta == 0 else (0 if py else 3))
                kx = ((2 if px else 1) if tb == 0 else (0 if px else 3))
                v[cls, tap] = w[:, :, ky, kx].T
    return np.ascontiguousarray(v), None


def _tile(v, kc, bn):
    """[cls][tap][row][k] -> [cls][chunk][tap][rows padded to bn][kc], zero padded"""
    ncls, nt, rows, kdim = v.shape
    rp, nch = -(-rows // bn) * bn, -(-kdim // kc)
    p = np.zeros((ncls, nt, rp, nch * kc), v.dtype)
    p[:, :, :rows, :kdim] = v
    return p.reshape(ncls, nt, rp, nch, kc).transpose(0, 3, 1, 2, 4)


def _arrange(c, v):
    """The packing's VALUE array and the axis its planes go to (None: no planes)."""
    if c.fn in ("pack", "bf16"):
        return _tile(v, c.kc, c.bn), None
    if c.fn == "wino6":
        return _tile(v, 16, 64)[0], 2                         # [chunk16][xi][plane][rows][16]
    if c.k == 1:                                              # [chunk16][plane][rows][16], channels in the pointwise tile's slot order
        slot = [4 * (q >> 3) + (q & 7) if (q & 7) < 4 else 8 + 4 * (q >> 3) + ((q & 7) - 4) for q in range(16)]
        return _tile(v, 16, c.bn)[0, :, 0][..., slot], 1
    if c.k == 3:                                              # [chunk8][plane][tap 0..9][rows][8]: the tenth tap is zero
        v10 = np.concatenate([v, np.zeros_like(v[:, :1])], axis=1)
        return _tile(v10, 8, c.bn)[0], 1
    t = _tile(v, 8, c.bn)
    if c.role == DD:                                          # [class][chunk8][plane][tap][rows][8]
        return t, 2
    nch, rp = t.shape[1], t.shape[3]                          # 4x4 forward: [chunk8][sy][sx][plane][(ty, tx)][rows][8], ky = 2 ty + sy
    t = t[0].reshape(nch, 2, 2, 2, 2, rp, 8).transpose(0, 2, 4, 1, 3, 5, 6)
    return t.reshape(nch, 2, 2, 4, rp, 8), 3


def _planes(v, n, dt, axis):
    """h = rne(v), m = rne(v - h), l = rne(v - h - m) in dt, stacked along `axis`"""
    r, out = torch.from_numpy(np.ascontiguousarray(v)), []
    for _ in range(n):
        h = r.to(dt)
        out.append(h)
        r = r - h.float()                                     # exact in fp32
    return torch.stack(out, dim=axis).contiguous()


def _scale_exp(w, s, o_axis):
    ws = w if s is None else w * s.reshape([-1 if d == o_axis else 1 for d in range(4)])
    m = float(np.abs(ws).max())
    if not m > 0:
        return 0
    return int(min(110, max(-110, 12 - (np.frexp(np.float32(m))[1] - 1))))


def _bits(t):
    return t.contiguous().view(torch.uint8).reshape(-1).numpy()


# ---- one pass over the GPU: every case by its own call and inside one plan -------------------------------------------------------
def _call(ops, c, w, s, out=None):
    if c.fn in ("pack", "bf16"):
        fn = ops.pack_conv_weights if c.fn == "pack" else ops.pack_conv_weights_bf16
        return fn(w, c.role, c.bn, c.kc, c.k, c.k, c.o, c.i, out=out, oscale=s)
    if c.fn == "split":
        return ops.pack_conv_weights_split(w, c.role, c.bn, c.k, c.k, c.o, c.i, planes=c.planes, out=out, oscale=s, f16=c.f16)
    return ops.pack_conv_weights_wino6(w, c.role, c.o, c.i, out=out, oscale=s, terms=c.terms)


def _plan(plan, c, w, s, out):
    if c.fn in ("pack", "bf16"):
        plan.add_pack(w, c.role, c.bn, c.kc, c.k, c.k, c.o, c.i, out, oscale=s, bf16=c.fn == "bf16")
    elif c.fn == "split":
        plan.add_split(w, c.role, c.bn, c.k, c.k, c.o, c.i, c.planes, out, oscale=s, f16=c.f16)
    else:
        plan.add_wino6(w, c.role, c.o, c.i, out, oscale=s, terms=c.terms)


@pytest.fixture(scope="module")
def packed():
    from refid_amd import ops
    dev = torch.device("cuda:0")
    plan = ops.PackPlan(dev)
    lone, batched, keep = [], [], []
    va, vb = torch.from_numpy(_mixed((37,), 3)).to(dev), torch.from_numpy(_mixed((37,), 4)).to(dev)
    for n, c in enumerate(CASES):
        w = torch.from_numpy(_weights(c)).to(dev)
        s = None if not c.scaled else torch.from_numpy(_scale(c)).to(dev)
        a = _call(ops, c, w, s)
        lone.append(a)
        b = torch.empty_like(a)
        b.view(torch.uint8).fill_(0x5a)
        _plan(plan, c, w, s, b)
        batched.append(b)
        keep += [w, s]
        if n == len(CASES) // 2:                              # a vector product in the middle of the table
            vout = torch.empty_like(va)
            plan.add_mul_vec(va, vb, vout)
    plan.build().run()
    torch.cuda.synchronize()
    return dict(lone=[t.cpu() for t in lone], batched=[t.cpu() for t in batched], mul=(va.cpu(), vb.cpu(), vout.cpu()))


def test_the_plan_holds_every_kind_and_its_vector_product_is_exact(packed):
    a, b, out = packed["mul"]
    assert np.array_equal(_bits(out), _bits(a * b))
    assert len(packed["lone"]) == len(CASES) > 60


@pytest.mark.parametrize("n", range(len(CASES)), ids=[c.id for c in CASES])
def test_every_element_of_the_packing(packed, n):
    c = CASES[n]
    got, got_b = packed["lone"][n], packed["batched"][n]
    assert got.numel() * got.element_size() == c.nbytes == got_b.numel() * got_b.element_size()
    raw = _bits(got)
    assert np.array_equal(raw, _bits(got_b)), "the batched launch and the one-by-one call differ"
    w, s = _weights(c), _scale(c)
    v, bound = _logical(c, w, s)
    vals, axis = _arrange(c, v)
    header = c.f16 or c.terms in (1, 3)
    e = 0
    if header:
        e = _scale_exp(w, s, 0)
        assert int(raw[:4].view(np.int32)[0]) == e and not raw[4:HEADER].any()
        raw = raw[HEADER:]
    if bound is None:                                         # exact
        if axis is None:
            want = torch.from_numpy(np.ascontiguousarray(vals))
            want = want.to(torch.bfloat16) if c.fn == "bf16" else want
        elif header:
            want = _planes(np.ldexp(vals, e).astype(np.float32), 2, torch.float16, axis)
        else:
            want = _planes(vals, c.planes, torch.bfloat16, axis)
        assert raw.size == want.numel() * want.element_size()
        bad = np.flatnonzero(raw != _bits(want))
        assert bad.size == 0, f"{bad.size} bytes differ, first at byte {bad[0]}"
        return
    # Winograd: derived bounds
    pad = _arrange(c, np.ones_like(v))[0] == 0
    tol = 2.0 ** -20 * _arrange(c, bound)[0]
    assert not tol[pad].any()
    if axis is None:                                          # the fp32 tile layout
        u = raw.view(np.float32).reshape(vals.shape).astype(np.float64)
        assert not raw.view(np.int32).reshape(vals.shape)[pad].any()
        assert (np.abs(u - vals) <= tol).all()
        return
    npl = {0: 3, 3: 2, 1: 1}[c.terms]
    dt = torch.bfloat16 if c.terms == 0 else torch.float16
    shape = vals.shape[:axis] + (npl,) + vals.shape[axis:]
    pl = torch.from_numpy(raw.copy()).view(dt).reshape(shape)
    assert not pl.view(torch.int16).numpy()[np.broadcast_to(np.expand_dims(pad, axis), shape)].any()      # padding is +0
    p64 = [pl.select(axis, q).double().numpy() for q in range(npl)]
    if c.terms == 0:
        h, m, lo = p64
        u32 = h + m + lo
        assert np.array_equal(u32.astype(np.float32).astype(np.float64), u32)
        t32 = torch.from_numpy(u32.astype(np.float32))
        assert np.array_equal(t32.to(dt).double().numpy(), h)
        assert np.array_equal((t32 - torch.from_numpy(h).float()).to(dt).double().numpy(), m)
        assert np.array_equal(u32 - h - m, lo)
        assert (np.abs(u32 - vals) <= tol).all()
        return
    x = np.ldexp(vals, e)
    slack = np.ldexp(tol, e) + 2.0 ** -25
    assert (np.abs(p64[0] - x) <= 2.0 ** -11 * np.abs(x) + slack).all()
    if npl == 2:
        assert (np.abs(p64[0] + p64[1] - x) <= 2.0 ** -22 * np.abs(x) + slack).all()
    if c.peak:
        assert e == 3 and (np.abs(p64[0][~pad]) < 2.0 ** -14).any()       # the subnormal range is reached


def test_refusals_launch_nothing():
    from refid_amd import ops
    from refid_amd._lib import RefidHipError
    dev = torch.device("cuda:0")
    w3, w5, w1 = (torch.ones(20, 12, k, k, device=dev) for k in (3, 5, 1))
    wt = torch.ones(24, 12, 2, 2, device=dev)
    s = torch.ones(20, device=dev)
    with pytest.raises(RefidHipError):
        ops.pack_conv_weights_wino6(w3, F, 20, 12)
    with pytest.raises(RefidHipError):
        ops.pack_conv_weights_wino6(w3, WF, 20, 12, terms=2)
    with pytest.raises(RefidHipError):
        ops.pack_conv_weights_split(w5, F, 32, 5, 5, 20, 12)
    with pytest.raises(RefidHipError):
        ops.pack_conv_weights_split(w1, F, 32, 1, 1, 20, 12, f16=True)
    with pytest.raises(RefidHipError):
        ops.pack_conv_weights(wt, CT, 32, 8, 2, 2, 12, 24, oscale=torch.ones(12, device=dev))
    calls = (lambda out: ops.pack_conv_weights(w3, F, 32, 8, 3, 3, 20, 12, out=out),
             lambda out: ops.pack_conv_weights_bf16(w3, F, 32, 16, 3, 3, 20, 12, out=out),
             lambda out: ops.pack_conv_weights_split(w3, F, 32, 3, 3, 20, 12, planes=2, out=out, oscale=s),
             lambda out: ops.pack_conv_weights_split(w3, F, 32, 3, 3, 20, 12, out=out, f16=True),
             lambda out: ops.pack_conv_weights_wino6(w3, WF, 20, 12, out=out),
             lambda out: ops.pack_conv_weights_wino6(w3, WF, 20, 12, out=out, terms=1))
    for call in calls:
        good = call(None)
        bad = torch.zeros(good.numel() + 8, dtype=good.dtype, device=dev)
        with pytest.raises(RefidHipError, match="wrong size"):
            call(bad)
        torch.cuda.synchronize()
        assert not bad.view(torch.int16).any()                # nothing was written
