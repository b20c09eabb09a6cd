"""Thin torch-tensor wrappers over the C ABI (include/refid_hip.h).

Tensors are NHWC fp32 on the GPU: shape (N, H, W, C) with stride(-1) == 1; the pixel
pitch may exceed C (channel-slice views of wider buffers).  torch is used here only
for device memory and streams; all arithmetic happens in librefid_hip.so (one stated
exception: ``event_sim`` puts ``torch.cumsum`` and ``torch.sort`` between its launches).
"""
import collections
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import ConvDesc, WgradDesc, check, lib

ROLE_FWD, ROLE_DGRAD, ROLE_CONVT, ROLE_CONVT_DGRAD, ROLE_DOWN_DGRAD, ROLE_WINO_FWD, ROLE_WINO_DGRAD, ROLE_CONVT_DGRAD_PW = range(8)


# split-K policy for small grids (refid_conv_desc.split_k): REFID_SPLITK = auto (default: by total grid size) |
# sample (by per-sample geometry: a sample's bits do not depend on the batch it is in) | 0 (never)
WINO_SPLIT = {"0": 0, "s": 1}.get(os.environ.get("REFID_SPLITK", os.environ.get("REFID_WINO_SPLITK", "auto"))[:1], 2)

# Winograd x six / x three tile selection (refid_conv_desc.wino_tile): 0 = by problem size, 1 = the 64-channel tile wherever
# cout > 32, 4 = the 32-channel tile everywhere, 5 = as 0 with two K ranges on the grid split + finishing pass instead of inside
# one workgroup (A/B switches)
WINO_TILE = int(os.environ.get("REFID_WINO_TILE", "0"))

# bench.py's roofline leg: when PROFILE is a list, conv2d()/conv2d_wgrad() bracket each launch with
# events on the launch stream and append (kernel, algorithmic_flops, start_event, end_event).
PROFILE = None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_REQUIRE_CUDA = True       # (host-logic tests run the wrappers on CPU tensors against a recording library handle)


def _nhwc(t, name):
    """(ptr, ld) of an NHWC view; validates layout."""
    if t is None:
        return None, 0
    if t.dtype != torch.float32 or (_REQUIRE_CUDA and not t.is_cuda):
        raise _lib.RefidHipError(f"{name}: expected a CUDA float32 tensor, got {t.dtype} on {t.device}")
    if t.dim() != 4:
        raise _lib.RefidHipError(f"{name}: expected NHWC 4-D tensor, got shape {tuple(t.shape)}")
    n, h, w, c = t.shape
    ld = t.stride(2)
    ok = t.stride(3) == 1 and ld % 4 == 0 and ld >= c
    ok = ok and (h == 1 or t.stride(1) == w * ld) and (n == 1 or t.stride(0) == h * w * ld)
    if not ok or t.data_ptr() % 16 != 0:
        raise _lib.RefidHipError(f"{name}: not a dense-pixel NHWC view (shape {tuple(t.shape)}, "
                                 f"strides {t.stride()}, ptr%16={t.data_ptr() % 16})")
    return t.data_ptr(), ld


def conv_kc(kh, kw, stride, mode=0):
    return lib().refid_conv_kc(kh, kw, stride, mode)


def conv_bn(kh, kw, stride, mode, cout):
    return lib().refid_conv_bn(kh, kw, stride, mode, cout)


# Every weight packing: the public spelling (pack fp32 / bf16; split with planes or f16; wino6 with terms 0 / 6 / 3 / 1) -> the
# record kind and `planes` of refid_pack_entry_fill (None: the caller's), the element type of the packing's tensor (the one-plane
# Winograd packing is tagged by it: conv2d), the C size function and one-by-one entry point.  The geometry arguments of each C
# symbol, in its order: _lib.PACK_GEO.
_Form = collections.namedtuple("_Form", "kind planes dtype size entry")
_FORMS = {
    "f32": _Form(0, 0, torch.float32, "refid_packed_weight_floats", "refid_pack_conv_weights"),       # (+ "_scaled" with a scale)
    "bf16": _Form(0, 1, torch.bfloat16, "refid_packed_weight_floats", "refid_pack_conv_weights_bf16"),
    "split": _Form(1, None, torch.bfloat16, "refid_packed_weight_split_bytes", "refid_pack_conv_weights_split"),
    "split1x1": _Form(2, None, torch.bfloat16, "refid_packed_weight_split_bytes", "refid_pack_conv_weights_split"),
    "split_f16": _Form(6, 2, torch.bfloat16, "refid_packed_weight_split_f16_bytes", "refid_pack_conv_weights_split_f16"),
    "wino6": _Form(3, 3, torch.bfloat16, "refid_packed_weight_wino6_bytes", "refid_pack_conv_weights_wino6"),
    "wino3h": _Form(5, 2, torch.bfloat16, "refid_packed_weight_wino3h_bytes", "refid_pack_conv_weights_wino3h"),
    "wino1h": _Form(5, 1, torch.float16, "refid_packed_weight_wino1h_bytes", "refid_pack_conv_weights_wino1h"),
}


def pack_geo(role, o, i, kh=3, kw=3, kc=16, bn=64, planes=0):
    """The geometry of a packing (defaults: the Winograd plane forms')."""
    return dict(role=role, o=o, i=i, kh=kh, kw=kw, kc=kc, bn=bn, planes=planes)


def split_form(kh, kw, f16=False):
    return "split_f16" if f16 else ("split1x1" if kh == 1 and kw == 1 else "split")


def wino6_form(f16=False, terms=None):
    """The packing a conv2d(algo=5, terms=...) call reads.  `terms` wins over the older `f16` flag (f16=True = terms 3)."""
    if terms is None:
        terms = 3 if f16 else 0
    if terms not in (0, 6, 3, 1):
        raise _lib.RefidHipError(f"Winograd packing: terms must be 0 / 6 (three bf16 planes), 3 (two fp16 planes) or 1 (one fp16 "
                                 f"plane), got {terms}")
    return {0: "wino6", 6: "wino6", 3: "wino3h", 1: "wino1h"}[terms]


def pack_elems(form, geo):
    """Elements of the packing's tensor (0: bad geometry)."""
    f = _FORMS[form]
    n = getattr(lib(), f.size)(*(geo[k] for k in _lib.PACK_GEO[f.size]))
    return n if f.size.endswith("floats") else n // 2           # (every size in bytes is of two-byte elements)


def pack_bytes(form, geo):
    return pack_elems(form, geo) * _FORMS[form].dtype.itemsize


def pack_alloc(form, geo, device):
    return torch.empty(pack_elems(form, geo), dtype=_FORMS[form].dtype, device=device)


def pack_form(form, w, geo, out=None, oscale=None, what="pack_form"):
    """Pack `w` (contiguous, reference layout) as `form`: size, contiguity, allocate or check `out`, the one-by-one call."""
    f = _FORMS[form]
    n = pack_elems(form, geo)
    if n == 0:
        raise _lib.RefidHipError(f"{what}: bad geometry")
    if not w.is_contiguous():
        raise _lib.RefidHipError(f"{what}: weight must be contiguous")
    if out is None:
        out = torch.empty(n, dtype=f.dtype, device=w.device)
    elif out.numel() * out.element_size() != n * f.dtype.itemsize:
        raise _lib.RefidHipError(f"{what}: out has the wrong size")
    elif not out.is_contiguous():
        raise _lib.RefidHipError(f"{what}: out must be contiguous")
    name, ptrs = f.entry, [w.data_ptr(), None if oscale is None else oscale.data_ptr(), out.data_ptr()]
    if form == "f32":                                   # two C entry points: with a scale and without the argument
        name, ptrs = (name, ptrs[::2]) if oscale is None else (name + "_scaled", ptrs)
    check(getattr(lib(), name)(*ptrs, *(geo[k] for k in _lib.PACK_GEO[name]), _stream()), name)
    return out


def packed_weight_floats(role, bn, kc, kh, kw, o, i):
    return pack_elems("f32", pack_geo(role, o, i, kh, kw, kc, bn))


def pack_conv_weights(w, role, bn, kc, kh, kw, o, i, out=None, oscale=None):
    """Pack a reference-layout weight (OIHW, or IOHW for ConvTranspose2d) for the conv tile.

    oscale: optional per-output-channel factor folded into the packed copy (FWD/DGRAD)."""
    return pack_form("f32", w, pack_geo(role, o, i, kh, kw, kc, bn), out, oscale, "pack_conv_weights")


def pack_conv_weights_bf16(w, role, bn, kc, kh, kw, o, i, out=None, oscale=None):
    """bf16 packed weights for conv2d(algo=2); kc = 2 * conv_kc(...)."""
    return pack_form("bf16", w, pack_geo(role, o, i, kh, kw, kc, bn), out, oscale, "pack_conv_weights_bf16")


TERMS_F16X3 = 19          # refid_conv_desc.mfma_terms of the split tile's three-fp16-product form (16 + 3)


def packed_weight_split_bytes(role, bn, kh, kw, o, i, planes, f16=False):
    """f16: two fp16 planes behind a 64-byte header (conv2d algo 4 with terms = TERMS_F16X3); `planes` is then ignored."""
    return pack_bytes(split_form(kh, kw, f16), pack_geo(role, o, i, kh, kw, 8, bn, planes))


def pack_conv_weights_split(w, role, bn, kh, kw, o, i, planes=3, out=None, oscale=None, f16=False):
    """Split-bf16 packed weights for conv2d(algo=4): `planes` bf16 numbers per weight (3 = exact, 2 = 2^-17); f16: two fp16
    planes of w 2^eW (22 bits), the scale exponent found by a reduction over the tensor and kept in the packing's header."""
    return pack_form(split_form(kh, kw, f16), w, pack_geo(role, o, i, kh, kw, 8, bn, planes), out, oscale, "pack_conv_weights_split")


def packed_weight_wino6_bytes(role, o, i, f16=False, terms=None):
    """Bytes of the Winograd-domain packing for conv2d(algo=5): three bf16 planes (terms 0 / 6), a 64-byte header + two fp16
    planes (terms 3, or f16=True), or the header + one fp16 plane (terms 1)."""
    return pack_bytes(wino6_form(f16, terms), pack_geo(role, o, i))


def pack_conv_weights_wino6(w, role, o, i, out=None, oscale=None, f16=False, terms=None):
    """Winograd-domain weights as three bf16 planes for conv2d(algo=5); role = ROLE_WINO_FWD / ROLE_WINO_DGRAD.
    terms=3 (or f16=True): the two-fp16-plane packing of conv2d(algo=5, terms=3) (scaled by a per-tensor power of two kept in
    its header); terms=1: its high plane alone, for the one-product form conv2d(algo=5, terms=1)."""
    return pack_form(wino6_form(f16, terms), w, pack_geo(role, o, i), out, oscale, "pack_conv_weights_wino6")


def _pw_extras(pw, out):
    """refid_pw_extras from a dict of tensors / scalars (see include/refid_hip.h); returns (struct, keep-alive list)."""
    x = _lib.PwExtras()
    if pw.get("ln_gamma") is not None:
        x.ln_gamma, x.ln_beta, x.ln_eps = _c(pw["ln_gamma"], "ln_gamma"), _c(pw["ln_beta"], "ln_beta"), pw.get("ln_eps", 1e-6)
        if pw.get("ln_out") is not None:
            x.ln_out, x.ld_ln_out = _nhwc(pw["ln_out"], "ln_out")
    if pw.get("pool") is not None:
        pool = pw["pool"]
        x.pool, x.pool_parts, x.se_c = _c(pool, "pool"), pool.shape[1], pool.shape[2]
        x.hw = pw["hw"]
        x.inv_hw = 1.0 / pw["hw"]
        x.se_w1, x.se_b1, x.se_w2, x.se_b2 = (_c(pw[k], k) for k in ("se_w1", "se_b1", "se_w2", "se_b2"))
        if pw.get("se_s") is not None:
            x.se_m, x.se_z1, x.se_s = _c(pw["se_m"], "se_m"), _c(pw["se_z1"], "se_z1"), _c(pw["se_s"], "se_s")
        if pw.get("xs_out") is not None:
            x.xs_out, x.ld_xs_out = _nhwc(pw["xs_out"], "xs_out")
    if pw.get("res2") is not None:
        if pw["res2"].shape != out.shape:
            raise _lib.RefidHipError("conv2d: res2 shape differs from the output's")
        x.res2, x.ld_res2 = _nhwc(pw["res2"], "res2")
    if pw.get("out2") is not None:
        if pw["out2"].shape != out.shape:
            raise _lib.RefidHipError("conv2d: out2 shape differs from the output's")
        x.out2, x.ld_out2 = _nhwc(pw["out2"], "out2")
    return x


def conv2d(in_a, w_packed, out, *, kh, kw, stride=1, pad=0, mode=0, cout, cout_pad, co_base=0,
           in_b=None, bias=None, res=None, mask=None, slope_pre=1.0, slope_post=1.0, slope_mask=1.0, algo=0, pw=None,
           terms=0, add2=None, out2=None, mask_mode=0):
    """out = mask(post(pre(conv([in_a|in_b]) + bias) + res)); see refid_conv_desc.  pw: dict of the pointwise tile's
    EGACA fusions (refid_pw_extras); terms: algo 4's product count (0 / 6, 3 or 1); algo 5: 0 / 6 = six bf16
    products, 3 = three fp16 products, 1 = one fp16 product (w_packed from pack_conv_weights_wino6 with the same terms); algo 3: 0 = fp32 MFMA, 6 = six bf16 products
    (w_packed from pack_conv_weights_split with kh = kw = 1).  add2 / out2: second output out2 = out + add2 (not algo 3)."""
    if DESC_CACHE and pw is None and PROFILE is None:
        return _conv2d_cached(in_a, w_packed, out, kh, kw, stride, pad, mode, cout, cout_pad, co_base, in_b, bias, res, mask,
                              slope_pre, slope_post, slope_mask, algo, terms, add2, out2, mask_mode)
    d = ConvDesc()
    d.mfma_terms = terms
    if pw is not None:
        if algo != 3:
            raise _lib.RefidHipError("conv2d: pw fusions need the pointwise tile (algo 3)")
        pwx = _pw_extras(pw, out)
        d.pw = C.pointer(pwx)
    d.in_a, d.ld_a = _nhwc(in_a, "in_a")
    d.c_a = in_a.shape[3]
    if in_b is not None:
        d.in_b, d.ld_b = _nhwc(in_b, "in_b")
        d.c_b = in_b.shape[3]
        if in_b.shape[:3] != in_a.shape[:3]:
            raise _lib.RefidHipError("conv2d: in_a / in_b pixel grids differ")
    if algo == 5 and terms == 1:
        # the one-plane packing is half the two-plane one: a packing of the other form would be read as the wrong planes.  The
        # one-plane packing is the only one held in a float16 tensor (the others: bfloat16), and it must cover the chunks this
        # call reads (64-byte header + [chunk16][xi][cout_pad][16] fp16; a call may read the first chunks of a longer packing:
        # the first source alone of a two-source conv)
        chunk = 16 * cout_pad * 16 * 2
        have = w_packed.numel() * w_packed.element_size()
        if w_packed.dtype != torch.float16 or have < 64 + -(-(d.c_a + d.c_b) // 16) * chunk or (have - 64) % chunk:
            raise _lib.RefidHipError(f"conv2d: algo 5 with terms=1 reads the one-plane fp16 packing (a float16 tensor from "
                                     f"pack_conv_weights_wino6 with terms=1: 64 + chunks x {chunk} bytes), got {have} bytes of "
                                     f"{w_packed.dtype}")
    d.w_packed = w_packed.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.out, d.ld_out = _nhwc(out, "out")
    d.res, d.ld_res = _nhwc(res, "res")
    d.mask, d.ld_mask = _nhwc(mask, "mask")
    if out2 is not None:
        if add2 is None or add2.shape != out.shape or out2.shape != out.shape:
            raise _lib.RefidHipError("conv2d: out2 needs add2, both of the output's shape")
        d.add2, d.ld_add2 = _nhwc(add2, "add2")
        d.out2, d.ld_out2 = _nhwc(out2, "out2")
    d.n, d.h, d.w = in_a.shape[0], in_a.shape[1], in_a.shape[2]
    if mode == 0:
        d.ho, d.wo = out.shape[1], out.shape[2]
        chan_ok = out.shape[3] == cout
    else:
        d.ho, d.wo = d.h, d.w
        if out.shape[1] != 2 * d.h or out.shape[2] != 2 * d.w:
            raise _lib.RefidHipError("conv2d: mode 1/2 output must be (2h, 2w)")
        chan_ok = out.shape[3] == (cout // 4 if mode == 1 else cout)
    if not chan_ok or out.shape[0] != d.n:
        raise _lib.RefidHipError(f"conv2d: output shape {tuple(out.shape)} inconsistent with cout={cout} mode={mode}")
    for t, nm in ((res, "res"), (mask, "mask")):
        if t is not None and t.shape != out.shape:
            raise _lib.RefidHipError(f"conv2d: {nm} shape {tuple(t.shape)} != out shape {tuple(out.shape)}")
    d.cout, d.cout_pad, d.co_base = cout, cout_pad, co_base
    d.kh, d.kw, d.stride, d.pad, d.mode = kh, kw, stride, pad, mode
    d.slope_pre, d.slope_post, d.slope_mask = slope_pre, slope_post, slope_mask
    d.mask_mode = mask_mode
    d.algo = algo
    d.wino_tile = WINO_TILE
    if WINO_SPLIT and algo in (0, 1, 2, 4, 5):          # (algo 4: no workspace; the policy decides its tile shape)
        d.split_k = WINO_SPLIT
        need = lib().refid_conv_workspace_bytes(C.byref(d))
        if need:
            ws = _workspace(need, in_a.device, "conv")
            d.ws, d.ws_bytes = ws.data_ptr(), ws.numel() * 4
    if PROFILE is None:
        check(lib().refid_conv2d(C.byref(d), _stream()), "refid_conv2d")
        return out
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(lib().refid_conv2d(C.byref(d), _stream()), "refid_conv2d")
    e1.record()
    taps = {0: kh * kw, 1: 1, 2: 16}[mode]
    flops = 2.0 * d.n * d.ho * d.wo * cout * (d.c_a + d.c_b) * taps
    name = "conv_igemm_kernel<" + lib().refid_conv_tile_name(kh, kw, stride, mode, cout).decode() + \
        (", true> [bf16 operands]" if algo == 2 else ">")
    if algo == 1:
        name = "conv_wino_kernel<1, 2>" if cout <= 32 else "conv_wino_kernel<2, 1>"
    if algo == 5:
        name = "conv_wino6_kernel<2>" if cout > 32 else "conv_wino6_kernel<1>"     # 64- / 32-channel workgroup tile
        if terms == 3:
            name = name[:-1] + ", true>"                                           # three fp16 products
        if terms == 1:
            name = name[:-1] + ", true, fp16x1>"                                   # one fp16 product
    if algo == 4:
        name = "conv_split_kernel<%s>" % ("3, fp16" if terms == TERMS_F16X3 else (terms or 6))
    if algo == 3:
        name = "conv_pw_kernel<1, 8>" if cout <= 32 else ("conv_pw_kernel<2, 4, six>" if terms == 6 else "conv_pw_kernel<2, 4>")
    opix = d.n * out.shape[1] * out.shape[2]
    nbytes = 4.0 * (d.n * d.h * d.w * (d.c_a + d.c_b) + opix * out.shape[3] * (1 + (res is not None) + (mask is not None))
                    + cout * (d.c_a + d.c_b) * taps)
    if out2 is not None:                                   # the second output and its addend are algorithmic bytes too
        nbytes += 8.0 * opix * out.shape[3]
    if pw is not None:                                     # the pointwise tile's fused side outputs / second residual (EGACA)
        for k in ("ln_out", "xs_out", "out2", "res2"):
            if pw.get(k) is not None:
                nbytes += 4.0 * pw[k].numel()
    PROFILE.append((name, flops, e0, e1,
                    (d.n, d.h, d.w, d.c_a, d.c_b, cout, int(res is not None), int(mask is not None), int(bias is not None)),
                    nbytes))
    return out


# ---- descriptor cache (REFID_DESC_CACHE=1; off by default until it has been timed on a GPU box) -------------------------------
# At B=1 a train step is ~4800 launches of ~18 us of GPU time each, and the Python side of ONE conv2d call above -- ~35 ctypes
# field stores, five layout checks, the workspace query -- costs ~16 us: the host is part of what the step waits for (the hipGraph
# replay of the same step is 3.5 ms faster).  Everything in a descriptor except the pointers is a function of the call's scalar
# arguments and of the operands' shapes and strides: the first call with a given signature goes through conv2d's full path with a
# recording library handle, later calls copy the recorded descriptor, refresh the pointers (re-checking their alignment) and the
# workspace, and launch.  tests/test_host_logic.py compares the descriptor BYTES of the two paths call by call.
DESC_CACHE = os.environ.get("REFID_DESC_CACHE", "0") == "1"
_DESC_CACHE = {}
_DESC_PTRS = ("in_a", "in_b", "w_packed", "bias", "out", "res", "mask", "add2", "out2")


def _sig(t):
    return None if t is None else (t.shape, t.stride())


def _conv2d_cached(in_a, w_packed, out, kh, kw, stride, pad, mode, cout, cout_pad, co_base, in_b, bias, res, mask,
                   slope_pre, slope_post, slope_mask, algo, terms, add2, out2, mask_mode):
    global lib, DESC_CACHE
    key = (kh, kw, stride, pad, mode, cout, cout_pad, co_base, slope_pre, slope_post, slope_mask, algo, terms, mask_mode,
           WINO_TILE, WINO_SPLIT, _sig(in_a), _sig(in_b), _sig(out), _sig(res), _sig(mask), _sig(add2), _sig(out2),
           bias is not None, in_a.dtype, out.dtype, in_a.device)
    ent = _DESC_CACHE.get(key)
    if ent is None:
        # first call with this signature: the validating path, with the launch intercepted to keep its descriptor
        real, seen = lib(), []

        class _Recorder:
            def __getattr__(self, name):
                if name == "refid_conv2d":
                    def launch(dref, st):
                        seen.append(ConvDesc.from_buffer_copy(C.string_at(C.addressof(dref._obj), C.sizeof(ConvDesc))))
                        return real.refid_conv2d(dref, st)
                    return launch
                return getattr(real, name)

        keep_lib, keep_flag = lib, DESC_CACHE
        rec = _Recorder()
        lib, DESC_CACHE = (lambda: rec), False
        try:
            conv2d(in_a, w_packed, out, kh=kh, kw=kw, stride=stride, pad=pad, mode=mode, cout=cout, cout_pad=cout_pad,
                   co_base=co_base, in_b=in_b, bias=bias, res=res, mask=mask, slope_pre=slope_pre, slope_post=slope_post,
                   slope_mask=slope_mask, algo=algo, terms=terms, add2=add2, out2=out2, mask_mode=mask_mode)
        finally:
            lib, DESC_CACHE = keep_lib, keep_flag
        _DESC_CACHE[key] = (seen[0], int(seen[0].ws_bytes))
        return out
    d, ws_bytes = ConvDesc.from_buffer_copy(ent[0]), ent[1]     # (a private copy: the recorded descriptor is shared by threads)
    if _REQUIRE_CUDA and not (in_a.is_cuda and out.is_cuda):
        raise _lib.RefidHipError("conv2d: expected CUDA tensors")
    ptrs = (in_a.data_ptr(), None if in_b is None else in_b.data_ptr(), w_packed.data_ptr(),
            None if bias is None else bias.data_ptr(), out.data_ptr(), None if res is None else res.data_ptr(),
            None if mask is None else mask.data_ptr(),
            None if (add2 is None or out2 is None) else add2.data_ptr(),      # (as the validating path: add2 only with out2)
            None if out2 is None else out2.data_ptr())
    for nm, p in zip(_DESC_PTRS, ptrs):
        if p is not None and p % 16 != 0 and nm not in ("w_packed", "bias"):
            raise _lib.RefidHipError(f"{nm}: not a dense-pixel NHWC view (ptr%16={p % 16})")
        setattr(d, nm, p)
    if ws_bytes:
        ws = _workspace(ws_bytes, in_a.device, "conv")     # (per launching stream; grow-only)
        d.ws, d.ws_bytes = ws.data_ptr(), ws.numel() * 4
    check(lib().refid_conv2d(C.byref(d), _stream()), "refid_conv2d")
    return out


_ws_cache = {}
# Bumped whenever a scratch buffer a captured hipGraph may have baked in (split-K workspaces, persistent weight-gradient
# slabs) is replaced by a larger one: train.py re-captures its graphs when the epoch moved (the old buffer is freed).
ALLOC_EPOCH = 0


def _workspace(nbytes, device, kind="wgrad"):
    """Grow-only scratch buffer per (device, stream, kind): the C ABI never allocates, the caller lends it
    scratch that is private to the launching stream (stream-ordered re-use)."""
    key = (device.index, torch.cuda.current_stream().cuda_stream, kind)
    global ALLOC_EPOCH
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        if buf is not None:
            ALLOC_EPOCH += 1
        buf = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
        _ws_cache[key] = buf
    return buf


def conv2d_wgrad(g, in_a, dw, *, kh, kw, stride=1, pad=0, in_b=None, db=None, i_base=0, i_total=None, algo=0,
                 phase=0, slabs=None, more=()):
    """phase 0: one-shot.  phase 1/2: partial products into the caller's persistent `slabs`
    (overwrite / add); phase 3: reduce `slabs` into dw/db (see refid_wgrad_desc); phase 4: as 3 with the element-wise
    stage queued until wgrad_finish_flush().  Returns `slabs`."""
    """dw (+)= wgrad, db (+)= sum g; dw in the reference layout (c_o, i_total, kh, kw)."""
    d = WgradDesc()
    d.g, d.ld_g = _nhwc(g, "g")
    d.c_o = g.shape[3]
    d.in_a, d.ld_a = _nhwc(in_a, "in_a")
    d.c_a = in_a.shape[3]
    if in_b is not None:
        d.in_b, d.ld_b = _nhwc(in_b, "in_b")
        d.c_b = in_b.shape[3]
    d.n, d.h, d.w = in_a.shape[0], in_a.shape[1], in_a.shape[2]
    d.ho, d.wo = g.shape[1], g.shape[2]
    d.kh, d.kw, d.stride, d.pad = kh, kw, stride, pad
    d.i_base = i_base
    d.i_total = i_total if i_total is not None else dw.shape[1]
    d.o_real = dw.shape[0]
    d.algo = algo
    d.phase = phase
    # more: up to 23 further (g, in_a, in_b) triples (refid_wgrad_desc.groups <= 24) -- other time steps of the same conv, added
    # in the same launch
    if more:
        d.groups = 1 + len(more)
        for k, (g2, a2, b2) in enumerate(more):
            pg, ldg = _nhwc(g2, "g (group)")
            pa, lda = _nhwc(a2, "in_a (group)")
            pb, ldb = _nhwc(b2, "in_b (group)") if b2 is not None else (None, d.ld_b)
            if g2.shape != g.shape or a2.shape != in_a.shape or (b2 is None) != (in_b is None) or \
                    (ldg, lda, ldb) != (d.ld_g, d.ld_a, d.ld_b):
                raise _lib.RefidHipError("wgrad: grouped time steps must share shapes, pitches and the source split")
            d.g_more[k], d.in_a_more[k], d.in_b_more[k] = pg, pa, pb
    if not dw.is_contiguous() or dw.dim() != 4 or dw.shape[1] != d.i_total or dw.shape[2:] != (kh, kw) \
            or d.o_real > d.c_o:
        raise _lib.RefidHipError(f"wgrad: dw shape {tuple(dw.shape)} does not match g/in channels "
                                 f"({d.c_o},{d.i_total},{kh},{kw})")
    d.dw = dw.data_ptr()
    d.db = db.data_ptr() if db is not None else None
    nbytes = lib().refid_wgrad_workspace_bytes(C.byref(d))
    if nbytes == 0:
        raise _lib.RefidHipError("wgrad: unsupported geometry")
    if phase == 0:
        ws = _workspace(nbytes, g.device)
    else:
        if slabs is None or (phase == 1 and slabs.numel() * 4 < nbytes):
            # phase 1 overwrites: a larger batch / crop than the first step's simply gets a larger buffer
            if slabs is not None:
                global ALLOC_EPOCH
                ALLOC_EPOCH += 1
            slabs = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=g.device)
        elif slabs.numel() * 4 < nbytes:
            raise _lib.RefidHipError("wgrad: persistent slab buffer too small for this geometry (phase 2/3 must "
                                     "see the geometry of the phase-1 call)")
        ws = slabs
    d.slabs = ws.data_ptr()
    if PROFILE is None or phase >= 3:
        check(lib().refid_conv2d_wgrad(C.byref(d), _stream()), "refid_conv2d_wgrad")
        return slabs
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(lib().refid_conv2d_wgrad(C.byref(d), _stream()), "refid_conv2d_wgrad")
    e1.record()
    ngrp = max(1, d.groups)
    flops = 2.0 * ngrp * d.n * d.ho * d.wo * d.o_real * min(d.c_a + d.c_b, d.i_total) * kh * kw
    nbytes = 4.0 * ngrp * (d.n * d.h * d.w * (d.c_a + d.c_b) + d.n * d.ho * d.wo * d.c_o)
    PROFILE.append((("wgrad_wino_kernel" if algo == 1 else "wgrad_wino24_kernel" if algo == 5 else "wgrad_wino24_down_kernel" if algo == 7 else "wgrad_wino4_kernel" if algo == 6 else "wgrad_wino6_kernel" if algo == 3 else "wgrad_wino_dma_kernel" if algo == 4 else ("wgrad_bf16_kernel" if algo == 2 else
                                                           f"wgrad_kernel<{kh}x{kw}s{stride}>")), flops, e0, e1,
                    (d.n, d.h, d.w, d.c_a, d.c_b, d.c_o, 0, 0, int(db is not None)), nbytes))
    return slabs


_ROWS_KEEP = None          # partial-row buffers of the queued per-channel sums (alive until rows_sum_flush)


def rows_sum_defer():
    """From here to rows_sum_flush() the per-channel parameter-gradient sums of layernorm2d_bwd / dwconv3x3_bwd / colsum are
    queued (refid_rows_sum_defer); the caller must not read those gradients in between."""
    global _ROWS_KEEP
    check(lib().refid_rows_sum_defer(1), "refid_rows_sum_defer")
    _ROWS_KEEP = []


def rows_sum_flush():
    """Issue the queued sums (one launch per ~160, grouped by destination, call order within one) and end the deferral."""
    global _ROWS_KEEP
    if _ROWS_KEEP is None:
        return
    try:
        check(lib().refid_rows_sum_flush(_stream()), "refid_rows_sum_flush")
    finally:
        _ROWS_KEEP = None


def _keep_rows(parts):
    if _ROWS_KEEP is not None:
        _ROWS_KEEP.append(parts)


def wgrad_finish_flush():
    """Issue the element-wise slab-reduction stages queued by conv2d_wgrad(..., phase=4) calls: one launch per kernel
    family on the current stream (refid_wgrad_finish_flush)."""
    check(lib().refid_wgrad_finish_flush(_stream()), "refid_wgrad_finish_flush")


def nchw_to_nhwc(src, c_pad=None, out=None):
    """(N,C,H,W) with dense (C,H,W) planes (any batch stride) -> (N,H,W,c_pad), zero channel padding."""
    n, c, h, w = src.shape
    if src.stride(3) != 1 or src.stride(2) != w or src.stride(1) != h * w:
        raise _lib.RefidHipError("nchw_to_nhwc: per-sample (C,H,W) block must be dense")
    c_pad = c_pad or ((c + 3) // 4) * 4
    dst = out if out is not None else torch.empty((n, h, w, c_pad), dtype=torch.float32, device=src.device)
    check(lib().refid_nchw_to_nhwc(src.data_ptr(), src.stride(0) if n > 1 else c * h * w, dst.data_ptr(), n, c, h, w,
                                   c_pad, _stream()), "refid_nchw_to_nhwc")
    return dst


def nchw_to_nhwc_tb(src, c_pad=None):
    """(B,T,C,H,W) stack with dense (C,H,W) blocks -> (T*B,H,W,c_pad), TIME-major (sample t*B + b), one launch."""
    b, t, c, h, w = src.shape
    if src.stride(4) != 1 or src.stride(3) != w or src.stride(2) != h * w:
        raise _lib.RefidHipError("nchw_to_nhwc_tb: per-(sample, step) (C,H,W) block must be dense")
    c_pad = c_pad or ((c + 3) // 4) * 4
    dst = torch.empty((t * b, h, w, c_pad), dtype=torch.float32, device=src.device)
    check(lib().refid_nchw_to_nhwc_tb(src.data_ptr(), src.stride(0), src.stride(1), dst.data_ptr(), b, t, c, h, w, c_pad,
                                      _stream()), "refid_nchw_to_nhwc_tb")
    return dst


def nhwc_to_nchw_tb(src, c, dst):
    """First c channels of the time-major NHWC stack src (T*B,H,W,ld) -> dst (B,T,c,H,W), one launch."""
    ptr, ld = _nhwc(src, "src")
    b, t = dst.shape[0], dst.shape[1]
    n, h, w, _ = src.shape
    if n != b * t or dst.shape[2:] != (c, h, w) or dst.stride(4) != 1 or dst.stride(3) != w or dst.stride(2) != h * w:
        raise _lib.RefidHipError("nhwc_to_nchw_tb: dst must be (B,T,c,H,W) with dense (c,H,W) blocks matching src")
    check(lib().refid_nhwc_to_nchw_tb(ptr, ld, dst.data_ptr(), dst.stride(0), dst.stride(1), b, t, c, h, w, _stream()),
          "refid_nhwc_to_nchw_tb")
    return dst


def nchw_tsum_to_nhwc(src, c_pad=None):
    """(N,T,C,H,W) contiguous -> sum over T as (N,H,W,c_pad)."""
    n, t, c, h, w = src.shape
    if not src.is_contiguous():
        raise _lib.RefidHipError("nchw_tsum_to_nhwc: contiguous (N,T,C,H,W) tensor required")
    c_pad = c_pad or ((c + 3) // 4) * 4
    dst = torch.empty((n, h, w, c_pad), dtype=torch.float32, device=src.device)
    check(lib().refid_nchw_tsum_to_nhwc(src.data_ptr(), t * c * h * w, c * h * w, t, dst.data_ptr(), n, c, h, w, c_pad,
                                        _stream()), "refid_nchw_tsum_to_nhwc")
    return dst


def nhwc_to_nchw(src, c, dst, dst_batch_stride=None):
    """First c channels of NHWC src -> NCHW dst (dst may be a (B,T,...) stack slice)."""
    ptr, ld = _nhwc(src, "src")
    n, h, w, _ = src.shape
    if dst_batch_stride is None:
        dst_batch_stride = c * h * w
    check(lib().refid_nhwc_to_nchw(ptr, ld, dst.data_ptr(), dst_batch_stride, n, c, h, w, _stream()),
          "refid_nhwc_to_nchw")
    return dst


def add(a, b, out=None):
    if out is None:
        out = torch.empty_like(a)
    if not (a.is_contiguous() and b.is_contiguous() and out.is_contiguous()) or a.shape != b.shape:
        raise _lib.RefidHipError("add: contiguous same-shape tensors required")
    check(lib().refid_add(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream()), "refid_add")
    return out


SUM_MAX = 48


def sum_n(tensors, out=None):
    """out = tensors[0] + tensors[1] + ... (index order; any number of same-shape contiguous tensors; out may be
    tensors[0]).  More than SUM_MAX inputs are summed in passes."""
    ts = list(tensors)
    if not ts:
        raise _lib.RefidHipError("sum_n: no inputs")
    if out is None:
        out = torch.empty_like(ts[0])
    for t in ts + [out]:
        if not t.is_contiguous() or t.shape != ts[0].shape or t.dtype != torch.float32:
            raise _lib.RefidHipError("sum_n: contiguous same-shape float32 tensors required")
    while True:
        part, ts = ts[:SUM_MAX], ts[SUM_MAX:]
        ptrs = (C.c_void_p * len(part))(*[t.data_ptr() for t in part])
        check(lib().refid_sum_n(ptrs, len(part), out.data_ptr(), out.numel(), _stream()), "refid_sum_n")
        if not ts:
            return out
        ts = [out] + ts


def act_bwd(g, y, slope, out=None, accumulate=False):
    """out (+)= g * (y > 0 ? 1 : slope)."""
    if out is None:
        out = torch.empty_like(g)
        accumulate = False
    if not (g.is_contiguous() and y.is_contiguous() and out.is_contiguous()) or g.shape != y.shape:
        raise _lib.RefidHipError("act_bwd: contiguous same-shape tensors required")
    check(lib().refid_act_bwd(g.data_ptr(), y.data_ptr(), out.data_ptr(), slope, int(accumulate), g.numel(), _stream()),
          "refid_act_bwd")
    return out


# ---------------------------------------------------------------------------------------------
# EGACA pieces / train-step tail.  Plain contiguous NHWC tensors unless a pitch is mentioned.
# ---------------------------------------------------------------------------------------------
def _c(t, name):
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
        raise _lib.RefidHipError(f"{name}: contiguous CUDA float32 tensor required")
    return t.data_ptr()


def layernorm2d_fwd(x, w, b, out=None, eps=1e-6):
    px, ld = _nhwc(x, "x")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    po, ldo = _nhwc(out, "out")
    npix = x.shape[0] * x.shape[1] * x.shape[2]
    check(lib().refid_layernorm2d_fwd(px, ld, _c(w, "w"), _c(b, "b"), po, ldo, npix, x.shape[3], eps, _stream()),
          "refid_layernorm2d_fwd")
    return out


def layernorm2d_bwd(g, x, w, gx, dw, db, accumulate=False, res=None, eps=1e-6):
    """gx = (res or 0) + LayerNorm2d backward; accumulate=True is res=gx (in place)."""
    pg, ldg = _nhwc(g, "g")
    px, ldx = _nhwc(x, "x")
    pgx, ldgx = _nhwc(gx, "gx")
    if accumulate and res is None:
        res = gx
    pr, ldr = _nhwc(res, "res") if res is not None else (None, 0)
    npix = x.shape[0] * x.shape[1] * x.shape[2]
    c = x.shape[3]
    nb = lib().refid_layernorm2d_bwd_parts(npix, c)
    if nb <= 0:
        raise _lib.RefidHipError(f"layernorm2d_bwd: unsupported channel count {c}")
    parts = torch.empty((nb, 2 * c), dtype=torch.float32, device=x.device)      # fixed-order partial sums of dw / db
    check(lib().refid_layernorm2d_bwd(pg, ldg, px, ldx, _c(w, "w"), pgx, ldgx, pr, ldr, _c(dw, "dw"),
                                      _c(db, "db"), parts.data_ptr(), npix, c, eps, _stream()), "refid_layernorm2d_bwd")
    _keep_rows(parts)
    return gx


def dwconv_pool_parts(h, w, c):
    return lib().refid_dwconv_pool_parts(h, w, c)


def dwconv3x3_gelu_fwd(x, w, b, want_pool=False):
    """Returns (pre, act) or (pre, act, pool_parts) with pool_parts (n, parts, c) per-workgroup sums of act."""
    px, ld = _nhwc(x, "x")
    n, h, wd, c = x.shape
    pre = torch.empty((n, h, wd, c), dtype=torch.float32, device=x.device)
    act = torch.empty_like(pre)
    pool = None
    if want_pool:
        parts = lib().refid_dwconv_pool_parts(h, wd, c)
        if parts <= 0:
            raise _lib.RefidHipError(f"dwconv3x3: unsupported channel count {c}")
        pool = torch.empty((n, parts, c), dtype=torch.float32, device=x.device)
    check(lib().refid_dwconv3x3_gelu_fwd(px, ld, _c(w, "w"), _c(b, "b"), pre.data_ptr(), act.data_ptr(),
                                         pool.data_ptr() if pool is not None else None, n, h, wd, c, _stream()),
          "refid_dwconv3x3_gelu_fwd")
    return (pre, act, pool) if want_pool else (pre, act)


def dwconv3x3_bwd(gd, x, w, dw, db):
    px, ld = _nhwc(x, "x")
    n, h, wd, c = x.shape
    gin = torch.empty((n, h, wd, c), dtype=torch.float32, device=x.device)
    nparts = lib().refid_dwconv3x3_bwd_parts(h, wd, c)
    if nparts <= 0:
        raise _lib.RefidHipError(f"dwconv3x3_bwd: unsupported channel count {c}")
    parts = torch.empty((n * nparts, 10 * c), dtype=torch.float32, device=x.device)
    check(lib().refid_dwconv3x3_bwd(_c(gd, "gd"), px, ld, _c(w, "w"), gin.data_ptr(), _c(dw, "dw"), _c(db, "db"),
                                    parts.data_ptr(), n, h, wd, c, _stream()), "refid_dwconv3x3_bwd")
    _keep_rows(parts)
    return gin


def se_fwd(pool, inv_hw, w1, b1, w2, b2):
    """pool: (n, parts, c) partial sums (or (n, c))."""
    if pool.dim() == 2:
        pool = pool.unsqueeze(1)
    n, parts, c = pool.shape
    m = torch.empty((n, c), dtype=torch.float32, device=pool.device)
    z1 = torch.empty((n, c // 2), dtype=torch.float32, device=pool.device)
    s = torch.empty_like(m)
    check(lib().refid_se_fwd(_c(pool, "pool"), parts, inv_hw, _c(w1, "w1"), _c(b1, "b1"), _c(w2, "w2"), _c(b2, "b2"),
                             m.data_ptr(), z1.data_ptr(), s.data_ptr(), n, c, _stream()), "refid_se_fwd")
    return m, z1, s


def se_bwd(gs, s, z1, m, w1, w2, dw1, db1, dw2, db2):
    n, c = gs.shape
    gm = torch.empty_like(gs)
    scratch = torch.empty((n, c + c // 2), dtype=torch.float32, device=gs.device)
    check(lib().refid_se_bwd(_c(gs, "gs"), _c(s, "s"), _c(z1, "z1"), _c(m, "m"), _c(w1, "w1"), _c(w2, "w2"),
                             gm.data_ptr(), _c(dw1, "dw1"), _c(db1, "db1"), _c(dw2, "dw2"), _c(db2, "db2"),
                             scratch.data_ptr(), n, c, _stream()), "refid_se_bwd")
    return gm


def scale_cat(xi, xe, s):
    n, h, w, c = xi.shape
    out = torch.empty((n, h, w, 2 * c), dtype=torch.float32, device=xi.device)
    check(lib().refid_scale_cat(_c(xi, "xi"), _c(xe, "xe"), _c(s, "s"), out.data_ptr(), n, h * w, c, _stream()),
          "refid_scale_cat")
    return out


def egaca_gs_reduce(gxs, xi, xe):
    n, h, w, c = xi.shape
    gs = torch.empty((n, c), dtype=torch.float32, device=xi.device)
    nb = lib().refid_egaca_gs_reduce_parts(h * w, c)
    if nb <= 0:
        raise _lib.RefidHipError(f"egaca_gs_reduce: unsupported channel count {c}")
    parts = torch.empty((n, nb, c), dtype=torch.float32, device=xi.device)
    check(lib().refid_egaca_gs_reduce(_c(gxs, "gxs"), _c(xi, "xi"), _c(xe, "xe"), gs.data_ptr(), parts.data_ptr(), n,
                                      h * w, c, _stream()), "refid_egaca_gs_reduce")
    return gs


def egaca_bwd_elem(gxs, s, gm, dwe, gxi, accumulate_xi):
    n, h, w, c = dwe.shape
    gdwe = torch.empty_like(dwe)
    check(lib().refid_egaca_bwd_elem(_c(gxs, "gxs"), _c(s, "s"), _c(gm, "gm"), 1.0 / (h * w), _c(dwe, "dwe"),
                                     gdwe.data_ptr(), _c(gxi, "gxi"), int(accumulate_xi), n, h * w, c, _stream()),
          "refid_egaca_bwd_elem")
    return gdwe


def gelu_fwd(x):
    out = torch.empty_like(x)
    check(lib().refid_gelu_fwd(_c(x, "x"), out.data_ptr(), x.numel(), _stream()), "refid_gelu_fwd")
    return out


def gelu_bwd(g, x, out=None):
    if out is None:
        out = torch.empty_like(x)
    check(lib().refid_gelu_bwd(_c(g, "g"), _c(x, "x"), out.data_ptr(), x.numel(), _stream()), "refid_gelu_bwd")
    return out


def colsum(g, db):
    pg, ld = _nhwc(g, "g")
    npix = g.shape[0] * g.shape[1] * g.shape[2]
    nb = lib().refid_colsum_parts(npix, g.shape[3])
    if nb <= 0:
        raise _lib.RefidHipError(f"colsum: unsupported channel count {g.shape[3]}")
    parts = torch.empty((nb, g.shape[3]), dtype=torch.float32, device=g.device)
    check(lib().refid_colsum(pg, ld, _c(db, "db"), parts.data_ptr(), npix, g.shape[3], _stream()), "refid_colsum")
    _keep_rows(parts)


class PackPlan:
    """All weight packings of a model as ONE launch (refid_pack_batch).  add_* mirror pack_conv_weights[_bf16 / _split /
    _wino6] and mul_vec with preallocated outputs; the tensors must stay alive and in place (parameter arena, packed
    buffers).  run() after every optimiser step."""

    def __init__(self, device):
        self.device = device
        self.esz = lib().refid_pack_entry_bytes()
        self.items = []
        self.keep = []
        self.table = None
        self.nblocks = 0

    def _add(self, kind, w, oscale, dst, role=0, o=0, i=0, kh=1, kw=1, kc=8, bn=32, planes=0):
        if self.table is not None:
            raise _lib.RefidHipError("PackPlan: already built")
        for t in (w, oscale, dst):
            if t is not None and not t.is_contiguous():
                raise _lib.RefidHipError("PackPlan: tensors must be contiguous")
        self.items.append((kind, w, oscale, dst, role, o, i, kh, kw, kc, bn, planes))
        self.keep += [w, oscale, dst]

    def add_form(self, form, w, geo, out, oscale=None):
        f = _FORMS[form]
        self._add(f.kind, w, oscale, out, **dict(geo, planes=geo["planes"] if f.planes is None else f.planes))

    def add_pack(self, w, role, bn, kc, kh, kw, o, i, out, oscale=None, bf16=False):
        self.add_form("bf16" if bf16 else "f32", w, pack_geo(role, o, i, kh, kw, kc, bn), out, oscale)

    def add_split(self, w, role, bn, kh, kw, o, i, planes, out, oscale=None, f16=False):
        self.add_form(split_form(kh, kw, f16), w, pack_geo(role, o, i, kh, kw, 8, bn, planes), out, oscale)

    def add_wino6(self, w, role, o, i, out, oscale=None, f16=False, terms=None):
        self.add_form(wino6_form(f16, terms), w, pack_geo(role, o, i), out, oscale)

    def add_mul_vec(self, a, b, out):
        self._add(4, a, b, out, o=a.numel())

    def build(self):
        L = lib()
        buf = (C.c_char * (self.esz * len(self.items)))()
        blk = 0
        for n, (kind, w, oscale, dst, role, o, i, kh, kw, kc, bn, planes) in enumerate(self.items):
            nb = L.refid_pack_entry_fill(C.addressof(buf) + n * self.esz, kind, w.data_ptr(),
                                         oscale.data_ptr() if oscale is not None else None, dst.data_ptr(), role, o, i, kh, kw,
                                         kc, bn, planes, blk)
            if nb <= 0:
                raise _lib.RefidHipError(f"refid_pack_entry_fill (record {n}, kind {kind}): " + L.refid_last_error().decode())
            blk += nb
        # every record filled, first blocks consecutive from 0 (the kernel's binary search relies on it)
        if L.refid_pack_table_check(C.addressof(buf), len(self.items)) != blk:
            raise _lib.RefidHipError("refid_pack_table_check: " + L.refid_last_error().decode())
        self.nblocks = blk
        self.table = torch.frombuffer(bytearray(bytes(buf)), dtype=torch.uint8).to(self.device)
        return self

    def run(self):
        if any(it[0] in (5, 6) for it in self.items):       # the fp16 packings' scale exponents (max |w| per tensor) first
            check(lib().refid_pack_batch_prepass(self.table.data_ptr(), len(self.items), _stream()), "refid_pack_batch_prepass")
        check(lib().refid_pack_batch(self.table.data_ptr(), len(self.items), self.nblocks, _stream()), "refid_pack_batch")


def mul_vec(a, b, out=None):
    if out is None:
        out = torch.empty_like(a)
    check(lib().refid_mul_vec(_c(a, "a"), _c(b, "b"), out.data_ptr(), a.numel(), _stream()), "refid_mul_vec")
    return out


def fold_back(w, b, scale, gw_folded, gb_folded, gw, gb, dscale):
    """Un-fold the gradient of (scale[r]*W[r,:], scale[r]*b[r]) accumulated in gw_folded/gb_folded:
    dscale[r] += <W[r,:],Gf[r,:]> + b[r]*gbf[r];  gw[r,:] += scale[r]*Gf[r,:];  gb[r] += scale[r]*gbf[r]."""
    rows = scale.numel()
    k = w.numel() // rows
    check(lib().refid_fold_back(_c(w, "w"), _c(b, "b"), _c(scale, "scale"), _c(gw_folded, "gw_folded"),
                                _c(gb_folded, "gb_folded"), _c(gw, "gw"), _c(gb, "gb"), _c(dscale, "dscale"), rows, k,
                                _stream()), "refid_fold_back")


def charbonnier(pred, gt, grad=None, eps=1e-12, grad_scale=None):
    """Returns the device double holding sum sqrt((pred-gt)^2+eps); grad (optional) gets d/dpred of the MEAN.
    Two-stage, deterministic: buf[0] = the sum, buf[1:] = the per-workgroup partials."""
    n = pred.numel()
    buf = torch.empty(1 + lib().refid_charbonnier_parts(n), dtype=torch.float64, device=pred.device)
    if grad_scale is None:
        grad_scale = 1.0 / n
    check(lib().refid_charbonnier(_c(pred, "pred"), _c(gt, "gt"), grad.data_ptr() if grad is not None else None,
                                  buf.data_ptr(), buf[1:].data_ptr(), n, eps, grad_scale, _stream()), "refid_charbonnier")
    return buf[:1]


def psnr_loss(pred, gt, grad=None, weight=1.0, want_sq=False):
    """PSNRLoss (losses.py:95-120) of (B, ...) tensors; returns the 1-element double device tensor holding the loss
    (want_sq: and the per-sample sums of squared differences, (B,) doubles)."""
    nb = pred.shape[0]
    per = pred.numel() // nb
    buf = torch.empty(nb + 1 + lib().refid_psnr_loss_parts(nb, per), dtype=torch.float64, device=pred.device)
    check(lib().refid_psnr_loss(_c(pred, "pred"), _c(gt, "gt"), grad.data_ptr() if grad is not None else None,
                                buf.data_ptr(), buf[nb:].data_ptr(), buf[nb + 1:].data_ptr(), nb, per, weight, _stream()),
          "refid_psnr_loss")
    return (buf[nb:nb + 1], buf[:nb]) if want_sq else buf[nb:nb + 1]


SQNORM_WORDS = 2049


def grad_sqnorm(flat_g, out=None):
    """out[0] = sum g^2; `out` holds SQNORM_WORDS doubles (result + scratch for the block partials)."""
    if out is None:
        out = torch.empty(SQNORM_WORDS, dtype=torch.float64, device=flat_g.device)
    elif out.numel() < SQNORM_WORDS:
        raise _lib.RefidHipError("grad_sqnorm: out needs SQNORM_WORDS doubles")
    check(lib().refid_grad_sqnorm(_c(flat_g, "g"), out.data_ptr(), flat_g.numel(), _stream()), "refid_grad_sqnorm")
    return out


def clip_adamw(p, g, m, v, sqnorm, *, max_norm, lr, betas, eps, weight_decay, step, grad_scale=1.0):
    check(lib().refid_clip_adamw(_c(p, "p"), _c(g, "g"), _c(m, "m"), _c(v, "v"),
                                 sqnorm.data_ptr() if sqnorm is not None else None, max_norm, grad_scale, lr,
                                 betas[0], betas[1], eps, weight_decay, step, p.numel(), _stream()),
          "refid_clip_adamw")


def clip_adamw_dev(p, g, m, v, sqnorm, hyper, *, max_norm, betas, eps, weight_decay, grad_scale=1.0):
    """clip_adamw with (lr, 1 - beta1^t, sqrt(1 - beta2^t)) read from the 3-float device tensor `hyper`."""
    check(lib().refid_clip_adamw_dev(_c(p, "p"), _c(g, "g"), _c(m, "m"), _c(v, "v"),
                                     sqnorm.data_ptr() if sqnorm is not None else None, max_norm, grad_scale,
                                     _c(hyper, "hyper"), betas[0], betas[1], eps, weight_decay, p.numel(), _stream()),
          "refid_clip_adamw_dev")


# ---------------------------------------------------------------------------------------------
# SingleMultiConnectEVHINet non-GEMM pieces (csrc/evhinet.hip)
# ---------------------------------------------------------------------------------------------
def hin_lrelu_fwd(x, gamma, beta, slope=0.2, eps=1e-5, out=None):
    """LeakyReLU([InstanceNorm(x[..., :ch]) * gamma + beta | x[..., ch:]]), ch = len(gamma) (None: plain LeakyReLU).
    Returns (out, stats) with stats (n, 2, ch) = mean / rstd (None when ch == 0); `out` may be a channel slice."""
    px, ld = _nhwc(x, "x")
    n, h, w, c = x.shape
    ch = 0 if gamma is None else gamma.numel()
    if out is None:
        out = torch.empty((n, h, w, c), dtype=torch.float32, device=x.device)
    po, ldo = _nhwc(out, "out")
    stats = parts = None
    if ch:
        stats = torch.empty((n, 2, ch), dtype=torch.float32, device=x.device)
        parts = torch.empty((n, lib().refid_hin_parts(h * w), 2, ch), dtype=torch.float32, device=x.device)
    check(lib().refid_hin_lrelu_fwd(px, ld, _c(gamma, "gamma") if ch else None, _c(beta, "beta") if ch else None,
                                    po, ldo, stats.data_ptr() if ch else None,
                                    parts.data_ptr() if ch else None, n, h * w, c, ch, eps, slope, _stream()),
          "refid_hin_lrelu_fwd")
    return out, stats


def hin_lrelu_bwd(g, out, x, gamma, stats, dgamma, dbeta, slope=0.2, gx=None):
    """Gradient w.r.t. x of hin_lrelu_fwd; dgamma / dbeta accumulate; `gx` may be a channel slice."""
    pg, ldg = _nhwc(g, "g")
    po, ldo = _nhwc(out, "out")
    n, h, w, c = out.shape
    ch = 0 if gamma is None else gamma.numel()
    if gx is None:
        gx = torch.empty((n, h, w, c), dtype=torch.float32, device=g.device)
    pgx, ldgx = _nhwc(gx, "gx")
    px, ldx = _nhwc(x, "x") if ch else (None, 0)
    sums = parts = None
    if ch:
        sums = torch.empty((n, 2, ch), dtype=torch.float32, device=g.device)
        parts = torch.empty((n, lib().refid_hin_parts(h * w), 2, ch), dtype=torch.float32, device=g.device)
    check(lib().refid_hin_lrelu_bwd(pg, ldg, po, ldo, px, ldx, _c(gamma, "gamma") if ch else None,
                                    _c(stats, "stats") if ch else None, pgx, ldgx,
                                    _c(dgamma, "dgamma") if ch else None, _c(dbeta, "dbeta") if ch else None,
                                    sums.data_ptr() if ch else None, parts.data_ptr() if ch else None, n, h * w, c, ch,
                                    slope, _stream()), "refid_hin_lrelu_bwd")
    return gx


def fac_fwd(feat, filt, out=None):
    """FAC_bias: feat * filt[..., :C] + filt[..., C:]."""
    pf, ldf = _nhwc(feat, "feat")
    pi, ldi = _nhwc(filt, "filt")
    n, h, w, c = feat.shape
    if filt.shape[3] != 2 * c:
        raise _lib.RefidHipError(f"fac_fwd: filter has {filt.shape[3]} channels, expected {2 * c}")
    if out is None:
        out = torch.empty((n, h, w, c), dtype=torch.float32, device=feat.device)
    po, ldo = _nhwc(out, "out")
    check(lib().refid_fac_fwd(pf, ldf, pi, ldi, po, ldo, n * h * w, c, _stream()), "refid_fac_fwd")
    return out


def fac_bwd(g, feat, filt, gfeat=None, gfilt=None):
    """Returns (g_feat, g_filt); either may be given as a channel slice of a wider buffer."""
    pg, ldg = _nhwc(g, "g")
    pf, ldf = _nhwc(feat, "feat")
    pi, ldi = _nhwc(filt, "filt")
    n, h, w, c = feat.shape
    if gfeat is None:
        gfeat = torch.empty((n, h, w, c), dtype=torch.float32, device=g.device)
    if gfilt is None:
        gfilt = torch.empty((n, h, w, 2 * c), dtype=torch.float32, device=g.device)
    pgf, ldgf = _nhwc(gfeat, "gfeat")
    pgfi, ldgfi = _nhwc(gfilt, "gfilt")
    check(lib().refid_fac_bwd(pg, ldg, pf, ldf, pi, ldi, pgf, ldgf, pgfi, ldgfi, n * h * w, c, _stream()), "refid_fac_bwd")
    return gfeat, gfilt


def assemble_bins(m, n, layout):
    """Voxel bins of a batch-assembly layout (_lib.LAYOUT_BLUR: 2m+n+1, LAYOUT_SHARP: n+1); raises on an unsupported one."""
    bins = lib().refid_assemble_bins(int(m), int(n), int(layout))
    if bins < 0:
        raise _lib.RefidHipError("refid_assemble_bins: " + lib().refid_last_error().decode("utf-8", "replace"))
    return bins


def assemble_batch(desc, stages=_lib.ASSEMBLE_ALL):
    """Runs the batch-assembly kernels of csrc/sample.hip for an _lib.AssembleDesc on the current stream."""
    check(lib().refid_assemble_batch(C.byref(desc), int(stages), _stream()), "refid_assemble_batch")


def seq_assemble(desc, stages=_lib.ASSEMBLE_ALL):
    """Runs the pair-assembly kernels of csrc/sequence.hip for an _lib.SeqDesc on the current stream."""
    check(lib().refid_seq_assemble(C.byref(desc), int(stages), _stream()), "refid_seq_assemble")


ASSEMBLE_STATS = _lib.ASSEMBLE_STATS


def single_bins(bins):
    """Checks the bin count of the single-image layout (>= 1, not 3); raises on an unsupported one."""
    rc = lib().refid_single_bins(int(bins))
    if rc < 0:
        raise _lib.RefidHipError("refid_single_bins: " + lib().refid_last_error().decode("utf-8", "replace"))
    return rc


def voxel_norm_parts(batch, per_sample, device):
    """The scratch of voxel_norm's statistics pass for (batch, per_sample): an int64 tensor of 8-byte words."""
    return torch.empty(lib().refid_voxel_norm_parts(int(batch), int(per_sample)), dtype=torch.int64, device=device)


def voxel_norm(x, out=None):
    """voxel_norm (event_util.py:141-160) of every sample of a float32 CUDA tensor (B, ...): (x - mean) / std over each
    sample's non-zero elements, zeros stay zero; a sample without spread becomes all zeros (the reference: NaN).
    Deterministic (include/refid_hip.h).  ``out`` may be ``x``."""
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() < 2 or not x.is_contiguous() or x.numel() == 0:
        raise _lib.RefidHipError("voxel_norm: a non-empty contiguous float32 CUDA tensor (B, ...) is required")
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
        raise _lib.RefidHipError("voxel_norm: out must match x")
    batch, per = x.shape[0], x.numel() // x.shape[0]
    parts = voxel_norm_parts(batch, per, x.device)
    check(lib().refid_voxel_norm(x.data_ptr(), out.data_ptr(), batch, per, parts.data_ptr(), _stream()), "refid_voxel_norm")
    return out


def assemble_single(desc, stages=_lib.ASSEMBLE_ALL | _lib.ASSEMBLE_STATS):
    """Runs the single-image assembly of csrc/sample.hip for an _lib.SingleDesc on the current stream."""
    check(lib().refid_assemble_single(C.byref(desc), int(stages), _stream()), "refid_assemble_single")


def seq_assemble_single(desc, stages=_lib.ASSEMBLE_ALL | _lib.ASSEMBLE_STATS):
    """Runs the single-image item assembly of csrc/sequence.hip for an _lib.SeqSingleDesc on the current stream."""
    check(lib().refid_seq_assemble_single(C.byref(desc), int(stages), _stream()), "refid_seq_assemble_single")


def niqe_moments(u8, window, bgr=False, crop_border=0, planes=False):
    """refid_niqe_moments (csrc/niqe.hip) on the current stream: ``u8`` uint8 CUDA (..., H, W, 3), ``window`` the 49 float64
    weights on the device -> float64 sums (nf, 2 scales, blocks, 5 maps, 5) in the layout of include/refid_hip.h.
    ``planes=True`` also returns the float32 [Y, MSCN scale 1, MSCN scale 2] planes.  Does not synchronise."""
    if not u8.is_cuda or u8.dtype != torch.uint8 or u8.dim() < 3 or u8.shape[-1] != 3 or u8.numel() == 0:
        raise _lib.RefidHipError("niqe_moments: a non-empty uint8 CUDA tensor (..., H, W, 3) is required")
    if not window.is_cuda or window.dtype != torch.float64 or window.numel() != 49 or not window.is_contiguous():
        raise _lib.RefidHipError("niqe_moments: window must hold 49 contiguous float64 weights on the device")
    u8 = u8.contiguous()
    h, w, cb = int(u8.shape[-3]), int(u8.shape[-2]), int(crop_border)
    nf = u8.numel() // (3 * h * w)
    if cb < 0 or h - 2 * cb < 96 or w - 2 * cb < 96:
        raise _lib.RefidHipError(f"niqe_moments: a {h}x{w} frame with crop_border {cb} holds no 96x96 block")
    hc, wc = (h - 2 * cb) // 96 * 96, (w - 2 * cb) // 96 * 96
    sums = torch.empty((nf, 2, (hc // 96) * (wc // 96), 5, 5), dtype=torch.float64, device=u8.device)
    words = lib().refid_niqe_moments_parts(nf, h, w)
    parts = torch.empty(words, dtype=torch.int64, device=u8.device) if words > 0 else None
    outs = [torch.empty((nf, hc // s, wc // s), dtype=torch.float32, device=u8.device) for s in (1, 1, 2)] if planes else [None] * 3
    ptr = lambda t: None if t is None else t.data_ptr()       # noqa: E731
    check(lib().refid_niqe_moments(u8.data_ptr(), nf, h, w, _lib.NIQE_BGR if bgr else 0, cb, window.data_ptr(), sums.data_ptr(),
                                   ptr(parts), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), _stream()), "refid_niqe_moments")
    return (sums, outs) if planes else sums


def png_unfilter(rows_u8, n, h, w, channels, out=None, split_bands=True, bands=None):
    """refid_png_unfilter (csrc/png.hip) on the current stream: ``rows_u8`` holds the inflate output of ``n`` PNGs of one
    (h, w, channels) -- uint8 on the device, n*h*(1 + w*channels) bytes, filter byte first in every row -> uint8
    (n, h, w, 3), a grey file replicated to three channels.  ``out``: a contiguous uint8 (n, h, w, 3) view to write into.
    ``split_bands``: one wave per band of rows that does not read the row above it (``png.find_bands``) instead of one per
    frame; the bytes are the same.  ``bands``: that int32 (n_bands, 3) table from a caller that holds the filter bytes on
    the host and has checked them; without it the filter-byte column is copied back and checked here, which
    synchronises.  Does not synchronise otherwise."""
    import numpy as np
    from . import png
    n, h, w, channels = int(n), int(h), int(w), int(channels)
    if channels not in (1, 3) or min(n, h, w) < 1:
        raise _lib.RefidHipError(f"png_unfilter: n={n}, h={h}, w={w} must be positive and channels={channels} 1 or 3")
    if w * channels > _lib.PNG_MAX_ROW_BYTES:
        raise _lib.RefidHipError(f"png_unfilter: rows of {w * channels} bytes exceed the kernel's line of "
                                 f"{_lib.PNG_MAX_ROW_BYTES} (decode such files on the host)")
    pitch = 1 + w * channels
    if not rows_u8.is_cuda or rows_u8.dtype != torch.uint8 or not rows_u8.is_contiguous() or rows_u8.numel() != n * h * pitch:
        raise _lib.RefidHipError(f"png_unfilter: rows must be a contiguous uint8 CUDA tensor of {n}*{h}*{pitch} bytes, got "
                                 f"{rows_u8.dtype} {tuple(rows_u8.shape)} on {rows_u8.device}")
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=rows_u8.device)
    elif out.dtype != torch.uint8 or out.device != rows_u8.device or tuple(out.shape) != (n, h, w, 3) or not out.is_contiguous():
        raise _lib.RefidHipError(f"png_unfilter: out must be a contiguous uint8 ({n}, {h}, {w}, 3) tensor on {rows_u8.device}")
    table = None
    if bands is not None:
        table = np.ascontiguousarray(np.asarray(bands, dtype=np.int32).reshape(-1, 3))
    else:
        filters = png.check_filters(rows_u8.view(n, h, pitch)[:, :, 0].cpu().numpy())
        if split_bands:
            table = png.find_bands(filters)
    if table is not None:
        if not len(table) or table[:, 0].min() < 0 or table[:, 0].max() >= n or (table[:, 1] < 0).any() or \
                (table[:, 2] > h).any() or (table[:, 1] >= table[:, 2]).any():
            raise _lib.RefidHipError(f"png_unfilter: a band lies outside the {n} frames of {h} rows")
        table = torch.from_numpy(table).pin_memory().to(rows_u8.device, non_blocking=True)
    desc = _lib.PngUnfilterDesc(rows=rows_u8.data_ptr(), frames=out.data_ptr(), bands=None if table is None else table.data_ptr(),
                                n_bands=0 if table is None else int(table.shape[0]), n_frames=n, height=h, width=w,
                                channels=channels)
    check(lib().refid_png_unfilter(C.byref(desc), _stream()), "refid_png_unfilter")
    return out


def png_filter(frames_u8, mode="adaptive", out=None, costs=None):
    """refid_png_filter (csrc/png_filter.hip) on the current stream: uint8 CUDA frames (N, H, W, 3) -> the filtered rows of
    N PNGs, uint8 (N, H, 1 + 3W), the filter byte first in every row: what ``png.encode_png_rows`` deflates and what
    ``png_unfilter`` reads.  ``mode``: 'adaptive' (per row the type with the least sum of |residual as int8|, the lowest
    type on a tie) or a type number 0..4 (None, Sub, Up, Average, Paeth) for every row.  ``out``: a contiguous uint8
    tensor of N*H*(1 + 3W) elements to write into (any alignment; nothing outside it is written); the result is a view of
    it.  ``costs``: an int32 tensor (N, H, 5) that receives the five sums of every row (the bits of the header's
    uint32).  Does not synchronise."""
    f = frames_u8
    if not isinstance(f, torch.Tensor) or not f.is_cuda or f.dtype != torch.uint8 or f.dim() != 4 or f.shape[-1] != 3 or \
            f.numel() == 0 or not f.is_contiguous():
        raise _lib.RefidHipError("png_filter: a non-empty contiguous uint8 CUDA tensor (N, H, W, 3) is required, got "
                                 + (f"{f.dtype} {tuple(f.shape)} on {f.device}" if isinstance(f, torch.Tensor) else type(f).__name__))
    if mode != "adaptive" and not (type(mode) is int and 0 <= mode <= 4):
        raise _lib.RefidHipError(f"png_filter: mode {mode!r} is neither 'adaptive' nor a type number 0..4")
    code = _lib.PNG_FILTER_ADAPTIVE if mode == "adaptive" else mode
    n, h, w = int(f.shape[0]), int(f.shape[1]), int(f.shape[2])
    if w > _lib.PNG_FILTER_MAX_WIDTH:
        raise _lib.RefidHipError(f"png_filter: width {w} exceeds {_lib.PNG_FILTER_MAX_WIDTH} (write such frames with filter 0)")
    pitch = 1 + 3 * w
    if out is None:
        out = torch.empty((n, h, pitch), dtype=torch.uint8, device=f.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != f.device or \
            out.numel() != n * h * pitch or not out.is_contiguous():
        raise _lib.RefidHipError(f"png_filter: out must be a contiguous uint8 tensor of {n}*{h}*{pitch} elements on {f.device}")
    if costs is not None and (not isinstance(costs, torch.Tensor) or costs.dtype != torch.int32 or costs.device != f.device or
                              tuple(costs.shape) != (n, h, 5) or not costs.is_contiguous()):
        raise _lib.RefidHipError(f"png_filter: costs must be a contiguous int32 ({n}, {h}, 5) tensor on {f.device}")
    desc = _lib.PngFilterDesc(frames=f.data_ptr(), rows=out.data_ptr(), costs=None if costs is None else costs.data_ptr(),
                              n_frames=n, height=h, width=w, mode=code)
    check(lib().refid_png_filter(C.byref(desc), _stream()), "refid_png_filter")
    return out.view(n, h, pitch)


def png_deflate(rows, block_bytes=None, out=None):
    """refid_png_deflate (csrc/png_deflate.hip) on the current stream: uint8 CUDA ``rows`` (N, H, 1 + 3W) -- what
    ``png_filter`` returns -- or (N, bytes) -> (out uint8 (N, pitch), lens int32 (N,)): row n of ``out`` begins with the
    zlib stream of ``rows[n]``, ``lens[n]`` bytes long (Huffman codes only, one code per block of ``block_bytes`` input
    bytes, 1 .. 65535; default ``_lib.PNG_DEFLATE_BLOCK``); what ``png.wrap_zlib_stream`` puts into an IDAT chunk.  The
    bytes behind a stream are left as they were.  ``out``: a contiguous uint8 (N, pitch) tensor to write into (any
    alignment), pitch >= ``refid_png_deflate_bound``; without it the pitch is that bound.  Does not synchronise."""
    r = rows
    if not isinstance(r, torch.Tensor) or not r.is_cuda or r.dtype != torch.uint8 or r.dim() not in (2, 3) or r.numel() == 0 or \
            not r.is_contiguous():
        raise _lib.RefidHipError("png_deflate: a non-empty contiguous uint8 CUDA tensor (N, H, 1 + 3W) or (N, bytes) is required, got "
                                 + (f"{r.dtype} {tuple(r.shape)} on {r.device}" if isinstance(r, torch.Tensor) else type(r).__name__))
    block = _lib.PNG_DEFLATE_BLOCK if block_bytes is None else block_bytes
    if type(block) is not int or not 1 <= block <= _lib.PNG_DEFLATE_MAX_BLOCK:
        raise _lib.RefidHipError(f"png_deflate: block_bytes {block_bytes!r} is not an integer 1 .. {_lib.PNG_DEFLATE_MAX_BLOCK}")
    n, size = int(r.shape[0]), r.numel() // int(r.shape[0])
    L = lib()
    bound = L.refid_png_deflate_bound(size, block) if size < 2 ** 31 else 0
    work_bytes = L.refid_png_deflate_work_bytes(n, size, block) if bound else 0
    if not work_bytes:
        raise _lib.RefidHipError(f"png_deflate: {n} streams of {size} bytes in blocks of {block} exceed the grid or a 31-bit stream")
    if out is None:
        out = torch.empty((n, bound), dtype=torch.uint8, device=r.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != r.device or out.dim() != 2 or \
            out.shape[0] != n or out.shape[1] < bound or out.shape[1] >= 2 ** 31 or not out.is_contiguous():
        raise _lib.RefidHipError(f"png_deflate: out must be a contiguous uint8 ({n}, >= {bound}) tensor on {r.device}")
    lens = torch.empty((n,), dtype=torch.int32, device=r.device)
    work = torch.empty((work_bytes // 4,), dtype=torch.int32, device=r.device)
    desc = _lib.PngDeflateDesc(src=r.data_ptr(), out=out.data_ptr(), lens=lens.data_ptr(), work=work.data_ptr(), n_streams=n,
                               stream_bytes=size, block_bytes=block, out_pitch=int(out.shape[1]))
    check(L.refid_png_deflate(C.byref(desc), _stream()), "refid_png_deflate")
    return out, lens


JPEG_SUBSAMPLINGS = {"444": _lib.JPEG_444, "420": _lib.JPEG_420}


def jpeg_default_pitch(height, width):
    """The pitch ``jpeg_encode`` takes without one: the header and 3 bytes per pixel, rounded up to 4."""
    return (_lib.JPEG_HEADER_BYTES + 3 * height * width + 3) // 4 * 4


def jpeg_encode(frames_u8, quality=90, subsampling="420", restart_mcus=None, pitch=None, out=None):
    """refid_jpeg_encode (csrc/jpeg.hip) on the current stream: uint8 CUDA RGB ``frames_u8`` (N, H, W, 3) -- what
    ``val_tail`` writes -- -> (out uint8 (N, pitch), lens int32 (N,)): row n of ``out`` begins with the baseline JFIF file
    of frame n, ``lens[n]`` bytes long; a frame whose file does not fit the pitch has ``lens[n]`` = -(bytes needed).
    ``quality`` 1 .. 100, ``subsampling`` '420' or '444', ``restart_mcus`` 1 .. 65535 MCUs per restart interval (None: one
    MCU row).  ``pitch``: None = the header and 3 bytes per pixel, rounded up to 4 (every natural frame fits), 'bound' =
    ``refid_jpeg_bound`` (every frame fits), or an integer; ``out``: a contiguous uint8 (N, pitch) tensor to write into (any
    alignment), its width is then the pitch.  The bytes behind a file are left as they were.  Does not synchronise."""
    f = frames_u8
    if not isinstance(f, torch.Tensor) or not f.is_cuda or f.dtype != torch.uint8 or f.dim() != 4 or f.shape[-1] != 3 or f.numel() == 0 or \
            not f.is_contiguous():
        raise _lib.RefidHipError("jpeg_encode: a non-empty contiguous uint8 CUDA tensor (N, H, W, 3) is required, got "
                                 + (f"{f.dtype} {tuple(f.shape)} on {f.device}" if isinstance(f, torch.Tensor) else type(f).__name__))
    if type(quality) is not int or not 1 <= quality <= 100:
        raise _lib.RefidHipError(f"jpeg_encode: quality {quality!r} is not an integer 1 .. 100")
    if subsampling not in JPEG_SUBSAMPLINGS:
        raise _lib.RefidHipError(f"jpeg_encode: subsampling {subsampling!r} is not one of {sorted(JPEG_SUBSAMPLINGS)}")
    if restart_mcus is not None and (type(restart_mcus) is not int or not 1 <= restart_mcus <= 65535):
        raise _lib.RefidHipError(f"jpeg_encode: restart_mcus {restart_mcus!r} is not None or an integer 1 .. 65535")
    n, h, w = int(f.shape[0]), int(f.shape[1]), int(f.shape[2])
    ss, restart = JPEG_SUBSAMPLINGS[subsampling], restart_mcus or 0
    L = lib()
    bound = L.refid_jpeg_bound(h, w, ss, restart) if h <= 65535 and w <= 65535 else 0
    work_bytes = L.refid_jpeg_work_bytes(n, h, w, ss, restart) if bound else 0
    if not work_bytes:
        raise _lib.RefidHipError(f"jpeg_encode: {n} frames of {h}x{w} exceed 65535 a side, the grid or a 31-bit file")
    least = _lib.JPEG_HEADER_BYTES + 2
    if out is not None:
        if pitch is not None:
            raise _lib.RefidHipError("jpeg_encode: give pitch or out, not both (the width of out is the pitch)")
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != f.device or out.dim() != 2 or \
                out.shape[0] != n or out.shape[1] < least or out.shape[1] >= 2 ** 31 or not out.is_contiguous():
            raise _lib.RefidHipError(f"jpeg_encode: out must be a contiguous uint8 ({n}, >= {least}) tensor on {f.device}")
    else:
        if pitch is None:
            pitch = min(jpeg_default_pitch(h, w), 2 ** 31 - 1)
        elif pitch == "bound":
            pitch = bound
        elif type(pitch) is not int or not least <= pitch < 2 ** 31:
            raise _lib.RefidHipError(f"jpeg_encode: pitch {pitch!r} is not None, 'bound' or an integer {least} .. 2^31 - 1")
        out = torch.empty((n, pitch), dtype=torch.uint8, device=f.device)
    lens = torch.empty((n,), dtype=torch.int32, device=f.device)
    work = torch.empty((work_bytes // 4,), dtype=torch.int32, device=f.device)
    desc = _lib.JpegDesc(frames=f.data_ptr(), out=out.data_ptr(), lens=lens.data_ptr(), work=work.data_ptr(), n_frames=n, height=h,
                         width=w, quality=quality, subsampling=ss, restart_mcus=restart, out_pitch=int(out.shape[1]))
    check(L.refid_jpeg_encode(C.byref(desc), _stream()), "refid_jpeg_encode")
    return out, lens


JPEG_DECODE_SAMPLINGS = {"grey": _lib.JPEG_DEC_GREY, "444": _lib.JPEG_DEC_444, "422": _lib.JPEG_DEC_422, "420": _lib.JPEG_DEC_420}


def jpeg_decode_blocks(h, w, sampling):
    """(blocks per component [3], their sum) of a frame: the first dimension of one frame's ``coefs`` (host only, no GPU)."""
    if sampling not in JPEG_DECODE_SAMPLINGS:
        raise _lib.RefidHipError(f"jpeg_decode: sampling {sampling!r} is not one of {sorted(JPEG_DECODE_SAMPLINGS)}")
    blocks = (C.c_int32 * 3)()
    total = lib().refid_jpeg_decode_blocks(int(h), int(w), JPEG_DECODE_SAMPLINGS[sampling], blocks) if max(int(h), int(w)) < 2 ** 31 else 0
    if total <= 0:
        raise _lib.RefidHipError(f"jpeg_decode: height {h} and width {w} must be 1 .. 65535")
    return list(blocks), total


def jpeg_decode(coefs, quant, n, h, w, sampling, out=None):
    """refid_jpeg_decode (csrc/jpeg_decode.hip) on the current stream: the quantised coefficients ``coefs`` int16
    (n, total_blocks, 64) and tables ``quant`` uint16 or int16 (n, components, 64) of ``n`` JPEG files of one (h, w, sampling)
    -- what ``jpeg.entropy_decode`` writes, on the device -> uint8 (n, h, w, 3) RGB, a grey file replicated to three
    channels.  ``sampling``: 'grey', '444', '422' or '420'.  ``out``: a contiguous uint8 (n, h, w, 3) view to write into
    (any alignment; nothing outside it is written).  The scratch between the two launches is allocated here.  Does not
    synchronise."""
    n, h, w = int(n), int(h), int(w)
    if n < 1:
        raise _lib.RefidHipError(f"jpeg_decode: n={n} must be positive")
    blocks, total = jpeg_decode_blocks(h, w, sampling)
    comps = 1 if sampling == "grey" else 3
    if not isinstance(coefs, torch.Tensor) or not coefs.is_cuda or coefs.dtype != torch.int16 or not coefs.is_contiguous() or \
            coefs.numel() != n * total * 64:
        raise _lib.RefidHipError(f"jpeg_decode: coefs must be a contiguous int16 CUDA tensor of {n}*{total}*64 elements (no CPU fallback), got "
                                 + (f"{coefs.dtype} {tuple(coefs.shape)} on {coefs.device}" if isinstance(coefs, torch.Tensor) else type(coefs).__name__))
    if not isinstance(quant, torch.Tensor) or quant.device != coefs.device or quant.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16)) or \
            not quant.is_contiguous() or quant.numel() != n * comps * 64:
        raise _lib.RefidHipError(f"jpeg_decode: quant must be a contiguous 16-bit tensor of {n}*{comps}*64 elements on {coefs.device}")
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=coefs.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != coefs.device or tuple(out.shape) != (n, h, w, 3) or \
            not out.is_contiguous():
        raise _lib.RefidHipError(f"jpeg_decode: out must be a contiguous uint8 ({n}, {h}, {w}, 3) tensor on {coefs.device}")
    L = lib()
    work_bytes = L.refid_jpeg_decode_work_bytes(n, h, w, JPEG_DECODE_SAMPLINGS[sampling])
    if not work_bytes:
        raise _lib.RefidHipError(f"jpeg_decode: {n} frames of {h}x{w} exceed the grid (split the call)")
    work = torch.empty((work_bytes // 8,), dtype=torch.int64, device=coefs.device)
    desc = _lib.JpegDecodeDesc(coefs=coefs.data_ptr(), quant=quant.data_ptr(), frames=out.data_ptr(), work=work.data_ptr(), n_frames=n,
                               height=h, width=w, sampling=JPEG_DECODE_SAMPLINGS[sampling])
    check(L.refid_jpeg_decode(C.byref(desc), _stream()), "refid_jpeg_decode")
    return out


def score_u8(a_u8, b_u8, bgr=False, crop_border=0, sq_rgb=True, sq_y=False, ssim3d=True, ssim_y=False, taps=False):
    """refid_score_u8 (csrc/score.hip) on the current stream: two uint8 CUDA tensors (..., H, W, 3) of one shape -> an int64
    CUDA tensor (4, nf) of 8-byte words, row 0 the integer squared errors, rows 1..3 the bits of the float64 sums sq_y,
    ssim3d, ssim_y in the layout of include/refid_hip.h (``.view(torch.float64)``); a row that was not asked for is not
    written.  Both frames are cropped by ``crop_border`` first.  ``taps=True`` also returns [Y of ``a_u8`` float32
    (nf, hc, wc), the Y SSIM map float64 (nf, hc, wc) or None without ``ssim_y``].  Does not synchronise."""
    for t in (a_u8, b_u8):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.uint8 or t.dim() < 3 or t.shape[-1] != 3 or t.numel() == 0:
            raise _lib.RefidHipError("score_u8: non-empty uint8 CUDA tensors (..., H, W, 3) are required (no CPU fallback)")
    if a_u8.shape != b_u8.shape or a_u8.device != b_u8.device:
        raise _lib.RefidHipError(f"score_u8: the frames differ: {tuple(a_u8.shape)} on {a_u8.device}, {tuple(b_u8.shape)} on "
                                 f"{b_u8.device}")
    a_u8, b_u8 = a_u8.contiguous(), b_u8.contiguous()
    h, w, cb = int(a_u8.shape[-3]), int(a_u8.shape[-2]), int(crop_border)
    nf = a_u8.numel() // (3 * h * w)
    hc, wc = h - 2 * cb, w - 2 * cb
    if cb < 0 or hc < 1 or wc < 1:
        raise _lib.RefidHipError(f"score_u8: crop_border {cb} leaves nothing of a {h}x{w} frame")
    words = lib().refid_score_u8_parts(nf, h, w, cb)
    if words <= 0:
        raise _lib.RefidHipError(f"score_u8: {nf} frames of {h}x{w} exceed a 31-bit offset or the grid (split the call)")
    buf = torch.empty(4 * nf + words, dtype=torch.int64, device=a_u8.device)
    out = buf[:4 * nf].view(4, nf)
    ya = torch.empty((nf, hc, wc), dtype=torch.float32, device=a_u8.device) if taps else None
    ymap = torch.empty((nf, hc, wc), dtype=torch.float64, device=a_u8.device) if taps and ssim_y else None
    ptr = lambda t, on=True: t.data_ptr() if (t is not None and on) else None      # noqa: E731
    check(lib().refid_score_u8(a_u8.data_ptr(), b_u8.data_ptr(), nf, h, w, _lib.SCORE_BGR if bgr else 0, cb,
                               ptr(out[0], sq_rgb), ptr(out[1], sq_y), ptr(out[2], ssim3d), ptr(out[3], ssim_y),
                               buf[4 * nf:].data_ptr(), ptr(ya), ptr(ymap), _stream()), "refid_score_u8")
    return (out, [ya, ymap]) if taps else out


def _event_sim_threshold(name, c, h, w, device):
    """(scalar, map tensor or None) of one threshold argument of ``event_sim``."""
    if torch.is_tensor(c):
        if not c.is_cuda or c.device != device or c.dtype != torch.int32 or tuple(c.shape) != (h, w) or not c.is_contiguous():
            raise _lib.RefidHipError(f"event_sim: a {name} map must be a contiguous int32 ({h}, {w}) tensor on {device}, got {c.dtype} "
                                     f"{tuple(c.shape)} on {c.device}")
        return 0, c
    if isinstance(c, bool) or not isinstance(c, (int, np.integer)):
        raise _lib.RefidHipError(f"event_sim: {name} must be an int in units of 2^-16 or an int32 ({h}, {w}) map, got {type(c).__name__}")
    if not 1 <= int(c) < 2 ** 31:
        raise _lib.RefidHipError(f"event_sim: {name} {int(c)} must be 1 .. 2^31 - 1 (units of 2^-16)")
    return int(c), None


def event_sim_reset(frame_u8, lut, state=None, bgr=False):
    """RESET of refid_event_sim on the current stream: ``state`` int32 (H, W) = lut[Y8(frame)] for a uint8 (H, W, 3) CUDA
    frame.  Does not synchronise."""
    if not torch.is_tensor(frame_u8) or not frame_u8.is_cuda or frame_u8.dtype != torch.uint8 or frame_u8.dim() != 3 or \
            frame_u8.shape[2] != 3 or not frame_u8.is_contiguous() or frame_u8.numel() == 0:
        raise _lib.RefidHipError("event_sim_reset: the frame must be a contiguous non-empty uint8 (H, W, 3) CUDA tensor (no CPU fallback), got "
                                 + (f"{frame_u8.dtype} {tuple(frame_u8.shape)} on {frame_u8.device}" if torch.is_tensor(frame_u8)
                                    else type(frame_u8).__name__))
    h, w = int(frame_u8.shape[0]), int(frame_u8.shape[1])
    dev = frame_u8.device
    if not torch.is_tensor(lut) or lut.device != dev or lut.dtype != torch.int32 or tuple(lut.shape) != (256,) or not lut.is_contiguous():
        raise _lib.RefidHipError(f"event_sim_reset: lut must be a contiguous int32 (256,) tensor on {dev}")
    if state is None:
        state = torch.empty((h, w), dtype=torch.int32, device=dev)
    elif not torch.is_tensor(state) or state.device != dev or state.dtype != torch.int32 or tuple(state.shape) != (h, w) or \
            not state.is_contiguous():
        raise _lib.RefidHipError(f"event_sim_reset: state must be a contiguous int32 ({h}, {w}) tensor on {dev}")
    desc = _lib.EventSimDesc(frames=frame_u8.data_ptr(), lut=lut.data_ptr(), state=state.data_ptr(), n_frames=1, height=h, width=w,
                             bgr=int(bool(bgr)), stage=_lib.EVENT_SIM_RESET)
    check(lib().refid_event_sim(C.byref(desc), _stream()), "refid_event_sim (reset)")
    return state


def event_sim(frames_u8, stamps, state, lut, c_pos, c_neg, bgr=False, lut_range=None, c_min=None):
    """refid_event_sim (csrc/event_sim.hip) on the current stream: the events of the N - 1 intervals of ``frames_u8`` uint8
    (N, H, W, 3) on the device (a contiguous view of any alignment), by the ESIM model of include/refid_hip.h ->
    ``(rows, offsets)``: ``rows`` float32 (E, 4) [t, x, y, p] on the device, ascending in (interval, tick, pixel, j) and so
    non-decreasing in t; ``offsets`` int64 (N,) on the host, interval k's rows being [offsets[k], offsets[k+1]).  An event
    exactly at stamps[k+1] (tick 2^20) lies in interval k's rows but, under ``sequence.pair_windows``' half-open rule,
    in the time window that begins at stamps[k+1].

    ``stamps``: N strictly increasing float64 on the host.  ``state`` int32 (H, W) on the device, the pixels' reference
    levels: read, and written with the levels after the last frame (``event_sim_reset`` makes the first one).  ``lut``
    int32 (256,) on the device.  ``c_pos`` / ``c_neg``: an int in units of 2^-16, or an int32 (H, W) map on the device.
    ``lut_range`` = (min, max) of the table and ``c_min`` = the smallest value of the maps, when the caller knows them
    (``event_sim.EventSimulator`` reduces once at construction); None: reduced here, one more synchronisation each.

    Launches: count, ``torch.cumsum`` over the pixels, ONE synchronisation that reads the per-interval totals, the overflow
    flag and E, emit, ``torch.sort`` of the unique 64-bit keys, gather.  E = 0 returns an empty (0, 4) tensor after the
    synchronisation, without an emit launch.  A pixel with more than 255 events in an interval (only maps or tables that
    belie ``c_min`` / ``lut_range`` get that far) raises RefidHipError and leaves ``state`` as it was; so does E >= 2^31."""
    if not torch.is_tensor(frames_u8) or not frames_u8.is_cuda or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or \
            frames_u8.shape[3] != 3 or not frames_u8.is_contiguous():
        raise _lib.RefidHipError("event_sim: frames must be a contiguous uint8 (N, H, W, 3) CUDA tensor (no CPU fallback), got "
                                 + (f"{frames_u8.dtype} {tuple(frames_u8.shape)} on {frames_u8.device}" if torch.is_tensor(frames_u8)
                                    else type(frames_u8).__name__))
    n, h, w = (int(v) for v in frames_u8.shape[:3])
    dev = frames_u8.device
    if n < 2:
        raise _lib.RefidHipError(f"event_sim: frames holds N={n} frames, at least 2 are needed")
    if n > _lib.EVENT_SIM_MAX_FRAMES:
        raise _lib.RefidHipError(f"event_sim: N={n} frames exceed {_lib.EVENT_SIM_MAX_FRAMES} in one call: use a smaller chunk")
    if h < 1 or w < 1 or h * w > _lib.EVENT_SIM_MAX_PIXELS:
        raise _lib.RefidHipError(f"event_sim: height {h} * width {w} must be 1 .. {_lib.EVENT_SIM_MAX_PIXELS} pixels (what the sort key holds)")
    stamps_host = np.ascontiguousarray(np.asarray(stamps.cpu() if torch.is_tensor(stamps) else stamps, dtype=np.float64).reshape(-1))
    if stamps_host.shape != (n,):
        raise _lib.RefidHipError(f"event_sim: {stamps_host.size} stamps for N={n} frames")
    if not np.all(np.isfinite(stamps_host)) or not np.all(stamps_host[1:] > stamps_host[:-1]):
        raise _lib.RefidHipError("event_sim: stamps must be finite and strictly increasing")
    if not torch.is_tensor(state) or state.device != dev or state.dtype != torch.int32 or tuple(state.shape) != (h, w) or not state.is_contiguous():
        raise _lib.RefidHipError(f"event_sim: state must be a contiguous int32 ({h}, {w}) tensor on {dev}")
    if not torch.is_tensor(lut) or lut.device != dev or lut.dtype != torch.int32 or tuple(lut.shape) != (256,) or not lut.is_contiguous():
        raise _lib.RefidHipError(f"event_sim: lut must be a contiguous int32 (256,) tensor on {dev}")
    cp, cp_map = _event_sim_threshold("c_pos", c_pos, h, w, dev)
    cn, cn_map = _event_sim_threshold("c_neg", c_neg, h, w, dev)
    if lut_range is None:
        host = lut.cpu()
        lut_range = (int(host.min()), int(host.max()))
    maps = [m for m in (cp_map, cn_map) if m is not None]
    if maps and c_min is None:
        c_min = min(int(m.min()) for m in maps)
    c_min = int(c_min) if maps else 0
    L = lib()
    stamps_dev = torch.from_numpy(stamps_host).to(dev)
    counts = torch.empty((h * w,), dtype=torch.int32, device=dev)
    totals = torch.zeros((n + 1,), dtype=torch.int64, device=dev)          # rows per interval, the flag word, then E
    ptr = lambda t: t.data_ptr() if t is not None else None               # noqa: E731
    desc = _lib.EventSimDesc(frames=frames_u8.data_ptr(), stamps_host=stamps_host.ctypes.data, stamps_dev=stamps_dev.data_ptr(),
                             lut=lut.data_ptr(), c_pos_map=ptr(cp_map), c_neg_map=ptr(cn_map), state=state.data_ptr(),
                             counts=counts.data_ptr(), totals=totals.data_ptr(), n_frames=n, height=h, width=w, bgr=int(bool(bgr)),
                             c_pos=cp, c_neg=cn, c_min=c_min, lut_min=lut_range[0], lut_max=lut_range[1], stage=_lib.EVENT_SIM_COUNT)
    check(L.refid_event_sim(C.byref(desc), _stream()), "refid_event_sim (count)")
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    totals[n:].copy_(ends[-1:])
    host = totals.cpu()                                                     # the call's one synchronisation
    per_interval, flag, total = host[:n - 1].numpy(), int(host[n - 1]), int(host[n])
    offsets = np.zeros((n,), dtype=np.int64)
    np.cumsum(per_interval, out=offsets[1:])
    if flag & _lib.EVENT_SIM_FLAG_OVERFLOW:
        raise _lib.RefidHipError(f"event_sim: overflow: a pixel has more than {_lib.EVENT_SIM_CAP} events in one interval (a threshold or a "
                                 f"table entry lies outside what c_min / lut_range state); state is unchanged")
    if total != int(offsets[-1]):
        raise _lib.RefidHipError(f"event_sim: the per-pixel rows sum to {total}, the per-interval rows to {int(offsets[-1])}")
    if total >= 2 ** 31:
        raise _lib.RefidHipError(f"event_sim: E={total} rows in one call reach 2^31: use a smaller chunk")
    if total == 0:
        return torch.empty((0, 4), dtype=torch.float32, device=dev), offsets
    rows = torch.empty((total, 4), dtype=torch.float32, device=dev)
    keys = torch.empty((total,), dtype=torch.int64, device=dev)
    desc.ends, desc.rows, desc.keys, desc.n_rows, desc.stage = ends.data_ptr(), rows.data_ptr(), keys.data_ptr(), total, _lib.EVENT_SIM_EMIT
    check(L.refid_event_sim(C.byref(desc), _stream()), "refid_event_sim (emit)")
    perm = torch.sort(keys)[1]
    out = torch.empty_like(rows)
    desc.perm, desc.sorted, desc.stage = perm.data_ptr(), out.data_ptr(), _lib.EVENT_SIM_GATHER
    check(L.refid_event_sim(C.byref(desc), _stream()), "refid_event_sim (gather)")
    return out, offsets


def blur_synth(frames_u8, windows, to_linear=None, out=None, max_groups=0):
    """refid_blur_synth (csrc/blur_synth.hip) on the current stream: uint8 CUDA frames (N, H, W, 3), a contiguous view of any
    alignment, and ``windows`` int32 (K, 2) rows [first, count] on the host (1 <= count <= 64, first + count <= N; they may
    overlap or repeat) -> uint8 (K, H, W, 3): window k's frames averaged byte by byte, by the integer formulas of
    include/refid_hip.h ("Blur synthesis").  ``to_linear``: None (plain mode: the codes are averaged) or uint32 (256,) on the
    host, strictly increasing, at most 2^24 (response mode: the levels are averaged and the nearest code is looked up;
    ``blur_synth.gamma_table``).  ``out``: a contiguous uint8 tensor of K*H*W*3 elements to write into (any alignment;
    nothing outside it is written); the result is a view of it.  ``max_groups``: the cap of the grid in workgroups (0: the
    launcher's own).  One launch; does not synchronise."""
    f = frames_u8
    if not isinstance(f, torch.Tensor) or not f.is_cuda or f.dtype != torch.uint8 or f.dim() != 4 or f.shape[-1] != 3 or \
            f.numel() == 0 or not f.is_contiguous():
        raise _lib.RefidHipError("blur_synth: frames must be a non-empty contiguous uint8 (N, H, W, 3) CUDA tensor (no CPU fallback), got "
                                 + (f"{f.dtype} {tuple(f.shape)} on {f.device}" if isinstance(f, torch.Tensor) else type(f).__name__))
    n, h, w = (int(v) for v in f.shape[:3])
    try:
        win = np.asarray(windows.cpu() if torch.is_tensor(windows) else windows)
    except (TypeError, ValueError):
        win = np.zeros((0,), dtype=np.float64)
    if win.ndim != 2 or win.shape[1] != 2 or win.shape[0] < 1 or win.dtype.kind not in "iu":
        raise _lib.RefidHipError(f"blur_synth: windows must be integer (K, 2) rows [first, count] with K >= 1, got {win.dtype} {tuple(win.shape)}")
    if int(win.min()) < -2 ** 31 or int(win.max()) >= 2 ** 31:
        raise _lib.RefidHipError("blur_synth: windows do not fit int32")
    win = np.ascontiguousarray(win, dtype=np.int32)
    k = int(win.shape[0])
    lin = None
    if to_linear is not None:
        lin = np.asarray(to_linear.cpu() if torch.is_tensor(to_linear) else to_linear)
        if lin.shape != (256,) or lin.dtype.kind not in "iu" or int(lin.min()) < 0 or int(lin.max()) >= 2 ** 32:
            raise _lib.RefidHipError(f"blur_synth: to_linear must be 256 unsigned integers on the host, got {lin.dtype} {tuple(lin.shape)}")
        lin = np.ascontiguousarray(lin, dtype=np.uint32)
    if isinstance(max_groups, bool) or not isinstance(max_groups, (int, np.integer)) or not 0 <= int(max_groups) < 2 ** 31:
        raise _lib.RefidHipError(f"blur_synth: max_groups {max_groups!r} must be an int, 0 (the launcher's cap) .. 2^31 - 1")
    if out is None:
        out = torch.empty((k, h, w, 3), dtype=torch.uint8, device=f.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != f.device or out.numel() != k * h * w * 3 or \
            not out.is_contiguous():
        raise _lib.RefidHipError(f"blur_synth: out must be a contiguous uint8 tensor of {k}*{h}*{w}*3 elements on {f.device}")
    win_dev = torch.from_numpy(win).to(f.device)
    lin_dev = None if lin is None else torch.from_numpy(lin.view(np.int32)).to(f.device)     # (the bits of the uint32)
    desc = _lib.BlurSynthDesc(frames=f.data_ptr(), windows_host=win.ctypes.data, windows=win_dev.data_ptr(),
                              to_linear_host=None if lin is None else lin.ctypes.data,
                              to_linear=None if lin is None else lin_dev.data_ptr(), out=out.data_ptr(),
                              n_frames=n, height=h, width=w, n_windows=k, max_groups=int(max_groups))
    check(lib().refid_blur_synth(C.byref(desc), _stream()), "refid_blur_synth")
    return out.view(k, h, w, 3)


def edi(frames_u8, stream, items, bounds, instants, m=1, exposure="samples", c_pos=13107, c_neg=13107, eps=1e-3, out=None):
    """refid_edi (csrc/edi.hip) on the current stream: the event-based double integral of include/refid_hip.h ("Double
    integral").  ``frames_u8``: uint8 CUDA key frames (N, H, W, 3), a contiguous view of any alignment.  ``stream``: the
    sequence's events packed by pixel (``edi.EdiStream``, same device, same (H, W)).  On the host: ``items`` int (P, 2) rows
    [left, right] (right < 0: no right key), ``bounds`` (P, 4) rows [s0, e0, s1, e1], ``instants`` (P, T) ascending output
    instants.  ``exposure``: 'samples' (a key frame is the mean of ``m`` frames at ``edi.sample_instants``) or 'continuous'
    (a real shutter; ``m`` is not read).  ``c_pos`` / ``c_neg``: thresholds in units of 2^-16 (``event_sim.to_fixed``).
    ``out``: a contiguous uint8 tensor of P*T*H*W*3 elements to write into (any alignment).  Returns ``(frames uint8
    (P, T, H, W, 3), clamped)``; ``clamped.sum()`` is the number of (item, pixel) pairs whose gain was held at exp(+-32).  One
    launch; does not synchronise."""
    from . import edi as E
    f = frames_u8
    if not isinstance(f, torch.Tensor) or not f.is_cuda or f.dtype != torch.uint8 or f.dim() != 4 or f.shape[-1] != 3 or \
            f.numel() == 0 or not f.is_contiguous():
        raise _lib.RefidHipError("edi: frames must be a non-empty contiguous uint8 (N, H, W, 3) CUDA tensor (no CPU fallback), got "
                                 + (f"{f.dtype} {tuple(f.shape)} on {f.device}" if isinstance(f, torch.Tensor) else type(f).__name__))
    n, h, w = (int(v) for v in f.shape[:3])
    if not isinstance(stream, E.EdiStream) or stream.t is None:
        raise _lib.RefidHipError(f"edi: stream must be a loaded edi.EdiStream, got {type(stream).__name__}")
    if (stream.height, stream.width) != (h, w) or stream.t.device != f.device:
        raise _lib.RefidHipError(f"edi: stream is {stream.height}x{stream.width} on {stream.t.device}, frames are {h}x{w} on {f.device}")
    if exposure not in E.EXPOSURES:
        raise _lib.RefidHipError(f"edi: unknown exposure {exposure!r} ('samples' or 'continuous')")
    sampled = exposure == "samples"
    m = int(m)
    if sampled and not 1 <= m <= _lib.BLUR_MAX_COUNT:
        raise _lib.RefidHipError(f"edi: m {m} must be 1 .. {_lib.BLUR_MAX_COUNT}")
    for name, c in (("c_pos", c_pos), ("c_neg", c_neg)):
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 1 <= int(c) <= _lib.EDI_MAX_THRESHOLD:
            raise _lib.RefidHipError(f"edi: {name} {c!r} must be an int 1 .. {_lib.EDI_MAX_THRESHOLD} in units of 2^-16 (event_sim.to_fixed)")
    eps = float(eps)
    if not (np.isfinite(eps) and eps >= 0.0):
        raise _lib.RefidHipError(f"edi: eps {eps} must be finite and not negative")
    try:
        it = np.asarray(items)
        bd = np.asarray(bounds, dtype=np.float32)
        tau = np.asarray(instants, dtype=np.float32)
    except (TypeError, ValueError):
        raise _lib.RefidHipError("edi: items, bounds and instants must be arrays on the host") from None
    if it.ndim != 2 or it.shape[1] != 2 or it.dtype.kind not in "iu" or not 1 <= it.shape[0] <= _lib.EDI_MAX_ITEMS:
        raise _lib.RefidHipError(f"edi: items must be integer (P, 2) rows [left, right] with P = 1 .. {_lib.EDI_MAX_ITEMS}, got {it.dtype} "
                                 f"{tuple(it.shape)}")
    p = int(it.shape[0])
    if bd.shape != (p, 4):
        raise _lib.RefidHipError(f"edi: bounds must be ({p}, 4) rows [s0, e0, s1, e1], got {tuple(bd.shape)}")
    if tau.ndim != 2 or tau.shape[0] != p or not 1 <= tau.shape[1] <= _lib.EDI_MAX_INSTANTS:
        raise _lib.RefidHipError(f"edi: instants must be ({p}, T) with T = 1 .. {_lib.EDI_MAX_INSTANTS}, got {tuple(tau.shape)}")
    t = int(tau.shape[1])
    it = np.ascontiguousarray(np.clip(it, -1, 2 ** 31 - 1), dtype=np.int32)
    bd, tau = np.ascontiguousarray(bd), np.ascontiguousarray(tau)
    smp = None
    if sampled:
        smp = np.ascontiguousarray(np.stack([np.concatenate([E.sample_instants(b[0], b[1], m), E.sample_instants(b[2], b[3], m)])
                                             for b in bd]), dtype=np.float32)
    if out is None:
        out = torch.empty((p, t, h, w, 3), dtype=torch.uint8, device=f.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != f.device or out.numel() != p * t * h * w * 3 or \
            not out.is_contiguous():
        raise _lib.RefidHipError(f"edi: out must be a contiguous uint8 tensor of {p}*{t}*{h}*{w}*3 elements on {f.device}")
    groups = (h * w + _lib.EDI_THREADS - 1) // _lib.EDI_THREADS
    clamped = torch.empty((p * groups,), dtype=torch.int32, device=f.device)
    host = np.concatenate([v.view(np.int32).reshape(-1) for v in (it, bd, tau) + (() if smp is None else (smp,))])
    # one upload of the rows' bits, items | bounds | instants | samples, from pinned memory: it does not wait for the stream
    dev = torch.from_numpy(host).pin_memory().to(f.device, non_blocking=True)
    at = [0, 2 * p, 6 * p, 6 * p + p * t]
    ptr = lambda k: dev.data_ptr() + 4 * at[k]                # noqa: E731
    desc = _lib.EdiDesc(frames=f.data_ptr(), ev_t=stream.t.data_ptr() if stream.n_events else None,
                        ev_p=stream.p.data_ptr() if stream.n_events else None, seg=stream.seg.data_ptr(),
                        items_host=it.ctypes.data, items=ptr(0), bounds_host=bd.ctypes.data, bounds=ptr(1),
                        samples_host=None if smp is None else smp.ctypes.data, samples=None if smp is None else ptr(3),
                        instants_host=tau.ctypes.data, instants=ptr(2), tables=E.device_tables(f.device).data_ptr(),
                        out=out.data_ptr(), clamped=clamped.data_ptr(), eps255=255.0 * eps, n_events=stream.n_events,
                        n_frames=n, height=h, width=w, n_items=p, n_instants=t, m=m if sampled else 1,
                        exposure=_lib.EDI_SAMPLES if sampled else _lib.EDI_CONTINUOUS, c_pos=int(c_pos), c_neg=int(c_neg))
    check(lib().refid_edi(C.byref(desc), _stream()), "refid_edi")
    return out.view(p, t, h, w, 3), clamped
