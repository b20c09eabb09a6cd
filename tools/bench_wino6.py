#!/usr/bin/env python3
"""fp32 Winograd tile (algo 1) vs Winograd x six bf16 products (algo 5) vs Winograd x three fp16 products (algo 5, terms 3) vs
Winograd x ONE fp16 product (algo 5, terms 1: compute_dtype 'fp16') vs the bf16 one-product direct tile (algo 4, terms 1:
compute_dtype 'bf16'; single-source layers only, as in the engine) at the config-2 shapes (B=8): time and -- on a small crop --
the largest deviation of each from the float64 convolution.

  python tools/bench_wino6.py               the table above
  python tools/bench_wino6.py ab [B ...]    the routing before the in-group split-K (wino_tile 5: two launch rows + finishing pass)
                                            and the library's choice (wino_tile 0) on the three-fp16-product form, ALTERNATING in
                                            one process: ROUNDS (5) timings per layer and form, median and min..max, results
                                            compared bit for bit.  Layers: the 32-channel shapes and the bottleneck conv, whose plan
                                            has two K ranges at B=8; at the batch sizes given (default 8 1 2) every split layer."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from refid_amd import ops
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_kernels import timeit, B


def one(name, H, Ca, Cb, Co, res=False, mask=False):
    Ci = Ca + Cb
    a = torch.randn(B, H, H, Ca, device="cuda")
    b = torch.randn(B, H, H, Cb, device="cuda") if Cb else None
    w = torch.randn(Co, Ci, 3, 3, device="cuda") * (1.0 / (Ci * 9) ** 0.5)
    bias = torch.randn(Co, device="cuda")
    r = torch.randn(B, H, H, Co, device="cuda") if res else None
    m = torch.randn(B, H, H, Co, device="cuda") if mask else None
    fl = 2.0 * B * H * H * Co * Ci * 9
    kw = dict(kh=3, kw=3, pad=1, cout=Co, cout_pad=-(-Co // 64) * 64, in_b=b, bias=bias, slope_pre=0.1, res=r, mask=m,
              slope_mask=0.2 if mask else 1.0)
    w1 = ops.pack_conv_weights(w, ops.ROLE_WINO_FWD, 64, 8, 3, 3, Co, Ci)
    w6 = ops.pack_conv_weights_wino6(w, ops.ROLE_WINO_FWD, Co, Ci)
    w3 = ops.pack_conv_weights_wino6(w, ops.ROLE_WINO_FWD, Co, Ci, f16=True)
    o1 = torch.empty(B, H, H, Co, device="cuda")
    o6 = torch.empty(B, H, H, Co, device="cuda")
    o3 = torch.empty(B, H, H, Co, device="cuda")
    wh = ops.pack_conv_weights_wino6(w, ops.ROLE_WINO_FWD, Co, Ci, terms=1)
    oh = torch.empty(B, H, H, Co, device="cuda")
    ob = tb = None
    if b is None:                                           # (one bf16 product: the engine sends single-source convs only)
        bn = ops.conv_bn(3, 3, 1, 0, Co)
        wb = ops.pack_conv_weights_split(w, ops.ROLE_FWD, bn, 3, 3, Co, Ci, planes=1)
        ob = torch.empty(B, H, H, Co, device="cuda")
        tb = timeit(lambda: ops.conv2d(a, wb, ob, algo=4, terms=1, **dict(kw, cout_pad=-(-Co // bn) * bn)))
    t1 = timeit(lambda: ops.conv2d(a, w1, o1, algo=1, **kw))
    t6 = timeit(lambda: ops.conv2d(a, w6, o6, algo=5, **kw))
    t3 = timeit(lambda: ops.conv2d(a, w3, o3, algo=5, terms=3, **kw))
    th = timeit(lambda: ops.conv2d(a, wh, oh, algo=5, terms=1, **kw))
    # float64 reference on a crop of sample 0 (rows 0..15: includes the top border)
    crop = 18
    xa = torch.cat([a[:1, :crop], b[:1, :crop]], 3) if b is not None else a[:1, :crop]
    ref = F.conv2d(xa.permute(0, 3, 1, 2).double().cpu(), w.double().cpu(), bias.double().cpu(), 1, 1)
    ref = torch.where(ref > 0, ref, 0.1 * ref)[:, :, :crop - 2].permute(0, 2, 3, 1)
    if res:
        ref = ref + r[:1, :crop - 2].double().cpu()
    if mask:
        ref = ref * torch.where(m[:1, :crop - 2].cpu() > 0, 1.0, 0.2)
    e1, e6, e3, eh = ((o[:1, :crop - 2].double().cpu() - ref).abs().max().item() for o in (o1, o6, o3, oh))
    direct = "bf16 direct       -                -" if ob is None else \
        f"bf16 direct {tb*1e6:7.1f} us  err {(ob[:1, :crop - 2].double().cpu() - ref).abs().max().item():.1e}"
    print(f"{name:28s} wino fp32 {t1*1e6:7.1f} us | x6 bf16 {t6*1e6:7.1f} us | x3 fp16 {t3*1e6:7.1f} us {fl/t3/1e12:6.1f} TF(eff) "
          f"x{t6/t3:4.2f} vs x6 | x1 fp16 {th*1e6:7.1f} us x{t3/th:4.2f} vs x3 | {direct} | err vs fp64: fp32 {e1:.1e}  x6 {e6:.1e}  "
          f"x3 {e3:.1e}  x1 {eh:.1e}", flush=True)


AB_SHAPES = [   # name, H, Ca, Cb, Co, res + mask
    ("D2 res 32->32 @256", 256, 32, 0, 32, False), ("D2 res dgrad 32->32 +res+mask", 256, 32, 0, 32, True),
    ("L0 first dgrad 64->32 @256", 256, 64, 0, 32, False), ("D2 main.0 64->32 +res+mask", 256, 32, 32, 32, True),
    ("bottleneck 256->256 @32", 32, 256, 0, 256, False), ("bottleneck dgrad +res+mask", 32, 256, 0, 256, True),
    ("L2 res 256->256 @64", 64, 256, 0, 256, False), ("L2 main.0 512->256 @64", 64, 256, 256, 256, False),
    ("L1 res 128->128 @128", 128, 128, 0, 128, False),
]


def run_ab(batches):
    import statistics
    rounds = int(os.environ.get("ROUNDS", 5))
    print(f"# x3 fp16, rounds={rounds}: us per call, median (min..max); grid = wino_tile 5 (grid split + finishing pass), "
          f"group = wino_tile 0 (in-group split where the plan has two K ranges); ws = the grid form wrote the workspace")
    for nb in batches:
        for name, H, Ca, Cb, Co, rm in AB_SHAPES:
            torch.manual_seed(1)
            Ci = Ca + Cb
            a = torch.randn(nb, H, H, Ca, device="cuda")
            b = torch.randn(nb, H, H, Cb, device="cuda") if Cb else None
            w = torch.randn(Co, Ci, 3, 3, device="cuda") * (1.0 / (Ci * 9) ** 0.5)
            r = torch.randn(nb, H, H, Co, device="cuda") if rm else None
            m = torch.randn(nb, H, H, Co, device="cuda") if rm else None
            kw = dict(kh=3, kw=3, pad=1, cout=Co, cout_pad=-(-Co // 64) * 64, in_b=b, bias=torch.randn(Co, device="cuda"),
                      slope_pre=0.1, res=r, mask=m, slope_mask=0.2 if rm else 1.0, algo=5, terms=3)
            w3 = ops.pack_conv_weights_wino6(w, ops.ROLE_WINO_FWD, Co, Ci, f16=True)
            outs = {t: torch.empty(nb, H, H, Co, device="cuda") for t in (5, 0)}
            times = {5: [], 0: []}
            ws = ops._workspace(64 << 20, a.device, "conv")
            ws.fill_(-12345.0)
            for _ in range(rounds):
                for t in (5, 0):
                    ops.WINO_TILE = t
                    times[t].append(timeit(lambda: ops.conv2d(a, w3, outs[t], **kw), iters=20) * 1e6)
            split = not bool((ws == -12345.0).all())
            ops.WINO_TILE = 0
            m5, m0 = statistics.median(times[5]), statistics.median(times[0])
            print(f"B={nb} {name:30s} grid {m5:7.1f} ({min(times[5]):7.1f}..{max(times[5]):7.1f})  group {m0:7.1f} "
                  f"({min(times[0]):7.1f}..{max(times[0]):7.1f})  group/grid {m0 / m5:5.3f}  ws {'yes' if split else 'no '}  "
                  f"bits {'equal' if torch.equal(outs[5], outs[0]) else 'DIFFER'}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "ab":
        run_ab([int(v) for v in sys.argv[2:]] or [8, 1, 2])
        sys.exit(0)
    one("L0 first dgrad 64->32.. skip", 256, 64, 0, 64)
    one("L0 main.0 128->64 @256", 256, 64, 64, 64)
    one("L0 res 64->64 @256", 256, 64, 0, 64)
    one("L0 res 64->64 @256 +res", 256, 64, 0, 64, res=True)
    one("L0 res dgrad +res +mask", 256, 64, 0, 64, res=True, mask=True)
    one("L0 first 32->64 @256", 256, 32, 0, 64)
    one("L1 main.0 256->128 @128", 128, 128, 128, 128)
    one("L1 res 128->128 @128", 128, 128, 0, 128)
    one("L2 main.0 512->256 @64", 64, 256, 256, 256)
    one("L2 res 256->256 @64", 64, 256, 0, 256)
    one("L2 first 128->256 @64", 64, 128, 0, 256)
    one("bottleneck 256->256 @32", 32, 256, 0, 256)
    one("D1 main.0 128->64 @128", 128, 64, 64, 64)
    # 32 output channels: the tile's one-column-tile form (round 4)
    one("D2 main.0 64->32 @256", 256, 32, 32, 32)
    one("D2 res 32->32 @256", 256, 32, 0, 32)
    one("D2 res 32->32 @256 +res", 256, 32, 0, 32, res=True)
    one("D2 res dgrad +res +mask", 256, 32, 0, 32, res=True, mask=True)
    one("L0 first dgrad 64->32 @256", 256, 64, 0, 32)
    one("L0 first dgrad 64->32 +res +mask", 256, 64, 0, 32, res=True, mask=True)
