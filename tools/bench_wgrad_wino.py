#!/usr/bin/env python3
"""fp32 Winograd weight gradient at the config-2 shapes, 8 grouped time steps per launch as in the train step: the F(2x2,3x3)
tile (algo 1, "regs") against the 2x4-tile form (algo 5, "f24").  Not bit-equal: the largest relative difference is printed.

  python tools/bench_wgrad_wino.py pair     the 2x4-tile form's four-wave and pair workgroups (REFID_W24_PAIR=0 / 1) side by
                                            side, ALTERNATING in one process (ROUNDS rounds per layer; median and min..max
                                            of each form, so a difference can be held against the spread of the same form);
                                            the conv_down shapes (algo 7) included; results compared bit for bit.
  python tools/bench_wgrad_wino.py down     conv_down's weight gradient (algo 7, F(2,3) x F(2,4) tiles) at the three DOWN_SHAPES:
                                            ROUNDS timings per layer, median and min..max."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = [("L0 res 64->64 @256", 256, 64, 0, 64), ("L0 main.0 128->64 @256", 256, 64, 64, 64),
          ("L0 first 32->64 @256", 256, 32, 0, 64), ("L0 dec 64->32 @256", 256, 64, 0, 32),
          ("L1 res 128->128 @128", 128, 128, 0, 128), ("L1 main.0 256->128 @128", 128, 128, 128, 128),
          ("L2 res 256->256 @64", 64, 256, 0, 256), ("L2 main.0 512->256 @64", 64, 256, 256, 256),
          ("bottleneck 256->256 @32", 32, 256, 0, 256)]


def run(tag, algo):
    import torch
    from refid_amd import ops
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from bench_kernels import timeit, B
    G = int(os.environ.get("GROUPS", 8))
    out = {}
    only = os.environ.get("ONLY_SHAPE")
    for name, H, Ca, Cb, Co in (SHAPES if only is None else [SHAPES[int(only)]]):
        torch.manual_seed(1)
        Ci = Ca + Cb
        steps = []
        for t in range(G):
            a = torch.randn(B, H, H, Ca, device="cuda")
            b = torch.randn(B, H, H, Cb, device="cuda") if Cb else None
            g = torch.randn(B, H, H, Co, device="cuda") * 0.01
            steps.append((g, a, b))
        dw = torch.zeros(Co, Ci, 3, 3, device="cuda"); db = torch.zeros(Co, device="cuda")
        g0, a0, b0 = steps[0]

        def go():
            return ops.conv2d_wgrad(g0, a0, dw, kh=3, kw=3, pad=1, in_b=b0, db=db, algo=algo, phase=1, more=steps[1:])
        go()
        if "REPS" in os.environ:                               # counter passes (tools/probes/w4_pmc.sh): a few launches, no timing loop
            for _ in range(int(os.environ["REPS"])):
                go()
            torch.cuda.synchronize()
            continue
        t = timeit(go)
        dw.zero_(); db.zero_()
        slabs = go()
        ops.conv2d_wgrad(g0, a0, dw, kh=3, kw=3, pad=1, in_b=b0, db=db, algo=algo, phase=3, slabs=slabs)
        fl = 2.0 * G * B * H * H * Co * Ci * ({5: 24 / 8, 6: 36 / 16}.get(algo, 16 / 4))
        print(f"{tag} {name:26s} {t*1e6:8.1f} us  {fl/t/1e12:6.1f} TF/s issued", flush=True)
        out[name] = (dw.cpu(), db.cpu())
    torch.save(out, f"/tmp/wgrad_wino_{tag}.pt")


DOWN_SHAPES = [("down 64->64 @256", 256, 64, 64), ("down 128->128 @128", 128, 128, 128), ("down 256->256 @64", 64, 256, 256)]


def run_pair():
    import statistics
    import torch
    from refid_amd import ops
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from bench_kernels import timeit, B
    G, rounds = int(os.environ.get("GROUPS", 8)), int(os.environ.get("ROUNDS", 5))
    cases = [(n, H, Ca, Cb, Co, False) for n, H, Ca, Cb, Co in SHAPES] + [(n, H, Ca, 0, Co, True) for n, H, Ca, Co in DOWN_SHAPES]
    only = os.environ.get("ONLY_SHAPE")
    print(f"# B={B} grouped steps={G} rounds={rounds}: us per launch, median (min..max); 4w = four-wave form, pair = pair form")
    for name, H, Ca, Cb, Co, down in (cases if only is None else [cases[int(only)]]):
        torch.manual_seed(1)
        Ci, k, Ho = Ca + Cb, (4 if down else 3), (H // 2 if down else H)
        steps = []
        for t in range(G):
            a = torch.randn(B, H, H, Ca, device="cuda")
            b = torch.randn(B, H, H, Cb, device="cuda") if Cb else None
            g = torch.randn(B, Ho, Ho, Co, device="cuda") * 0.01
            steps.append((g, a, b))
        g0, a0, b0 = steps[0]
        geo = dict(kh=4, kw=4, stride=2, pad=1, algo=7) if down else dict(kh=3, kw=3, pad=1, algo=5)
        times, grads = {"0": [], "1": []}, {}
        for r in range(rounds):
            for mode in ("0", "1"):
                os.environ["REFID_W24_PAIR"] = mode
                dw = torch.zeros(Co, Ci, k, k, device="cuda"); db = torch.zeros(Co, device="cuda")

                def go():
                    return ops.conv2d_wgrad(g0, a0, dw, in_b=b0, db=db, phase=1, more=steps[1:], **geo)
                times[mode].append(timeit(go) * 1e6)
                if r == 0:
                    ops.conv2d_wgrad(g0, a0, dw, in_b=b0, db=db, phase=3, slabs=go(), **geo)
                    grads[mode] = (dw.clone(), db.clone())
        same = torch.equal(grads["0"][0], grads["1"][0]) and torch.equal(grads["0"][1], grads["1"][1])
        m0, m1 = statistics.median(times["0"]), statistics.median(times["1"])
        print(f"{name:26s} 4w {m0:8.1f} ({min(times['0']):8.1f}..{max(times['0']):8.1f})  pair {m1:8.1f} "
              f"({min(times['1']):8.1f}..{max(times['1']):8.1f})  pair/4w {m1 / m0:5.3f}  bits {'equal' if same else 'DIFFER'}",
              flush=True)


def run_down():
    import statistics
    import torch
    from refid_amd import ops
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from bench_kernels import timeit, B
    G, rounds = int(os.environ.get("GROUPS", 8)), int(os.environ.get("ROUNDS", 5))
    only = os.environ.get("ONLY_SHAPE")
    print(f"# B={B} grouped steps={G} rounds={rounds}: us per launch, median (min..max)")
    for name, H, Ca, Co in (DOWN_SHAPES if only is None else [DOWN_SHAPES[int(only)]]):
        torch.manual_seed(1)
        steps = [(torch.randn(B, H // 2, H // 2, Co, device="cuda") * 0.01, torch.randn(B, H, H, Ca, device="cuda"), None)
                 for t in range(G)]
        g0, a0, b0 = steps[0]
        geo = dict(kh=4, kw=4, stride=2, pad=1, algo=7)
        dw = torch.zeros(Co, Ca, 4, 4, device="cuda"); db = torch.zeros(Co, device="cuda")

        def go():
            return ops.conv2d_wgrad(g0, a0, dw, in_b=b0, db=db, phase=1, more=steps[1:], **geo)
        times = [timeit(go) * 1e6 for r in range(rounds)]
        print(f"{name:26s} {statistics.median(times):8.1f} ({min(times):8.1f}..{max(times):8.1f})", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "pair":
        run_pair()
    elif len(sys.argv) > 1 and sys.argv[1] == "down":
        run_down()
    elif len(sys.argv) > 1:
        run(sys.argv[1], {"regs": 1, "f24": 5}[sys.argv[1]])
    else:
        other = "f24"
        for tag in ("regs", other):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), tag])
        import torch
        a, b = torch.load("/tmp/wgrad_wino_regs.pt"), torch.load(f"/tmp/wgrad_wino_{other}.pt")
        for k in a:
            dwd = ((a[k][0] - b[k][0]).abs().max() / a[k][0].abs().max()).item()
            dbd = ((a[k][1] - b[k][1]).abs().max() / a[k][1].abs().max()).item()
            print(f"{k:26s} rel diff dw {dwd:.1e} db {dbd:.1e}")
