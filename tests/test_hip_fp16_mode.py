"""compute_dtype 'fp16': the bf16 compute mode with every 3x3 call that the fp32 mode runs on the Winograd fp16 tile moved to
that tile's ONE-product form (refid_conv2d algo 5, mfma_terms 1).  End-to-end parity on the bars of the bf16 mode
(test_hip_network.py::test_bf16_compute_path_psnr_parity, unchanged), the routing contract call by call, graph replay, and the
option's validation."""
import numpy as np
import pytest
import torch

from oracle import refid_oracle as O

MODES = ("fp32", "bf16x3", "bf16", "fp16")


def _net(img_chn, base, dtype, P=None):
    from refid_amd.archs import define_network
    net = define_network(dict(type="FinalBidirectionAttenfusion", img_chn=img_chn, ev_chn=2, num_encoders=3,
                              base_num_channels=base, num_block=1, num_residual_blocks=2, compute_dtype=dtype))
    if P is not None:
        net.load_state_dict(P, strict=True)
    return net


def test_compute_dtype_validation():
    """'fp16' is an option value next to the other three; anything else is still a ValueError that names the choices."""
    with pytest.raises(ValueError, match="fp16"):
        _net(6, 8, "fp8")
    for dt in MODES:
        assert _net(6, 8, dt).compute_dtype == dt


@pytest.mark.gpu
def test_engine_validates_compute_dtype():
    from refid_amd.engine import Engine
    with pytest.raises(ValueError, match="fp16"):
        Engine(6, 2, 3, 8, 2, device=torch.device("cuda"), compute_dtype="fp8")
    assert Engine(6, 2, 3, 8, 2, device=torch.device("cuda"), compute_dtype="fp16").compute_dtype == "fp16"


@pytest.mark.gpu
def test_fp16_compute_path_psnr_parity(golden_dir):
    """The bf16 mode's bars on full26_train: PSNR against the reference's fp32 output > 50 dB, PSNR against the ground truth
    moved by < 0.01 dB, loss within 2e-3, the large gradient norms within 5 %, exactly 13 gradient-less parameters."""
    from test_hip_network import load
    z, P, x, ev, gt, img_chn, base = load(golden_dir, "full26_train")
    ref = torch.from_numpy(z["out"])
    with torch.no_grad():
        pb = _net(img_chn, base, "bf16", P).cuda()(x=x.cuda(), event=ev.cuda())
    psnr_bf16 = O.psnr_between(pb.cpu(), ref)
    net = _net(img_chn, base, "fp16", P).cuda()
    pred = net(x=x.cuda(), event=ev.cuda())
    psnr = O.psnr_between(pred.detach().cpu(), ref)
    msg = f"PSNR against the fp32 golden output: fp16 mode {psnr:.2f} dB, bf16 mode {psnr_bf16:.2f} dB"
    print(msg)
    assert psnr > 50.0, msg
    p16 = O.psnr_between(pred.detach().cpu().clamp(0, 1), gt)
    p32 = O.psnr_between(ref.clamp(0, 1), gt)
    assert abs(p16 - p32) < 0.01, (p16, p32, msg)
    loss = torch.sqrt((pred - gt.cuda()) ** 2 + 1e-12).mean()
    loss.backward()
    np.testing.assert_allclose(loss.item(), float(z["loss"]), rtol=2e-3)
    gn = np.array([float(p.grad.norm()) for _, p in net.named_parameters()])
    ref_gn = z["grad_norms_all"]
    big = ref_gn > 1e-3 * ref_gn.max()
    np.testing.assert_allclose(gn[big], ref_gn[big], rtol=0.05)
    assert int((gn == 0).sum()) == 13


def _conv_calls(monkeypatch, dtype, P, x, ev, gt):
    """(kh, stride, mode, algo, terms) of every ops.conv2d call of one forward + backward."""
    from refid_amd import ops
    calls, real = [], ops.conv2d

    def conv2d(*a, **kw):
        calls.append((kw["kh"], kw.get("stride", 1), kw.get("mode", 0), kw.get("algo", 0), kw.get("terms", 0)))
        return real(*a, **kw)

    net = _net(26, 32, dtype, P).cuda()
    with monkeypatch.context() as m:
        m.setattr(ops, "conv2d", conv2d)
        pred = net(x=x.cuda(), event=ev.cuda())
        torch.sqrt((pred - gt.cuda()) ** 2 + 1e-12).mean().backward()
    torch.cuda.synchronize()
    return calls


@pytest.mark.gpu
def test_routing_contract(monkeypatch):
    """'fp16': the one-product Winograd form wherever the fp32 mode runs the Winograd fp16 tile -- call for call --, a bf16-mode
    route everywhere else, never the three- or six-product form; the other modes never see the new form."""
    P = O.make_params(26, base_num_channels=32, mode="hash", seed=5)
    x, ev, gt = O.make_inputs(1, 2, 32, 32, 26, seed=3, mode="hash")
    calls = {dt: _conv_calls(monkeypatch, dt, P, x, ev, gt) for dt in MODES}
    at = lambda dt: [c[3:] for c in calls[dt]]
    assert (5, 1) in at("fp16")
    assert (5, 3) not in at("fp16") and (5, 0) not in at("fp16") and (5, 6) not in at("fp16")
    assert (5, 1) not in at("fp32") and (5, 1) not in at("bf16") and (5, 1) not in at("bf16x3")
    is3x3 = lambda c: c[0] == 3 and c[1] == 1 and c[2] == 0
    bf16_routes = {c[3:] for c in calls["bf16"] if is3x3(c)}
    assert bf16_routes <= {(2, 0), (4, 1)}, bf16_routes
    stray = {c[3:] for c in calls["fp16"] if is3x3(c) and c[3:] != (5, 1)} - bf16_routes
    assert not stray, f"3x3 calls of the fp16 mode on neither the one-product form nor a bf16-mode route: {stray}"
    # the three modes issue the same conv calls in the same order (same geometry): compare them one by one
    assert [c[:3] for c in calls["fp16"]] == [c[:3] for c in calls["fp32"]] == [c[:3] for c in calls["bf16"]]
    wino_fp32 = (5, 3) if (5, 3) in at("fp32") else (5, 0)
    for k, (c32, cb, c16) in enumerate(zip(calls["fp32"], calls["bf16"], calls["fp16"])):
        if c32[3:] == wino_fp32:
            assert c16[3:] == (5, 1), (k, c32, cb, c16)
        else:
            assert c16[3:] == cb[3:], (k, c32, cb, c16)
    # "bf16x3" keeps its tile: every call the bf16 mode runs on the one-product split tile is on the three-product one
    assert [c[:3] for c in calls["bf16x3"]] == [c[:3] for c in calls["bf16"]]
    assert (4, 3) in at("bf16x3") and (4, 1) not in at("bf16x3")
    for k, (cb, cx) in enumerate(zip(calls["bf16"], calls["bf16x3"])):
        if cb[3:] == (4, 1) and is3x3(cb):
            assert cx[3:] == (4, 3), (k, cb, cx)


@pytest.mark.gpu
def test_no_split_planes_next_to_winograd_planes():
    """A conv that runs on the one-plane Winograd packing allocates no split-tile planes (the mode would never read them)."""
    from refid_amd import engine as E
    arena = E.ParamArena({"t.weight": (64, 64, 3, 3), "t.bias": (64,), "u.weight": (16, 64, 3, 3), "u.bias": (16,)}, torch.device("cuda"))
    op = E.ConvOp(arena, "t", compute_dtype="fp16")
    assert op.wp6 is not None and op.wd6 is not None and op.wps is None and op.wds is None
    assert op.wp6.numel() * 2 == 64 + 4 * 16 * 64 * 16 * 2
    thin = E.ConvOp(arena, "u", compute_dtype="fp16")         # 16 output channels: forward as in the bf16 mode, Winograd input gradient
    assert thin.wp6 is None and thin.wps is not None and thin.wd6 is not None and thin.wds is None
    # the other modes keep the packings and routes they had: "bf16x3" holds Winograd planes it does not run on
    x3 = E.ConvOp(arena, "t", compute_dtype="bf16x3")
    assert x3.wp6 is not None and x3.wd6 is not None and x3.wps is not None and x3.wds is not None
    a = torch.empty(1, 8, 8, 64, device="cuda")
    assert _route(x3._fwd_route(1, 8, 8, a, None, None)) == (4, 3) and _route(x3._dgrad_route(a, 64)) == (4, 3)
    assert _route(op._fwd_route(1, 8, 8, a, None, None)) == (5, 1) and _route(op._dgrad_route(a, 64)) == (5, 1)


def _route(r):
    return r[1]["algo"], r[1].get("terms", 0)


@pytest.mark.gpu
def test_row_range_below_the_winograd_tile_stays_on_the_bf16_route():
    """ci == 2 co with co = 16 (base_num_channels 8 / 16): the input gradient is issued as two halves of 16 rows, fewer than
    the Winograd tile takes.  The halves go where the bf16 mode sends them (split tile, one product), a call for all 32 rows
    goes to the one-product Winograd form as in the fp32 mode."""
    from refid_amd import engine as E
    arena = E.ParamArena({"f.weight": (16, 32, 3, 3), "f.bias": (16,)}, torch.device("cuda"))
    ops16, opsb, ops32 = (E.ConvOp(arena, "f", compute_dtype=dt) for dt in ("fp16", "bf16", "fp32"))
    g = torch.empty(1, 8, 8, 16, device="cuda")
    assert ops16.wd6 is not None and ops16.wds is not None
    assert _route(opsb._dgrad_route(g, 16)) == (4, 1) == _route(ops16._dgrad_route(g, 16))
    assert _route(ops32._dgrad_route(g, 32))[0] == 5 and _route(ops16._dgrad_route(g, 32)) == (5, 1)
    assert _route(ops32._dgrad_route(g, 16))[0] != 5


@pytest.mark.gpu
def test_graph_replayed_steps_equal_eager_steps_fp16():
    """Three train steps captured into a hipGraph and replayed == the same steps launched eagerly, bit for bit (the one-plane
    packings and their scale pre-pass are written inside the captured step like the others)."""
    from refid_amd.train import TwoImageEventRecurrentRestorationModel
    from test_hip_train_step import _opt
    base = 16
    P = O.make_params(26, base_num_channels=base, mode="hash", seed=5)
    batches = [O.make_inputs(2, 3, 32, 32, 26, seed=30 + i, mode="hash") for i in range(3)]

    def run(graph):
        m = TwoImageEventRecurrentRestorationModel(_opt(26, base, T_max=6, dtype="fp16"))
        m.net_g.load_state_dict(P)
        m.set_graph_mode(graph)
        losses, norms = [], []
        for it, (x, ev, gt) in enumerate(batches, start=1):
            m.update_learning_rate(it)
            m.feed_data({"lq": x, "voxel": ev, "gt": gt})
            m.optimize_parameters(it)
            losses.append(m.get_current_log()["l_pix"])
            norms.append(m.grad_norm())
        assert m.step_count == len(batches)
        return losses, norms, {k: v.double().cpu() for k, v in m.net_g.state_dict().items()}, m

    le, ne, sde, _ = run(False)
    lg, ng, sdg, mg = run(True)
    assert mg._graph is not None and len(mg._graph["graphs"]) == 1
    assert all(np.isfinite(le)) and lg == le and ng == ne, (lg, le, ng, ne)
    for k in sde:
        assert torch.equal(sdg[k], sde[k]), k
