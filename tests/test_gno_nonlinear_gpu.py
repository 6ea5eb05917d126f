"""transform_type 'nonlinear' / 'nonlinear_kernelonly' of IntegralTransform on the fused GNO kernels (csrc/gno.hip, gno_bf16.hip,
gno_bwd3_bf16.hip in their MODE_NONLINEAR / MODE_KERNELONLY instantiations, gaot_gno_fwd_nl / gaot_gno_bwd_nl).

  * the new entry points exist and `_fused_plan` takes both types on the shipped shapes (not with use_attn or without f_y);
  * no per-edge tensor: forward + backward of the module raise the peak of allocated memory by less than E x 64 x 4 bytes, the size
    of ONE per-edge hidden tensor (control: the fused linear transform stays under it, the general path does not);
  * fp32 mode against the oracle on the CPU (oracle/gaot_oracle.py integral_transform): outputs rtol 1e-4 / atol 1e-5, gradients
    with respect to f_y and every parameter (both column blocks of W_0 separately) rtol 1e-3 / atol 1e-5 -- the bars of
    tests/test_edgeops_gpu.py for this operator -- and, in one case per type, with respect to y_pos / x_pos at FP32_BAR of
    tests/test_coord_grad_gpu.py;
  * two calls of forward + backward are bit-identical, in both precision modes;
  * a whole model with a 'nonlinear' decoder: one training step against the oracle, and the same step captured into a hipGraph
    replays to the eager step's loss and gradients bit for bit (the comparison of tests/test_trajectory_gpu.py).
The bf16 kernels against the fp64 rounding model: tests/test_gno_nonlinear_bf16_fp64_gpu.py.  Cases: tests/gno_nl_ref.py."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import gaot_oracle as orc  # noqa: E402
import gno_nl_ref as N  # noqa: E402
from test_coord_grad_gpu import FP32_BAR  # noqa: E402
from test_coord_grad_gpu import check as coord_check  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def close(name, a, b, rtol, atol):
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    err = (a - b).abs().max().item() if a.numel() else 0.0
    print(f"[parity] {name}: max_abs={err:.3e} ref_peak={b.abs().max().item() if b.numel() else 0:.3e}")
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"{name}: max abs err {err:.3e}"


def _module(c, use_attn=False):
    from gaot_3d_amd.model.layers.integral_transform import IntegralTransform
    layers = [c["ws"][0].shape[1]] + [w.shape[0] for w in c["ws"]]
    it = IntegralTransform(channel_mlp_layers=layers, transform_type=c["mode"], use_attn=use_attn, coord_dim=c["y"].shape[1])
    with torch.no_grad():
        for fc, w, b in zip(it.channel_mlp.fcs, c["ws"], c["bs"]):
            fc.weight.copy_(w.view_as(fc.weight))
            fc.bias.copy_(b)
    return it


def test_entry_points_exist():
    """the C ABI and its binding carry the new entry points (absent before this feature)"""
    from gaot_3d_amd import _lib, ops
    lib = _lib.load()
    for name in ("gaot_gno_fwd_nl", "gaot_gno_bwd_nl", "gaot_gno_bwd_nl_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert callable(ops.gno_nl_forward) and callable(ops.gno_nl_backward)
    assert lib.gaot_abi_version() == 11


@pytest.mark.parametrize("mode", N.MODES)
@pytest.mark.parametrize("layers", [[6 + 32, 64, 64, 64, 32], [6 + 32, 64, 64, 32]], ids=["nh3", "nh2"])
def test_fused_plan_takes_the_shipped_shapes(mode, layers):
    from gaot_3d_amd.model.layers.integral_transform import IntegralTransform
    y, x, f = torch.rand(50, 3, device=DEV), torch.rand(20, 3, device=DEV), torch.randn(50, 32, device=DEV)
    it = IntegralTransform(channel_mlp_layers=layers, transform_type=mode).to(DEV)
    fcs = list(it.channel_mlp.fcs)
    assert it._fused_plan(fcs, f, y, x) is not None
    assert it._fused_plan(fcs, None, y, x) is None
    att = IntegralTransform(channel_mlp_layers=layers, transform_type=mode, use_attn=True, coord_dim=3).to(DEV)
    assert att._fused_plan(list(att.channel_mlp.fcs), f, y, x) is None
    # a first layer that does not match [y, x, f_y] stays on the general path
    assert it._fused_plan(fcs, torch.randn(50, 16, device=DEV), y, x) is None


# ---- no per-edge tensor ---------------------------------------------------------------------------------------------------------------
MEM_E, MEM_SRC, MEM_DST = 400003, 20000, 7000


def _peak_rise(it, y, x, f, g, gout):
    def step():
        for p in it.parameters():
            p.grad = None
        f.grad = None
        out = it(y, x, None, f_y=f, graph=g)
        out.backward(gout)
    step()                                   # warm-up: workspaces of the caching allocator, lazily built tables
    torch.cuda.synchronize()
    for p in it.parameters():
        p.grad = None
    f.grad = None
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_no_per_edge_tensor(precision):
    import gaot_3d_amd
    from gaot_3d_amd import ops
    from gaot_3d_amd.model.layers.integral_transform import IntegralTransform
    bound = MEM_E * 64 * 4
    ei = N.rand_graph(MEM_SRC, MEM_DST, MEM_E, 5, heavy_dst=5000, heavy_src=3000).to(DEV)
    g = ops.build_graph(ei, MEM_SRC, MEM_DST)
    gen = torch.Generator().manual_seed(3)
    y = (torch.rand(MEM_SRC, 3, generator=gen) * 2 - 1).to(DEV)
    x = (torch.rand(MEM_DST, 3, generator=gen) * 2 - 1).to(DEV)
    f = torch.randn(MEM_SRC, 32, generator=gen).to(DEV).requires_grad_()
    gout = torch.randn(MEM_DST, 32, generator=gen).to(DEV)
    gaot_3d_amd.set_precision(precision)
    try:
        rises = {}
        for tt in ("linear",) + N.MODES:
            torch.manual_seed(0)
            it = IntegralTransform(channel_mlp_layers=[6 + (0 if tt == "linear" else 32), 64, 64, 64, 32], transform_type=tt).to(DEV)
            rises[tt] = _peak_rise(it, y, x, f, g, gout)
            if tt != "linear":
                rises[tt + "/general"] = _peak_rise_general(it, y, x, f, g, gout)
    finally:
        gaot_3d_amd.set_precision("fp32")
    for k, v in rises.items():
        print(f"[memory] {precision} {k}: peak rise {v / 2**20:.1f} MiB (one per-edge hidden tensor: {bound / 2**20:.1f} MiB)")
    assert rises["linear"] < bound                       # control: the fused linear transform
    for tt in N.MODES:
        assert rises[tt] < bound, (tt, rises[tt], bound)
        assert rises[tt + "/general"] > bound            # control: the general path materialises several of them (printed above)


def _peak_rise_general(it, y, x, f, g, gout):
    plan = it._fused_plan
    it._fused_plan = lambda *a, **k: None
    try:
        return _peak_rise(it, y, x, f, g, gout)
    finally:
        it._fused_plan = plan


# ---- fp32 mode against the oracle -----------------------------------------------------------------------------------------------------
def _oracle(c, coords):
    leaf = {}
    for i, (w, b) in enumerate(zip(c["ws"], c["bs"])):
        leaf[f"it.channel_mlp.fcs.{i}.weight"] = w.clone().requires_grad_()
        leaf[f"it.channel_mlp.fcs.{i}.bias"] = b.clone().requires_grad_()
    y, x, f = (c[k].clone().requires_grad_() for k in ("y", "x", "f"))
    out = orc.integral_transform(leaf, "it.", y, x, c["ei"].long(), f, transform_type=c["mode"])
    if c["ei"].shape[1] == 0:
        return out.detach(), None
    gs = torch.autograd.grad((out * c["gout"]).sum(), [y, x, f] + list(leaf.values()), allow_unused=True)
    return out.detach(), {"y": gs[0], "x": gs[1], "f": gs[2], "params": list(gs[3:])}


def _check_fp32(args, coords=False):
    import gaot_3d_amd
    from gaot_3d_amd import ops
    gaot_3d_amd.set_precision("fp32")
    c = N.nl_case(args[0], args[1], *args[2:])
    cd = c["y"].shape[1]
    out_r, gr = _oracle(c, coords)
    it = _module(c).to(DEV)
    y, x = (c[k].to(DEV).requires_grad_(coords) for k in ("y", "x"))
    f = c["f"].to(DEV).requires_grad_()
    g = ops.build_graph(c["ei"].to(DEV), c["n_src"], c["n_dst"])
    assert it._fused_plan(list(it.channel_mlp.fcs), f, y, x) is not None
    out = it(y, x, None, f_y=f, graph=g)
    tag = c["tag"]
    close(f"{tag}/out", out, out_r, 1e-4, 1e-5)
    out.backward(c["gout"].to(DEV))
    torch.cuda.synchronize()
    if gr is None:      # no edge: the oracle returns zeros that depend on nothing
        assert float(out.abs().max()) == 0.0
        for fc in it.channel_mlp.fcs:
            assert float(fc.weight.grad.abs().max()) == 0.0 and float(fc.bias.grad.abs().max()) == 0.0
        assert f.grad is None or float(f.grad.abs().max()) == 0.0
        return
    close(f"{tag}/grad_f", f.grad, gr["f"], 1e-3, 1e-5)
    for l, fc in enumerate(it.channel_mlp.fcs):
        gw, gw_r = fc.weight.grad.reshape(fc.weight.shape[0], -1), gr["params"][2 * l]
        if l == 0:
            close(f"{tag}/dW0c", gw[:, :2 * cd], gw_r[:, :2 * cd], 1e-3, 1e-5)
            close(f"{tag}/dW0f", gw[:, 2 * cd:], gw_r[:, 2 * cd:], 1e-3, 1e-5)
        else:
            close(f"{tag}/dW{l}", gw, gw_r, 1e-3, 1e-5)
        close(f"{tag}/db{l}", fc.bias.grad, gr["params"][2 * l + 1], 1e-3, 1e-5)
    if coords:
        coord_check(f"{tag}/grad_y", y.grad, gr["y"], FP32_BAR)
        coord_check(f"{tag}/grad_x", x.grad, gr["x"], FP32_BAR)
    # sources without an edge: exact zero rows
    hit = torch.zeros(c["n_src"], dtype=torch.bool)
    hit[c["ei"][0].long()] = True
    if (~hit).any():
        assert float(f.grad.cpu()[~hit].abs().max()) == 0.0


_ID = lambda a: "-".join(str(v) for v in a)  # noqa: E731
FP32_SMALL = N.small_cases(N.NHS_FP32)


@pytest.mark.parametrize("args", FP32_SMALL, ids=_ID)
def test_gno_nl_fp32(args):
    _check_fp32(args)


@pytest.mark.parametrize("mode", N.MODES)
def test_gno_nl_fp32_coordinate_gradients(mode):
    _check_fp32(("mid", mode, 20011, 3, 32, 32, 64, 3), coords=True)


@pytest.mark.parametrize("mode", N.MODES)
def test_gno_nl_fp32_coordinate_gradients_dim2(mode):
    _check_fp32(("mid", mode, 2003, 2, 32, 32, 64, 2), coords=True)


@pytest.mark.parametrize("args", N.LARGE, ids=_ID)
def test_gno_nl_fp32_steady_state(args):
    _check_fp32(args)


@pytest.mark.parametrize("mode", N.MODES)
def test_gno_nl_fp32_empty_graph(mode):
    _check_fp32(("tail", mode, 0, 2, 32, 32, 64, 3))


@pytest.mark.parametrize("mode", N.MODES)
@pytest.mark.parametrize("nh", [1, 3])
def test_ops_entry_points_fp32(mode, nh):
    """ops.gno_nl_forward / gno_nl_backward called directly (one 32-channel pass, the caller's per-node products done here in
    fp64): out, dt -- which the module never shows -- every gradient and the coordinate gradients against the exact form of
    tests/gno_nl_ref.py (equal to the oracle: tests/test_gno_nl_ref_cpu.py)"""
    from gaot_3d_amd import ops
    c = N.nl_case("mid", mode, 2003, nh)
    ref = N.nl_forms(c, "E")
    ws, bs = [w.to(DEV) for w in c["ws"]], [b.to(DEV) for b in c["bs"]]
    y, x, f, gout = (c[k].to(DEV) for k in ("y", "x", "f", "gout"))
    g = ops.build_graph(c["ei"].to(DEV), c["n_src"], c["n_dst"])
    w0c, w0f = ws[0][:, :6].contiguous(), ws[0][:, 6:].contiguous()
    t = (f.double() @ w0f.double().t()).float()
    fk = f if mode == "nonlinear" else None
    wk = [w0c] + ws[1:]
    out = ops.gno_nl_forward(mode, wk, bs, y, x, fk, t, g, precision=0)
    gf, dt, gw, gb, gy, gx = ops.gno_nl_backward(mode, wk, bs, y, x, fk, t, gout, g, precision=0, coords=True)
    gf2, dt2, gw2, gb2 = ops.gno_nl_backward(mode, wk, bs, y, x, fk, t, gout, g, precision=0)
    torch.cuda.synchronize()
    assert (gf is None) == (mode == "nonlinear_kernelonly")
    tag = c["tag"]
    close(f"{tag}/out", out, ref["out"].float(), 1e-4, 1e-5)
    close(f"{tag}/dt", dt, ref["dt"].float(), 1e-3, 1e-5)
    total = dt.double() @ w0f.double() + (gf.double() if gf is not None else 0.0)
    close(f"{tag}/grad_f", total.float(), ref["grad_f"].float(), 1e-3, 1e-5)
    close(f"{tag}/dW0f", (dt.double().t() @ f.double()).float(), ref["dW0f"].float(), 1e-3, 1e-5)
    close(f"{tag}/dW0c", gw[0], ref["dW0c"].float(), 1e-3, 1e-5)
    close(f"{tag}/db0", gb[0], ref["db0"].float(), 1e-3, 1e-5)
    for l in range(1, nh + 1):
        close(f"{tag}/dW{l}", gw[l], ref[f"dW{l}"].float(), 1e-3, 1e-5)
        close(f"{tag}/db{l}", gb[l], ref[f"db{l}"].float(), 1e-3, 1e-5)
    coord_check(f"{tag}/grad_y", gy, ref["grad_y"], FP32_BAR)
    coord_check(f"{tag}/grad_x", gx, ref["grad_x"], FP32_BAR)
    # with and without the coordinate gradients: the same numbers
    assert torch.equal(dt, dt2) and all(torch.equal(u, v) for u, v in zip(gw + gb, gw2 + gb2))
    assert gf is None or torch.equal(gf, gf2)


# ---- determinism ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", N.MODES)
def test_two_calls_are_bit_identical(mode, precision):
    import gaot_3d_amd
    from gaot_3d_amd import ops
    c = N.nl_case("mid", mode, 20011, 3)
    it = _module(c).to(DEV)
    g = ops.build_graph(c["ei"].to(DEV), c["n_src"], c["n_dst"])
    gout = c["gout"].to(DEV)

    def run():
        y, x, f = (c[k].to(DEV).requires_grad_() for k in ("y", "x", "f"))
        out = it(y, x, None, f_y=f, graph=g)
        grads = torch.autograd.grad((out * gout).sum(), [y, x, f] + list(it.parameters()))
        return [out.detach()] + list(grads)
    gaot_3d_amd.set_precision(precision)
    try:
        a, b = run(), run()
        torch.cuda.synchronize()
    finally:
        gaot_3d_amd.set_precision("fp32")
    names = ["out", "grad_y", "grad_x", "grad_f"] + [k for k, _ in it.named_parameters()]
    bad = [n for n, u, v in zip(names, a, b) if not torch.equal(u, v)]
    assert not bad, bad


# ---- whole model ------------------------------------------------------------------------------------------------------------------------
def _model():
    from gaot_3d_amd.data import make_synthetic_sample
    from gaot_3d_amd.model import init_model
    from gaot_3d_amd.model.layers.attn import AttentionConfig, FFNConfig, TransformerConfig
    from gaot_3d_amd.model.layers.magno import MAGNOConfig
    cfg = types.SimpleNamespace(
        magno=MAGNOConfig(gno_coord_dim=3, lifting_channels=32, encoder_feature_attr="pos", mlp_type="linear",
                          use_geoembed=[True, True], in_gno_transform_type="linear", out_gno_transform_type="nonlinear",
                          use_attn=None, neighbor_strategy="knn", k_neighbors=6, precompute_edges=True),
        transformer=TransformerConfig(patch_size=2, hidden_size=256, num_layers=2, positional_embedding="rope",
                                      attn_config=AttentionConfig(hidden_size=256, num_heads=8, num_kv_heads=8,
                                                                  atten_dropout=0.0),
                                      ffn_config=FFNConfig(hidden_size=1024)),
        latent_tokens=(8, 8, 8))
    torch.manual_seed(0)
    model = init_model(3, 2, "gaot_3d", cfg)
    batch, tokens = make_synthetic_sample(3000, cfg.latent_tokens, k=6, in_normals=False, surface=False, seed=1, out_channels=2)
    return cfg, model, batch, tokens


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_model_with_nonlinear_decoder(precision):
    """one training step of a model whose decoder GNO is 'nonlinear' (fused) against the oracle, with the bars of
    test_edgeops_gpu.py::test_model_with_nonlinear_attention_pointnet; then the same step captured into a hipGraph replays to the eager
    step's loss and gradients bit for bit"""
    import gaot_3d_amd
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd import ops
    cfg, model, batch, tokens = _model()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    pred_r, loss_r, grads_r = orc.train_step_grads(sd, cfg, batch, tokens)
    gaot_3d_amd.set_precision(precision)
    try:
        model = model.to(DEV).train()
        bd, tk = batch.to(DEV), tokens.to(DEV)
        params = {k: p for k, p in model.named_parameters() if p.requires_grad}

        def step():
            for p in params.values():
                p.grad = None
            pred = model(batch=bd, tokens_pos=tk)
            loss = GF.mse_loss(pred, bd.x)
            loss.backward()
            return pred.detach(), loss.detach()
        ops.timing_reset(True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            pred, loss = step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        used = set(ops.timing_summary())
        ops.timing_reset(False)
        assert any(k.startswith("gno_fwd_nl1") for k in used) and any(k.startswith("gno_bwd_nl1") for k in used), used
        eager = {k: p.grad.clone() for k, p in params.items()}
        pred_e, loss_e = pred.clone(), loss.clone()
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph, capture_error_mode="global"):
            pred_g, loss_g = step()
        graph.instantiate()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss_g, loss_e) and torch.equal(pred_g, pred_e)
        bad = [k for k, p in params.items() if not torch.equal(p.grad, eager[k])]
        assert not bad, bad
        del graph
    finally:
        ops.timing_reset(False)
        gaot_3d_amd.set_precision("fp32")
    if precision == "fp32":
        close("nonlinear_model/pred", pred_e, pred_r, 1e-4, 2e-5)
        close("nonlinear_model/loss", loss_e, loss_r, 1e-5, 1e-7)
        for k in params:
            close(f"nonlinear_model/grad/{k}", eager[k], grads_r[k], 1e-3, 1e-5)
    else:
        close("nonlinear_model_bf16/pred", pred_e, pred_r, 2e-2, 2e-2)
        num = d1 = d2 = 0.0
        for k in params:
            a, b = eager[k].cpu().double().flatten(), grads_r[k].double().flatten()
            num += (a * b).sum().item(); d1 += (a * a).sum().item(); d2 += (b * b).sum().item()
        cos = num / (d1 ** 0.5 * d2 ** 0.5)
        print(f"[parity] nonlinear model bf16 grad cosine = {cos:.6f}")
        assert cos >= 0.999
