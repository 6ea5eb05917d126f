"""The WEIGHTED fused GNO kernels (the WFwd / WBwd instantiations of csrc/gno.hip, gno_bf16.hip, gno_bwd3_bf16.hip; gaot_gno_fwd_w /
gaot_gno_bwd_w; functional.GnoWFn) and IntegralTransform with use_attn=True on them.

  1. fp32 mode, kernels against the fp64 statement tests/gno_w_ref.py with a random SIGNED weight per edge: modes linear / nonlinear /
     nonlinear_kernelonly, 1-3 hidden layers (forward also 4), E in {1, 31, 32, 33, 127, 128, 129} on 40 sources / 23 queries and
     E = 2003 on 3000 / 700 (a query row of 200 edges, a heavy source row, empty rows on both sides).  The project's fp32 bars
     (tests/test_edgeops_gpu.py): out rtol 1e-4 / atol 1e-5; grad_f, dt, every dW / db and dalpha rtol 1e-3 / atol 1e-5.
  2. alpha = 1/deg reproduces the unweighted fused kernels (ops.gno_forward / gno_nl_forward) at rtol 1e-5: another rounding of the
     same sum (alpha_e k f added, against the sum divided once), so not bit equality; atol 1e-6 stands for the rounding of the
     sum itself, 2^-23 of the sum of the terms' magnitudes (at most ~8 here).
  3. bf16 mode at E = 2003, 1-4 hidden layers, the bf16 bars of tests/test_gno_gpu.py: outputs within 3e-2 x peak, cosine of all
     gradients concatenated >= 0.999; dalpha on its own under the same two bars.
  4. the module against the oracle (cosine and dot_product x the three transform types; coord_dim 3, 2, and 2 on 3-D coordinates;
     C = 16 and C = 64 (two passes: dalpha summed by autograd); hidden 48), the bars of tests/test_gno_attn_scores_gpu.py in both
     precisions, and the timing keys show the weighted kernels (and, for dot_product, the bilinear score kernels) ran.  Hidden 96, MLP
     dropout in training and f_y=None have no plan and run the general path.
  5. no per-edge row tensor: E = 400 003, the peak of allocated memory rises by less than E x 128 B (control: the general path rises
     above E x 256 B).
  6. two calls are bit-identical in both precisions, dalpha included; the module's step replays from a hipGraph bit for bit.
  7. one training step of a small GAOT3D with use_attn=True against the oracle; the weighted kernels ran on the encoder and decoder."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import gaot_oracle as orc  # noqa: E402
import gno_nl_ref as N  # noqa: E402
import gno_w_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PREC = {"fp32": 0, "bf16": 1}


def close(name, a, b, rtol, atol):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    err = (a - b).abs().max().item() if a.numel() else 0.0
    print(f"[parity] {name}: max_abs={err:.3e} ref_peak={b.abs().max().item() if b.numel() else 0:.3e}")
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"{name}: max abs err {err:.3e}"


def cosine(pairs):
    num = d1 = d2 = 0.0
    for a, b in pairs:
        a, b = a.detach().cpu().double().flatten(), b.detach().cpu().double().flatten()
        num += (a * b).sum().item(); d1 += (a * a).sum().item(); d2 += (b * b).sum().item()
    return num / max(d1 ** 0.5 * d2 ** 0.5, 1e-300)


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
_REF = {}


def _ref(kind, mode, e, nh):
    """the case and its fp64 reference, computed once and shared"""
    key = (kind, mode, e, nh)
    if key not in _REF:
        c = WR.w_case(kind, mode, e, nh)
        _REF[key] = (c, WR.w_ref(c))
    return _REF[key]


def _kernel_inputs(c, alpha=None):
    from gaot_3d_amd import ops
    g = ops.build_graph(c["ei"].to(DEV), c["n_src"], c["n_dst"])
    perm = g.by_dst.perm.long()                                  # dst-sorted position -> edge of the case's list
    a = (c["alpha"] if alpha is None else alpha).to(DEV)[perm].contiguous()
    ws = [w.to(DEV) for w in c["ws"]]
    bs = [b.to(DEV) for b in c["bs"]]
    y, x, f = c["y"].to(DEV), c["x"].to(DEV), c["f"].to(DEV)
    t = None
    if c["mode"] != "linear":
        t = (f.double() @ ws[0][:, 6:].double().t()).float().contiguous()
        ws = [ws[0][:, :6].contiguous()] + ws[1:]
    fk = None if c["mode"] == "nonlinear_kernelonly" else f
    return g, perm, a, ws, bs, y, x, fk, t


def _kernels(c, precision, backward=True, alpha=None, want_grad_w=True):
    from gaot_3d_amd import ops
    g, perm, a, ws, bs, y, x, fk, t = _kernel_inputs(c, alpha)
    res = {"out": ops.gno_w_forward(c["mode"], ws, bs, y, x, fk, t, a, g, precision=PREC[precision])}
    if backward:
        gf, gt, gw, gb, gew = ops.gno_w_backward(c["mode"], ws, bs, y, x, fk, t, a, c["gout"].to(DEV), g, precision=PREC[precision],
                                                 want_grad_w=want_grad_w)
        res.update(grad_f=gf, dt=gt, dalpha=gew)
        for l, (u, v) in enumerate(zip(gw, gb)):
            res[f"dW{l}"], res[f"db{l}"] = u, v
    torch.cuda.synchronize()
    res["perm"] = perm.cpu()
    return res


def _grad_names(ref):
    return [k for k, v in ref.items() if k != "out" and v is not None]


@pytest.mark.parametrize("nh", [1, 2, 3, 4])
@pytest.mark.parametrize("mode", WR.MODES)
def test_kernels_fp32_against_reference(mode, nh):
    for kind, e in [("tail", e) for e in WR.TILE_E] + [("mid", WR.MID_E)]:
        c, ref = _ref(kind, mode, e, nh)
        got = _kernels(c, "fp32", backward=nh <= 3)              # four hidden layers: forward only in fp32 mode
        tag = f"{c['tag']}/fp32"
        close(f"{tag}/out", got["out"], ref["out"], 1e-4, 1e-5)
        if nh > 3:
            continue
        for k in _grad_names(ref):
            r = ref[k][got["perm"]] if k == "dalpha" else ref[k]
            close(f"{tag}/{k}", got[k], r, 1e-3, 1e-5)
        assert (got["grad_f"] is None) == (mode == "nonlinear_kernelonly") and (got["dt"] is None) == (mode == "linear")


def test_fp32_backward_refuses_four_hidden_layers():
    from gaot_3d_amd._lib import GaotError
    c, _ = _ref("tail", "linear", 33, 4)
    with pytest.raises(GaotError, match="unsupported MLP shape"):
        _kernels(c, "fp32")


def test_dalpha_is_optional():
    c, ref = _ref("mid", "nonlinear", WR.MID_E, 2)
    got = _kernels(c, "fp32", want_grad_w=False)
    assert got["dalpha"] is None
    close("w_no_dalpha/grad_f", got["grad_f"], ref["grad_f"], 1e-3, 1e-5)
    close("w_no_dalpha/dW2", got["dW2"], ref["dW2"], 1e-3, 1e-5)


def test_empty_edge_list():
    c = dict(WR.w_case("tail", "linear", 1, 2))
    c["ei"] = c["ei"][:, :0]
    c["alpha"] = c["alpha"][:0]
    got = _kernels(c, "fp32")
    assert float(got["out"].abs().max()) == 0.0 and float(got["grad_f"].abs().max()) == 0.0 and got["dalpha"].shape == (0,)
    assert all(float(got[f"dW{l}"].abs().max()) == 0.0 for l in range(3))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", WR.MODES)
def test_inverse_degree_weights_reproduce_the_mean_kernels(mode, precision):
    from gaot_3d_amd import ops
    c, _ = _ref("mid", mode, WR.MID_E, 2)
    q = c["ei"][1].long()
    deg = torch.bincount(q, minlength=c["n_dst"]).float()
    got = _kernels(c, precision, backward=False, alpha=(1.0 / deg)[q])
    g, perm, a, ws, bs, y, x, fk, t = _kernel_inputs(c)
    if mode == "linear":
        ref = ops.gno_forward(ws, bs, y, x, fk, g, precision=PREC[precision])
    else:
        ref = ops.gno_nl_forward(mode, ws, bs, y, x, fk, t, g, precision=PREC[precision])
    torch.cuda.synchronize()
    close(f"w_inv_deg_{mode}/{precision}/out", got["out"], ref, 1e-5, 1e-6)
    assert bool((got["out"][deg.to(DEV) == 0] == 0).all())


PARITY = []


@pytest.mark.parametrize("nh", [1, 2, 3, 4])
@pytest.mark.parametrize("mode", WR.MODES)
def test_kernels_bf16_against_reference(mode, nh):
    c, ref = _ref("mid", mode, WR.MID_E, nh)
    got = _kernels(c, "bf16")
    peak, err = ref["out"].abs().max().item(), (got["out"].cpu().double() - ref["out"]).abs().max().item()
    names = [k for k in _grad_names(ref) if k != "dalpha"]
    cos = cosine([(got[k], ref[k]) for k in names])
    da_ref = ref["dalpha"][got["perm"]]
    da_peak, da_err = da_ref.abs().max().item(), (got["dalpha"].cpu().double() - da_ref).abs().max().item()
    da_cos = cosine([(got["dalpha"], da_ref)])
    print(f"[parity] {c['tag']}/bf16: out max_abs={err:.3e} peak={peak:.3e} ({err / peak:.2e} x peak), grad cosine={cos:.6f}; "
          f"dalpha max_abs={da_err:.3e} peak={da_peak:.3e} ({da_err / da_peak:.2e} x peak), cosine={da_cos:.6f}")
    assert err <= 3e-2 * peak
    assert cos >= 0.999
    assert da_err <= 3e-2 * da_peak
    assert da_cos >= 0.999


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_kernel_calls_are_bit_identical(precision):
    for mode in WR.MODES:
        c, _ = _ref("mid", mode, WR.MID_E, 2)
        a, b = _kernels(c, precision), _kernels(c, precision)
        bad = [k for k in a if a[k] is not None and not torch.equal(a[k], b[k])]
        assert not bad, (mode, bad)


# ---- the module ---------------------------------------------------------------------------------------------------------------------------
def _case(tt, cin=32, cout=32, hidden=64, cd=3):
    c = dict(N.nl_case("mid", "nonlinear" if tt == "linear" else tt, 2003, 2, cin, cout, hidden, cd))
    if tt == "linear":
        c["ws"] = [c["ws"][0][:, :2 * cd].clone()] + list(c["ws"][1:])
        c["mode"] = "linear"
    return c


def _module(c, coord_dim, attention_type):
    from gaot_3d_amd.model.layers.integral_transform import IntegralTransform
    layers = [c["ws"][0].shape[1]] + [w.shape[0] for w in c["ws"]]
    torch.manual_seed(11)     # query_proj / key_proj: the module's own initialisation, seeded
    it = IntegralTransform(channel_mlp_layers=layers, transform_type=c["mode"], use_attn=True, coord_dim=coord_dim,
                           attention_type=attention_type)
    with torch.no_grad():
        for fc, w, b in zip(it.channel_mlp.fcs, c["ws"], c["bs"]):
            fc.weight.copy_(w.view_as(fc.weight))
            fc.bias.copy_(b)
    return it


def _oracle(c, it, coord_dim, attention_type):
    leaf = {"it." + k: v.detach().clone().requires_grad_() for k, v in it.state_dict().items()}
    f_r = c["f"].clone().requires_grad_()
    out_r = orc.integral_transform(leaf, "it.", c["y"], c["x"], c["ei"].long(), f_r, c["mode"], True, coord_dim, attention_type)
    gs = torch.autograd.grad((out_r * c["gout"]).sum(), [f_r] + list(leaf.values()))
    return out_r.detach(), list(gs)


def _device_inputs(c):
    from gaot_3d_amd import edgeops as EO
    from gaot_3d_amd import ops
    g = ops.build_graph(c["ei"].to(DEV), c["n_src"], c["n_dst"])
    EO.src_to_dst_map(g)
    return c["y"].to(DEV), c["x"].to(DEV), c["f"].to(DEV), c["gout"].to(DEV), g


def _run(it, inputs, precision="fp32", f_none=False):
    """one forward + backward of the module on the GPU -> (out, [grad f_y, grad of every parameter], timing keys)"""
    import gaot_3d_amd
    from gaot_3d_amd import ops
    y, x, f, gout, g = inputs
    f = None if f_none else f.clone().requires_grad_()
    gaot_3d_amd.set_precision(precision)
    ops.timing_reset(True)
    try:
        out = it(y, x, None, f_y=f, graph=g)
        grads = torch.autograd.grad((out * gout[:, :out.shape[1]]).sum(), ([] if f_none else [f]) + list(it.parameters()))
        torch.cuda.synchronize()
        used = set(ops.timing_summary())
    finally:
        ops.timing_reset(False)
        gaot_3d_amd.set_precision("fp32")
    return out.detach(), list(grads), used


def _ran_weighted(used, tt):
    md = WR.MODES.index(tt)
    return any(k.startswith(f"gno_fwd_w{md}_") for k in used) and any(k.startswith(f"gno_bwd_w{md}_") for k in used)


# (transform type, attention, C_in, C_out, hidden, coordinate dimension, coord_dim of the scores)
MODULE_CASES = [(tt, at, 32, 32, 64, 3, 3) for at in ("cosine", "dot_product") for tt in WR.MODES] + [
    ("nonlinear", "dot_product", 16, 16, 48, 2, 2),          # one padded pass, padded hidden width, 2-D coordinates
    ("nonlinear_kernelonly", "cosine", 16, 16, 48, 2, 2),
    ("linear", "cosine", 32, 32, 64, 3, 2),                  # the scores see two of three coordinates
    ("linear", "dot_product", 32, 32, 64, 3, 2),
    ("nonlinear", "cosine", 64, 64, 64, 3, 3),               # two passes: dalpha summed over the passes
    ("linear", "dot_product", 64, 64, 48, 3, 3),
]
_ORACLE = {}


def _module_case(cfg):
    tt, at, cin, cout, hidden, cd, coord_dim = cfg
    if cfg not in _ORACLE:
        c = _case(tt, cin, cout, hidden, cd)
        it = _module(c, coord_dim, at)
        _ORACLE[cfg] = (c, it.state_dict(), _oracle(c, it, coord_dim, at))
    c, sd, (out_r, gs) = _ORACLE[cfg]
    it = _module(c, coord_dim, at)
    it.load_state_dict(sd)
    return c, it.to(DEV), out_r, gs


@pytest.mark.parametrize("cfg", MODULE_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_module_against_oracle_fp32(cfg):
    c, it, out_r, gs = _module_case(cfg)
    out, grads, used = _run(it, _device_inputs(c))
    tag = "w_module_" + "-".join(str(v) for v in cfg)
    close(f"{tag}/out", out, out_r, 1e-4, 1e-5)
    close(f"{tag}/grad_f", grads[0], gs[0], 1e-3, 1e-5)
    for (k, _), a, b in zip(it.named_parameters(), grads[1:], gs[1:]):
        close(f"{tag}/grad/{k}", a.reshape(b.shape), b, 1e-3, 1e-5)
    assert _ran_weighted(used, cfg[0]), used
    if cfg[1] == "dot_product":
        assert {"edge_bilinear_fwd", "edge_bilinear_bwd"} <= used, used


@pytest.mark.parametrize("cfg", MODULE_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_module_against_oracle_bf16(cfg):
    c, it, out_r, gs = _module_case(cfg)
    out, grads, used = _run(it, _device_inputs(c), "bf16")
    peak, err = out_r.abs().max().item(), (out.cpu() - out_r).abs().max().item()
    cos = cosine(zip(grads, gs))
    print(f"[parity] w_module_{'-'.join(str(v) for v in cfg)}/bf16: out max_abs={err:.3e} peak={peak:.3e}, grad cosine={cos:.6f}")
    assert err <= 3e-2 * peak
    assert cos >= 0.999
    assert _ran_weighted(used, cfg[0]), used
    if cfg[1] == "dot_product":
        assert {"edge_bilinear_fwd", "edge_bilinear_bwd"} <= used, used


def test_shapes_without_a_plan_run_the_general_path():
    # a hidden width of 96
    c = _case("linear", 32, 32, 96, 3)
    it = _module(c, 3, "cosine").to(DEV)
    inputs = _device_inputs(c)
    fcs = list(it.channel_mlp.fcs)
    assert it._fused_attn_plan(fcs, inputs[2], inputs[0], inputs[1]) is None
    out_r, _ = _oracle(c, it.cpu(), 3, "cosine")
    out, _, used = _run(it.to(DEV), inputs)
    close("w_general_hidden96/out", out, out_r, 1e-4, 1e-5)
    assert not any(k.startswith("gno_fwd_w") for k in used), used
    # MLP dropout in training; f_y = None
    c = _case("linear")
    it = _module(c, 3, "dot_product").to(DEV)
    inputs = _device_inputs(c)
    fcs = list(it.channel_mlp.fcs)
    assert it._fused_attn_plan(fcs, inputs[2], inputs[0], inputs[1]) is not None
    assert it._fused_plan(fcs, inputs[2], inputs[0], inputs[1]) is None
    assert it._fused_attn_plan(fcs, None, inputs[0], inputs[1]) is None
    _, _, used = _run(it, inputs, f_none=True)
    assert not any(k.startswith("gno_fwd_w") for k in used), used
    it.channel_mlp.dropout_p = 0.1
    it.train()
    assert it._fused_attn_plan(fcs, inputs[2], inputs[0], inputs[1]) is None
    it.eval()
    assert it._fused_attn_plan(fcs, inputs[2], inputs[0], inputs[1]) is not None


# ---- no per-edge row tensor ---------------------------------------------------------------------------------------------------------------
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
def test_no_per_edge_row_tensor(precision):
    import gaot_3d_amd
    from gaot_3d_amd import edgeops as EO
    from gaot_3d_amd import ops
    from gaot_3d_amd.model.layers.integral_transform import IntegralTransform
    ei = N.rand_graph(MEM_SRC, MEM_DST, MEM_E, 5, heavy_dst=5000, heavy_src=3000).to(DEV)
    g = ops.build_graph(ei, MEM_SRC, MEM_DST)
    EO.src_to_dst_map(g)                     # the graph and its maps are built beforehand
    gen = torch.Generator().manual_seed(3)
    y = (torch.rand(MEM_SRC, 3, generator=gen) * 2 - 1).to(DEV)
    x = (torch.rand(MEM_DST, 3, generator=gen) * 2 - 1).to(DEV)
    f = torch.randn(MEM_SRC, 32, generator=gen).to(DEV).requires_grad_()
    gout = torch.randn(MEM_DST, 32, generator=gen).to(DEV)
    torch.manual_seed(0)
    it = IntegralTransform(channel_mlp_layers=[6 + 32, 64, 64, 64, 32], transform_type="nonlinear", use_attn=True, coord_dim=3,
                           attention_type="dot_product").to(DEV)
    gaot_3d_amd.set_precision(precision)
    try:
        rise = _peak_rise(it, y, x, f, g, gout)
        plan = it._fused_attn_plan
        it._fused_attn_plan = lambda *a, **k: None
        try:
            rise_general = _peak_rise(it, y, x, f, g, gout)
        finally:
            it._fused_attn_plan = plan
    finally:
        gaot_3d_amd.set_precision("fp32")
    print(f"[memory] {precision} weighted nonlinear dot_product, E = {MEM_E}: peak rise {rise / MEM_E:.1f} B/edge fused, "
          f"{rise_general / MEM_E:.1f} B/edge general path (one [E, 64] fp32 row tensor: 256 B/edge)")
    assert rise < MEM_E * 128, (rise, MEM_E * 128)
    assert rise_general > MEM_E * 256


# ---- determinism ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_module_two_calls_are_bit_identical(precision):
    for cfg in MODULE_CASES[:6]:
        c, it, _, _ = _module_case(cfg)
        inputs = _device_inputs(c)
        (o1, g1, _), (o2, g2, _) = _run(it, inputs, precision), _run(it, inputs, precision)
        names = ["grad_f"] + [k for k, _ in it.named_parameters()]
        bad = ([] if torch.equal(o1, o2) else ["out"]) + [n for n, u, v in zip(names, g1, g2) if not torch.equal(u, v)]
        assert not bad, (cfg, bad)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_module_step_replays_from_a_hipgraph(precision):
    """forward + backward of the dot-product module on the weighted kernels captured into a hipGraph: the replay gives the eager step's
    output and gradients bit for bit (the eager step runs first, on a side stream)"""
    import gaot_3d_amd
    c, it, _, _ = _module_case(MODULE_CASES[4])          # nonlinear, dot_product
    y, x, f, gout, g = _device_inputs(c)
    f.requires_grad_()
    params = dict(it.named_parameters())

    def step():
        f.grad = None
        for p in params.values():
            p.grad = None
        out = it(y, x, None, f_y=f, graph=g)
        out.backward(gout)
        return out.detach()
    gaot_3d_amd.set_precision(precision)
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            out = step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        out_e, gf_e = out.clone(), f.grad.clone()
        eager = {k: p.grad.clone() for k, p in params.items()}
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph, capture_error_mode="global"):
            out_g = step()
        graph.instantiate()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_g, out_e) and torch.equal(f.grad, gf_e)
        bad = [k for k, p in params.items() if not torch.equal(p.grad, eager[k])]
        assert not bad, bad
        del graph
    finally:
        gaot_3d_amd.set_precision("fp32")


# ---- the whole model --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_model_step_with_attention_runs_the_weighted_kernels(precision):
    """the configuration of tests/test_edgeops_gpu.py::test_model_with_nonlinear_attention_pointnet (encoder 'linear', decoder
    'nonlinear', dot-product attention weights on both, 3000 points, 8^3 tokens) at that test's bars"""
    import gaot_3d_amd
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd import ops
    from gaot_3d_amd.data import make_synthetic_sample
    from gaot_3d_amd.model import init_model
    from gaot_3d_amd.model.layers.attn import AttentionConfig, FFNConfig, TransformerConfig
    from gaot_3d_amd.model.layers.magno import MAGNOConfig
    cfg = types.SimpleNamespace(
        magno=MAGNOConfig(gno_coord_dim=3, lifting_channels=32, encoder_feature_attr="pos", mlp_type="linear",
                          use_geoembed=[True, True], embedding_method="pointnet", pooling="max",
                          in_gno_transform_type="linear", out_gno_transform_type="nonlinear",
                          use_attn=True, attention_type="dot_product", neighbor_strategy="knn", k_neighbors=6,
                          precompute_edges=True),
        transformer=TransformerConfig(patch_size=2, hidden_size=256, num_layers=2, positional_embedding="rope",
                                      attn_config=AttentionConfig(hidden_size=256, num_heads=8, num_kv_heads=8,
                                                                  atten_dropout=0.0),
                                      ffn_config=FFNConfig(hidden_size=1024)),
        latent_tokens=(8, 8, 8))
    torch.manual_seed(0)
    model = init_model(3, 2, "gaot_3d", cfg)
    batch, tokens = make_synthetic_sample(3000, cfg.latent_tokens, k=6, in_normals=False, surface=False, seed=1, out_channels=2)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    pred_r, loss_r, grads_r = orc.train_step_grads(sd, cfg, batch, tokens)
    gaot_3d_amd.set_precision(precision)
    ops.timing_reset(True)
    try:
        model = model.to(DEV).train()
        bd = batch.to(DEV)
        pred = model(batch=bd, tokens_pos=tokens.to(DEV))
        loss = GF.mse_loss(pred, bd.x)
        loss.backward()
        torch.cuda.synchronize()
        used = set(ops.timing_summary())
    finally:
        ops.timing_reset(False)
        gaot_3d_amd.set_precision("fp32")
    assert _ran_weighted(used, "linear"), used            # the encoder
    assert _ran_weighted(used, "nonlinear"), used         # the decoder
    if precision == "fp32":
        close("w_model/pred", pred, pred_r, 1e-4, 2e-5)
        close("w_model/loss", loss, loss_r, 1e-5, 1e-7)
        for k, p in model.named_parameters():
            if p.requires_grad:
                close(f"w_model/grad/{k}", p.grad, grads_r[k], 1e-3, 1e-5)
    else:
        close("w_model_bf16/pred", pred, pred_r, 2e-2, 2e-2)
        cos = cosine([(p.grad, grads_r[k]) for k, p in model.named_parameters() if p.requires_grad])
        print(f"[parity] w_model bf16 grad cosine = {cos:.6f}")
        assert cos >= 0.999
