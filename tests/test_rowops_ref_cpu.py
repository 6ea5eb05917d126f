"""The teeth of tests/rowops_ref.py, without a GPU: every hand-written backward formula against fp64 autograd of its forward formula,
the activation formulas against torch's own fp64 functions, the activation ids against csrc/common.h, and the name table
(model/layers/mlp.py: activation_name) entry by entry."""
import os
import re
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rowops_ref as R  # noqa: E402

TOL = 1e-12


def gen(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def same(name, got, ref, tol=TOL):
    err = ((got - ref).abs() / (1.0 + ref.abs())).max().item() if ref.numel() else 0.0
    assert got.shape == ref.shape and err <= tol, (name, err)


act_grid = R.act_grid


TORCH_ACT = {"none": lambda v: v.clone(), "gelu": F.gelu, "relu": F.relu, "silu": F.silu, "tanh": torch.tanh,
             "leaky_relu": F.leaky_relu, "elu": F.elu, "sigmoid": torch.sigmoid, "softplus": F.softplus, "selu": F.selu,
             "relu6": F.relu6, "hardswish": F.hardswish, "mish": F.mish, "gelu_tanh": lambda v: F.gelu(v, approximate="tanh")}


def test_grid_has_the_planted_points():
    v = act_grid()
    assert v.numel() == 4012 and v.numel() % 256 != 0
    assert v[4009].item() > 20.0 and v[4009].item() - 20.0 < 2e-6
    assert torch.signbit(v[4002]) and v[4002] == 0


@pytest.mark.parametrize("name", R.ACT_NAMES)
def test_activation_formulas(name):
    v = act_grid().double()
    # the written-out derivative == autograd of the written-out function, kinks included (torch.where picks autograd's side)
    leaf = v.clone().requires_grad_(True)
    R.act(name, leaf).sum().backward()
    same(name + "'", R.act_grad(name, v), leaf.grad)
    # ... and both == torch's own function in fp64 (a formula that restates the wrong function fails here)
    leaf2 = v.clone().requires_grad_(True)
    yt = TORCH_ACT[name](leaf2)
    yt.sum().backward()
    same(name, R.act(name, v), yt.detach(), 1e-11)
    same(name + "' (torch)", R.act_grad(name, v), leaf2.grad, 1e-11)


def test_kink_conventions():
    """one-sided values where a `<` / `<=` slip would hide"""
    t = lambda *a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    assert R.act_grad("relu", t(0.0, -0.0)).tolist() == [0.0, 0.0]
    assert R.act_grad("leaky_relu", t(0.0)).item() == 0.01
    assert R.act_grad("elu", t(0.0)).item() == 1.0
    assert R.act_grad("relu6", t(0.0, 6.0, 5.999, 1e-30)).tolist() == [0.0, 0.0, 1.0, 1.0]
    assert R.act_grad("hardswish", t(-3.0, 3.0, -3.0000001, 3.0000001)).tolist() == [0.0, 1.0, 0.0, 1.0]
    inner = R.act_grad("hardswish", t(-2.9999999, 2.9999999))
    assert abs(inner[0].item() + 0.5) < 1e-7 and abs(inner[1].item() - 1.5) < 1e-7
    above = float(torch.nextafter(torch.tensor(20.0), torch.tensor(float("inf"))))
    assert R.act("softplus", t(above)).item() == above and R.act_grad("softplus", t(above)).item() == 1.0
    assert R.act("softplus", t(20.0)).item() > 20.0 and R.act_grad("softplus", t(20.0)).item() < 1.0


@pytest.mark.parametrize("name", R.ACT_NAMES)
def test_torch_fp32_kernels_stay_within_the_activation_bar(name):
    """the bar of the GPU test is one torch's own fp32 CPU kernels meet on the same points, forward and gradient"""
    v = act_grid()
    leaf = v.clone().requires_grad_(True)
    y = TORCH_ACT[name](leaf)
    y.sum().backward()
    for what, got, ref in (("fwd", y.detach(), R.act(name, v)), ("grad", leaf.grad, R.act_grad(name, v))):
        ratio = ((got.double() - ref).abs() / R.act_bar(ref, v)).max().item()
        print(f"[parity] torch_fp32_act/{name}/{what}: max err/bar={ratio:.3f}")
        assert ratio <= 1.0, (name, what, ratio)


def test_linear_backward_formula():
    x, w, b, g = gen(37, 5, seed=1), gen(7, 5, seed=2), gen(7, seed=3), gen(37, 7, seed=4)
    for name in R.ACT_NAMES:
        lx, lw, lb = (t.clone().requires_grad_(True) for t in (x, w, b))
        y = TORCH_ACT[name](lx @ lw.t() + lb)
        (y * g).sum().backward()
        yr, z = R.linear_fwd(x, w, b, name)
        dx, dw, db = R.linear_bwd(x, w, z, g, name)
        for nm, a, r in (("y", yr, y.detach()), ("dx", dx, lx.grad), ("dw", dw, lw.grad), ("db", db, lb.grad)):
            same(f"linear/{name}/{nm}", a, r, 1e-11)


@pytest.mark.parametrize("rows,d", [(1, 4), (33, 252), (8, 256)])
def test_rmsnorm_backward_formula(rows, d):
    x, w, g, a, b = gen(rows, d, seed=1), gen(d, seed=2) * 0.1 + 1, gen(rows, d, seed=3), gen(rows, d, seed=4), gen(rows, d, seed=5)
    x[0] *= 1e-3
    lx, lw = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = lx * torch.rsqrt(lx.square().mean(-1, keepdim=True) + 1e-6) * lw
    ((y * g).sum() + (lx * a).sum() + (lx * b).sum()).backward()       # the residual and the tap are aliases of x
    yr, r = R.rmsnorm_fwd(x, w, 1e-6)
    same("y", yr, y.detach())
    same("rstd", r, torch.rsqrt(x.square().mean(-1) + 1e-6))
    dx, dw = R.rmsnorm_bwd(x, w, 1e-6, g, a, b)
    same("dx", dx, lx.grad, 1e-11)
    same("dw", dw, lw.grad, 1e-11)
    dx0, _ = R.rmsnorm_bwd(x, w, 1e-6, g)
    same("dx plain", dx0, lx.grad - a - b, 1e-11)


def test_swiglu_backward_formula():
    f = 12
    ag, du = gen(5, 2 * f, seed=1, scale=4.0), gen(5, f, seed=2)
    ag[0, :7] = torch.tensor([0.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0], dtype=torch.float64)
    leaf = ag.clone().requires_grad_(True)
    u = F.silu(leaf[:, :f]) * leaf[:, f:]
    (u * du).sum().backward()
    same("u", R.swiglu_fwd(ag, f), u.detach())
    same("dag", R.swiglu_bwd(ag, du, f), leaf.grad)


def test_rope_is_the_oracle_rotation_and_its_backward_is_the_inverse():
    sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
    import gaot_oracle as orc
    s, nh, hd, col0, ld = 50, 3, 32, 32, 32 + 3 * 32 + 6
    x, g = gen(2 * s, ld, seed=1), gen(2 * s, ld, seed=2)
    fr = R.rope_freqs(hd)
    out = R.rope(x, ld, col0, nh, hd, s, fr)
    assert torch.equal(out[:, :col0], x[:, :col0]) and torch.equal(out[:, col0 + nh * hd:], x[:, col0 + nh * hd:])
    span = x[:, col0:col0 + nh * hd].float().view(2, s, nh, hd).transpose(1, 2)
    ref = orc.rope_rotate(span, fr).transpose(1, 2).reshape(2 * s, nh * hd)       # fp32 throughout
    assert (out[:, col0:col0 + nh * hd] - ref.double()).abs().max().item() < 1e-5
    same("roundtrip", R.rope(out, ld, col0, nh, hd, s, fr, inverse=True), x)
    # a rotation's transpose is its inverse: <rope(x), g> = <x, rope^-1(g)>
    same("adjoint", (out * g).sum(), (x * R.rope(g, ld, col0, nh, hd, s, fr, inverse=True)).sum(), 1e-11)


@pytest.mark.parametrize("b,d,h,w,p,c", [(1, 1, 1, 1, 1, 4), (1, 2, 2, 2, 2, 8), (2, 4, 6, 2, 2, 32), (1, 6, 3, 9, 3, 4)])
def test_patchify_inverse_and_adjoint(b, d, h, w, p, c):
    grid = gen(b, d * h * w, c, seed=1)
    tok = R.patchify(grid, b, d, h, w, p, c)
    assert tok.shape == (b, (d // p) * (h // p) * (w // p), p ** 3 * c)
    assert torch.equal(R.unpatchify(tok, b, d, h, w, p, c), grid)
    # element (pd, ph, pw | i, j, k, ch) of the tokens is grid node (pd p + i, ph p + j, pw p + k), stated by index
    t6 = tok.view(b, d // p, h // p, w // p, p, p, p, c)
    g4 = grid.view(b, d, h, w, c)
    pd, ph, pw, i, j, k = d // p - 1, 0, w // p - 1, p - 1, 0, p // 2
    assert torch.equal(t6[:, pd, ph, pw, i, j, k], g4[:, pd * p + i, ph * p + j, pw * p + k])
    leaf = grid.clone().requires_grad_(True)
    gt = gen(*tok.shape, seed=2)
    (R.patchify(leaf, b, d, h, w, p, c) * gt).sum().backward()
    assert torch.equal(leaf.grad, R.unpatchify(gt, b, d, h, w, p, c))


def test_mse_scale_mix_axpy_colsum_formulas():
    p, t = gen(1234, 3, seed=1) + 1e3, gen(1234, 3, seed=2)
    t = p + 1e-3 * t
    leaf = p.clone().requires_grad_(True)
    loss = F.mse_loss(leaf, t)
    (loss * 1.7).backward()
    same("mse", R.mse_fwd(p, t), loss.detach())
    same("mse grad", R.mse_bwd(p, t, 1.7), leaf.grad)
    for ns in (1, 3, 8):
        xs = [gen(7, 32, seed=10 + s) for s in range(ns)]
        lg, go = gen(7, ns, seed=3, scale=30.0), gen(7, 32, seed=4)
        lx, ll = [x.clone().requires_grad_(True) for x in xs], lg.clone().requires_grad_(True)
        wts = torch.softmax(ll, -1)
        out = sum(wts[:, s:s + 1] * lx[s] for s in range(ns))
        (out * go).sum().backward()
        ro, rw = R.scale_mix_fwd(lg, xs)
        same("mix out", ro, out.detach())
        same("mix w", rw, wts.detach())
        dlog, dxs = R.scale_mix_bwd(lg, xs, go)
        same("mix dlogits", dlog, ll.grad)
        for s in range(ns):
            same(f"mix dx{s}", dxs[s], lx[s].grad)
    a, b = gen(257, seed=5), gen(7, seed=6)
    al = float(torch.tensor(-0.37, dtype=torch.float32))
    same("axpy", R.axpy(a, b, -0.37, 7), a + al * b.repeat(37)[:257])
    same("axpy plain", R.axpy(a, a, 1.0, 257), 2 * a)
    x = gen(65, 8, seed=7)
    x[:, 5:] = float("nan")
    s, mass = R.colsum(x, 5)
    same("colsum", s, x[:, :5].sum(0))
    assert torch.isfinite(mass).all()
    # chunks / rows per chunk as gaot_colsum computes them
    assert R.colsum_chain(1) == 1 + 7 + 1 + 31 and R.colsum_chain(65) == 5 + 7 + 1 + 31
    assert R.colsum_chain(7001) == 8 + 7 + 4 + 31 and R.colsum_chain(16500) == 9 + 7 + 8 + 31


def test_act_ids_match_common_h():
    from gaot_3d_amd import ops
    text = open(os.path.join(HERE, "..", "gaot_3d_amd", "csrc", "common.h")).read()
    enum = dict((k.lower(), int(v)) for k, v in re.findall(r"GAOT_ACT_([A-Z0-9_]+)\s*=\s*([0-9]+)", text))
    count = enum.pop("count")
    assert count == len(enum) == 14 and sorted(enum.values()) == list(range(count))
    named = {k: v for k, v in ops.ACT.items() if k is not None}
    assert named == enum
    assert ops.ACT[None] == enum["none"] == 0
    assert tuple(sorted(enum, key=enum.get)) == R.ACT_NAMES        # the reference's table is in id order
    # the GEMM epilogue's set (LinearFn: act > 3 runs as its own pass) is none / gelu / relu / silu
    assert [n for n in R.ACT_NAMES if enum[n] <= 3] == ["none", "gelu", "relu", "silu"]


def test_activation_name_accepts_every_table_entry():
    from gaot_3d_amd.model.layers.mlp import activation_name
    from gaot_3d_amd.ops import ACT
    modules = {nn.ReLU(): "relu", nn.SiLU(): "silu", nn.Tanh(): "tanh", nn.LeakyReLU(): "leaky_relu", nn.ELU(): "elu",
               nn.Sigmoid(): "sigmoid", nn.Softplus(): "softplus", nn.SELU(): "selu", nn.ReLU6(): "relu6",
               nn.Hardswish(): "hardswish", nn.Mish(): "mish", nn.GELU(): "gelu", nn.GELU(approximate="tanh"): "gelu_tanh",
               nn.Identity(): "none"}
    for fn, want in modules.items():
        assert activation_name(fn) == want, fn
    callables = {F.gelu: "gelu", F.relu: "relu", torch.relu: "relu", F.silu: "silu", F.tanh: "tanh", torch.tanh: "tanh",
                 F.leaky_relu: "leaky_relu", F.elu: "elu", F.sigmoid: "sigmoid", torch.sigmoid: "sigmoid", F.softplus: "softplus",
                 F.selu: "selu", F.relu6: "relu6", F.hardswish: "hardswish", F.mish: "mish"}
    for fn, want in callables.items():
        assert activation_name(fn) == want, fn
    for name in R.ACT_NAMES:
        assert activation_name(name) == name and activation_name(name.upper()) == name
    assert activation_name("swish") == "silu" and activation_name("Swish") == "silu"
    assert activation_name("identity") == "none" and activation_name(None) == "none"
    # every name the table can return has an id, and every id but none's is reachable from a module or a callable
    reached = set(modules.values()) | set(callables.values())
    assert reached == {k for k in ACT if k is not None}


@pytest.mark.parametrize("fn", [nn.Softplus(beta=2), nn.Softplus(threshold=10), nn.LeakyReLU(0.2), nn.ELU(alpha=0.5), "gelu_fast",
                                torch.exp, nn.Softmax(dim=-1)])
def test_activation_name_rejects_what_has_no_kernel(fn):
    from gaot_3d_amd.model.layers.mlp import activation_name
    with pytest.raises(NotImplementedError):
        activation_name(fn)
