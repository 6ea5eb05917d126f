"""The bf16 GNO kernels in their 'nonlinear' / 'nonlinear_kernelonly' modes (csrc/gno_bf16.hip, csrc/gno_bwd3_bf16.hip) and the per-node
products around them against the fp64 rounding model of tests/gno_nl_ref.py, tensor by tensor.

One rule for every tensor (Report.model, tests/block_ref.py): with R the rounding model and E the exact form, both in fp64,
    rms(got - R) <= 1/4 rms(R - E)   and   max|got - R| <= 2 max|R - E|,   exact zeros where R = E = 0.
The fp32 realisations of the model sit at least 12x (rms) and 1.5x (max) below the yardstick on every case used here
(tests/test_gno_nl_ref_cpu.py; the table and the achieved GPU ratios: profiles/gno_nl_bf16_fp64_parity.txt).

Tensors: out, grad_f, dt, dW_0c and dW_0f (the two column blocks of dW_0), db_0, every dW_l / db_l, grad_y / grad_x; the backward runs
with and without the coordinate gradients.  The 32-channel cases go through GF.GnoNlFn beside the per-node linear, which exposes dt;
the other shapes (C = 16, C = 64 in two passes, C_in = 40, hidden width 48, coordinate dimension 2) through IntegralTransform.

Cases (tests/gno_nl_ref.py): edge counts around the backward's 16-edge tile and 128-edge workgroup pass and the forward's 32-edge tile
and 64-edge macro tile, with a source row that spans several tiles and, from E = 193, crosses a 128-edge pass (the dt fix-up across
tiles and workgroups) and sources without an edge (exact zero rows); E = 0; one forward workgroup pass -1 / +1; E = 20 011; the steady
state E = 400 003 at NH = 3; NH = 4 (operand images from global memory)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_ref as B  # noqa: E402
import gno_nl_ref as N  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _bf16():
    import gaot_3d_amd
    gaot_3d_amd.set_precision("bf16")
    yield
    gaot_3d_amd.set_precision("fp32")


def run_functional(c, coords):
    """one 32-channel pass as IntegralTransform._forward_fused runs it -> every tensor, dt included"""
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd import ops
    nh = len(c["ws"]) - 1
    ws = [w.to(DEV).requires_grad_() for w in c["ws"]]
    bs = [b.to(DEV).requires_grad_() for b in c["bs"]]
    y, x = (c[k].to(DEV).requires_grad_(coords) for k in ("y", "x"))
    f = c["f"].to(DEV).requires_grad_()
    g = ops.build_graph(c["ei"].to(DEV), c["n_src"], c["n_dst"])
    t = GF.linear(f, ws[0][:, 6:].contiguous(), None, precision=0)
    t.retain_grad()
    params = [ws[0][:, :6].contiguous(), bs[0]]
    for l in range(1, nh + 1):
        params += [ws[l], bs[l]]
    out = GF.GnoNlFn.apply(c["mode"], f if c["mode"] == "nonlinear" else None, t, y, x, g, *params)
    out.backward(c["gout"].to(DEV))
    torch.cuda.synchronize()
    got = {"out": out.detach(), "grad_f": f.grad, "dt": t.grad, "dW0c": ws[0].grad[:, :6], "dW0f": ws[0].grad[:, 6:], "db0": bs[0].grad}
    for l in range(1, nh + 1):
        got[f"dW{l}"], got[f"db{l}"] = ws[l].grad, bs[l].grad
    if coords:
        got["grad_y"], got["grad_x"] = y.grad, x.grad
    return got


def run_module(c, coords):
    """the module itself (padding, passes) -> every tensor but dt"""
    from gaot_3d_amd import ops
    from gaot_3d_amd.model.layers.integral_transform import IntegralTransform
    nh, cd = len(c["ws"]) - 1, c["y"].shape[1]
    layers = [c["ws"][0].shape[1]] + [w.shape[0] for w in c["ws"]]
    it = IntegralTransform(channel_mlp_layers=layers, transform_type=c["mode"])
    with torch.no_grad():
        for fc, w, b in zip(it.channel_mlp.fcs, c["ws"], c["bs"]):
            fc.weight.copy_(w.view_as(fc.weight))
            fc.bias.copy_(b)
    it = it.to(DEV)
    y, x = (c[k].to(DEV).requires_grad_(coords) for k in ("y", "x"))
    f = c["f"].to(DEV).requires_grad_()
    g = ops.build_graph(c["ei"].to(DEV), c["n_src"], c["n_dst"])
    assert it._fused_plan(list(it.channel_mlp.fcs), f, y, x) is not None
    out = it(y, x, None, f_y=f, graph=g)
    out.backward(c["gout"].to(DEV))
    torch.cuda.synchronize()
    fcs = list(it.channel_mlp.fcs)
    w0g = fcs[0].weight.grad.reshape(fcs[0].weight.shape[0], -1)
    got = {"out": out.detach(), "grad_f": f.grad, "dW0c": w0g[:, :2 * cd], "dW0f": w0g[:, 2 * cd:], "db0": fcs[0].bias.grad}
    for l in range(1, nh + 1):
        got[f"dW{l}"], got[f"db{l}"] = fcs[l].weight.grad.reshape(fcs[l].weight.shape[0], -1), fcs[l].bias.grad
    if coords:
        got["grad_y"], got["grad_x"] = y.grad, x.grad
    return got


def check_case(args):
    c = N.nl_case(args[0], args[1], *args[2:])
    run = run_functional if tuple(args[4:]) == (32, 32, 64, 3) else run_module
    r, ex = N.nl_forms(c, "R", device=DEV), N.nl_forms(c, "E", device=DEV)
    rep = B.Report(c["tag"])
    for sfx, coords in (("", False), ("/coords", True)):
        for name, t in run(c, coords).items():
            rep.model(name + sfx, t, r[name], ex[name])
    rep.done()


_ID = lambda a: "-".join(str(v) for v in a)  # noqa: E731


@pytest.mark.parametrize("args", N.small_cases(), ids=_ID)
def test_gno_nl_bf16(args):
    check_case(args)


@pytest.mark.parametrize("args", N.LARGE, ids=_ID)
def test_gno_nl_bf16_steady_state(args):
    """E = 400 003 at NH = 3: the forward's third pass, the backward's thirteenth"""
    check_case(args)


@pytest.mark.parametrize("mode", N.MODES)
@pytest.mark.parametrize("nh", [1, 4])
def test_gno_nl_bf16_empty_graph(mode, nh):
    c = N.nl_case("tail", mode, 0, nh)
    r = N.nl_forms(c, "R", device=DEV)
    rep = B.Report(c["tag"])
    for sfx, coords in (("", False), ("/coords", True)):
        for name, t in run_functional(c, coords).items():
            if t is None and name in ("grad_y", "grad_x", "grad_f"):     # no edge: autograd may hand back no gradient at all
                continue
            rep.model(name + sfx, t, r[name], r[name])
    rep.done()
    assert all(float(t.abs().max()) == 0.0 for t in r.values())
