"""The bf16 GNO forward / backward (csrc/gno_bf16.hip, csrc/gno_bwd3_bf16.hip) and the fused projection MLP (csrc/mlp2.hip) against
the fp64 rounding model of tests/gno_ref.py, tensor by tensor.

One rule for every tensor (Report.model, tests/block_ref.py): with R the rounding model and E the exact form, both in fp64,
    rms(got - R) <= 1/4 rms(R - E)   and   max|got - R| <= 2 max|R - E|,   exact zeros where R = E = 0.
The yardstick R - E is the model's own bf16 error; the margins come from the fp32 realisations of the model, which sit at least
12x (rms) and 1.5x (max) below the yardstick on every case used here (tests/test_gno_ref_cpu.py for the small cases, the table in
profiles/gno_bf16_fp64_parity.txt for the large ones; the achieved GPU ratios are recorded there as well).  What the rule rejects
and what it cannot see: tests/test_gno_ref_cpu.py.

Cases: edge counts around the backward's 16-edge tile and 128-edge workgroup pass and the forward's 32-edge tile and 64-edge macro
tile; one forward workgroup pass (12 waves x 64 edges) minus / plus one; the mid-size graph of tests/test_gno_gpu.py; the steady
state -- E = 400 003 takes the forward (256 workgroups x 768 edges) into a third, ragged pass and the backward (256 x 128) into
its thirteenth, with idle prefetches, rows that run through the tiles of several workgroups and, at NH = 4, the operand images in
global memory -- and E = 70 001, the backward's third pass with part of the grid idle."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_ref as B  # noqa: E402
import gno_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _check_gno(kind, e, nh, forward=True):
    from gaot_3d_amd import ops
    c = G.gno_case(kind, e, nh)
    ws, bs = [w.to(DEV) for w in c["ws"]], [b.to(DEV) for b in c["bs"]]
    y, x, f, gout = (c[k].to(DEV) for k in ("y", "x", "f", "gout"))
    g = ops.build_graph(c["ei"].to(DEV), c["n_src"], c["n_dst"])
    got = {}
    if forward:
        got["out"] = ops.gno_forward(ws, bs, y, x, f, g, precision=1)
    runs = {"": ops.gno_backward(ws, bs, y, x, f, gout, g, precision=1),
            "/coords": ops.gno_backward(ws, bs, y, x, f, gout, g, precision=1, coords=True)}
    torch.cuda.synchronize()
    for sfx, run in runs.items():
        got["grad_f" + sfx] = run[0]
        for l in range(nh + 1):
            got[f"dW{l}{sfx}"], got[f"db{l}{sfx}"] = run[1][l], run[2][l]
    got["grad_y"], got["grad_x"] = runs["/coords"][3], runs["/coords"][4]
    r, ex = G.gno_forms(c, "R", device=DEV), G.gno_forms(c, "E", device=DEV)
    rep = B.Report(c["tag"])
    for name, t in got.items():
        base = name.split("/")[0]
        rep.model(name, t, r[base], ex[base])
    rep.done()


@pytest.mark.parametrize("nh", G.NHS)
@pytest.mark.parametrize("e", G.TAIL_E)
def test_gno_bf16_tails(e, nh):
    _check_gno("tail", e, nh)


@pytest.mark.parametrize("e", G.FWD_PASS_E)
def test_gno_bf16_forward_workgroup_pass(e):
    _check_gno("mid", e, 3)


@pytest.mark.parametrize("nh", G.NHS)
def test_gno_bf16_mid_size(nh):
    _check_gno("mid", 20011, nh)


@pytest.mark.parametrize("kind,e,nh", G.LARGE_GNO, ids=lambda v: str(v))
def test_gno_bf16_steady_state(kind, e, nh):
    """E = 400 003: forward and backward; E = 70 001: the backward alone (its third pass, 35 of 256 workgroups active)"""
    _check_gno(kind, e, nh, forward=(kind == "steady"))


@pytest.mark.parametrize("nh", [1, 4])
def test_gno_bf16_empty_graph(nh):
    from gaot_3d_amd import ops
    c = G.gno_case("tail", 0, nh)
    ws, bs = [w.to(DEV) for w in c["ws"]], [b.to(DEV) for b in c["bs"]]
    y, x, f, gout = (c[k].to(DEV) for k in ("y", "x", "f", "gout"))
    g = ops.build_graph(c["ei"].to(DEV), c["n_src"], c["n_dst"])
    out = ops.gno_forward(ws, bs, y, x, f, g, precision=1)
    a = ops.gno_backward(ws, bs, y, x, f, gout, g, precision=1)
    b = ops.gno_backward(ws, bs, y, x, f, gout, g, precision=1, coords=True)
    torch.cuda.synchronize()
    r = G.gno_forms(c, "R", device=DEV)
    rep = B.Report(c["tag"])
    rep.model("out", out, r["out"], r["out"])
    for sfx, run in (("", a), ("/coords", b)):
        rep.model("grad_f" + sfx, run[0], r["grad_f"], r["grad_f"])
        for l in range(nh + 1):
            rep.model(f"dW{l}{sfx}", run[1][l], r[f"dW{l}"], r[f"dW{l}"])
            rep.model(f"db{l}{sfx}", run[2][l], r[f"db{l}"], r[f"db{l}"])
    rep.model("grad_y", b[3], r["grad_y"], r["grad_y"])
    rep.model("grad_x", b[4], r["grad_x"], r["grad_x"])
    rep.done()
    assert all(float(t.abs().max()) == 0.0 for t in r.values())


# the smallest row counts at which a workgroup takes a second 128-row tile: one row past 128 x the grid cap of the backward
# (MLP_BWD_GRID = 256) and of the forward (fwd_oc: 2048) -- G.LARGE_MLP
@pytest.mark.parametrize("rows,hidden,oc,with_b2", G.SMALL_MLP + G.LARGE_MLP, ids=lambda v: str(v))
def test_mlp2_bf16(rows, hidden, oc, with_b2):
    from gaot_3d_amd import ops
    c = G.mlp_case(rows, hidden, oc, with_b2)
    x, w1, b1, w2, dout = (c[k].to(DEV) for k in ("x", "w1", "b1", "w2", "dout"))
    b2 = c["b2"].to(DEV) if with_b2 else None
    got = {"out": ops.mlp2_forward(x, w1, b1, w2, b2)}
    got["dx"], got["dW1"], got["db1"], got["dW2"] = ops.mlp2_backward(x, w1, b1, w2, dout)
    torch.cuda.synchronize()
    r, ex = G.mlp_forms(c, "R", device=DEV), G.mlp_forms(c, "E", device=DEV)
    rep = B.Report(c["tag"])
    for name, t in got.items():
        rep.model(name, t, r[name], ex[name])
    rep.done()
