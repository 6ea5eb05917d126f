"""CPU: the streamed field Jacobian on ROW lists is in place -- gaot_gno_fwd_jac (the tangent kernel on the ragged by-query list of a
'radius' / 'bidirectional' graph) and its workspace function are declared in the header, bound in _lib.SIGNATURES with the header's
argument counts and exported by the library, with the ABI still version 11; ops.gno_forward_jac and IntegralTransform.jacobian_rows
exist; both sample_jacobian methods take ``row_lists``; the closed-form reference the GPU tests compare against
(tests/gno_rows_jac_ref.py) is torch.autograd through the oracle's integral transform in fp64, on a ragged list with empty rows; and
the tangent of the softmax scale weights (magno._softmax_weight_tangents) is fp64 autograd of softmax(mlp(q)) . outs."""
import inspect
import math
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gaot_oracle as orc  # noqa: E402  (checker only)
import gno_rows_jac_ref as REF  # noqa: E402

NAMES = {"gaot_gno_fwd_jac_workspace_bytes": 1, "gaot_gno_fwd_jac": 16}      # arguments in the header


@pytest.mark.parametrize("name", list(NAMES))
def test_row_jacobian_symbols_declared_bound_and_exported(name):
    from gaot_3d_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gaot3d_hip.h")).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
    assert m, f"{name} is not declared in include/gaot3d_hip.h"
    assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == NAMES[name], f"{name}: header and SIGNATURES disagree"
    lib = _lib.load()
    assert hasattr(lib, name), f"{name} is not exported by libgaot3d_hip.so"
    assert lib.gaot_abi_version() == 11


def test_workspace_is_one_kib_per_tile():
    from gaot_3d_amd import _lib
    lib = _lib.load()
    for e, tiles in ((1, 1), (32, 1), (33, 2), (36000, 1125)):
        assert lib.gaot_gno_fwd_jac_workspace_bytes(e) == 1024 * tiles, e


def test_host_layers_exist():
    from gaot_3d_amd import ops
    from gaot_3d_amd.model.gaot_3d import GAOT3D
    from gaot_3d_amd.model.layers.integral_transform import IntegralTransform
    from gaot_3d_amd.model.layers.magno import MAGNODecoder
    assert callable(ops.gno_forward_jac)
    assert list(inspect.signature(ops.gno_forward_jac).parameters) == ["mode", "weights", "biases", "y_pos", "x_pos", "f_y", "src_table",
                                                                        "g"]
    assert callable(IntegralTransform.jacobian_rows)
    assert list(inspect.signature(IntegralTransform.jacobian_rows).parameters) == ["self", "y_pos", "x_pos", "f_y", "graph"]
    from gaot_3d_amd import graph
    assert inspect.signature(graph.query_lists).parameters["lead"].default == 0
    for cls in (MAGNODecoder, GAOT3D):
        par = inspect.signature(cls.sample_jacobian).parameters
        assert "row_lists" in par and par["row_lists"].default is False, cls


DEGREES = [0, 3, 1, 0, 0, 7, 2, 40, 1, 0]        # empty rows first, in the middle and last; one row longer than a 32-edge tile


@pytest.mark.parametrize("mode", ["linear", "nonlinear", "nonlinear_kernelonly"])
def test_reference_is_autograd_through_the_oracle(mode):
    """both sides are fp64 evaluations of the same expression: one summed-channel backward per channel through the oracle"""
    nsrc, nh = 23, 2
    nq = len(DEGREES)
    gen = torch.Generator().manual_seed(40 + len(mode))
    cin = 0 if mode == "linear" else 32
    dims = [6 + cin] + [64] * nh + [32]
    ws = [torch.randn(dims[i + 1], dims[i], generator=gen, dtype=torch.float64) / math.sqrt(dims[i]) for i in range(len(dims) - 1)]
    bs = [0.1 * torch.randn(dims[i + 1], generator=gen, dtype=torch.float64) for i in range(len(dims) - 1)]
    y = torch.rand(nsrc, 3, generator=gen, dtype=torch.float64) * 2 - 1
    x = torch.rand(nq, 3, generator=gen, dtype=torch.float64) * 2 - 1
    f = torch.randn(nsrc, 32, generator=gen, dtype=torch.float64)
    src, dst, rowptr = REF.ragged_list(DEGREES, nsrc, gen)
    out, jac = REF.gno_rows_jac(ws, bs, y, x, src, dst, rowptr, f, mode)
    assert out.shape == (nq, 32) and jac.shape == (3, nq, 32) and out.dtype == jac.dtype == torch.float64
    empty = torch.tensor(DEGREES) == 0
    assert torch.equal(out[empty], torch.zeros_like(out[empty])) and torch.equal(jac[:, empty], torch.zeros_like(jac[:, empty]))
    sd = {}
    for l, (w, b) in enumerate(zip(ws, bs)):
        sd[f"channel_mlp.fcs.{l}.weight"] = w
        sd[f"channel_mlp.fcs.{l}.bias"] = b
    xg = x.clone().requires_grad_(True)
    o = orc.integral_transform(sd, "", y, xg, torch.stack([src.long(), dst.long()]), f, mode, False, 3)
    assert torch.allclose(out, o.detach(), rtol=1e-10, atol=1e-12), (out - o.detach()).abs().max().item()
    ref = torch.stack([torch.autograd.grad(o[:, c].sum(), xg, retain_graph=True)[0] for c in range(32)], dim=-1)   # [Nq, 3, C]
    ref = ref.permute(1, 0, 2)
    assert jac[:, ~empty].abs().min(dim=0).values.max() > 0
    assert torch.allclose(jac, ref, rtol=1e-10, atol=1e-12), (jac - ref).abs().max().item()


@pytest.mark.parametrize("ns", [2, 3])
def test_mix_weight_tangent_is_autograd_of_the_softmax_mix(ns):
    """d/dq [ sum_s softmax(mlp(q))_s out_s(q) ] = sum_s w_s d out_s + sum_s (d w_s) out_s with d w from _softmax_weight_tangents,
    against fp64 autograd; out_s(q) is a smooth function of q with a known Jacobian"""
    from gaot_3d_amd.model.layers.magno import _softmax_weight_tangents
    n, c = 50, 5
    gen = torch.Generator().manual_seed(ns)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)
    w1, b1, w2, b2 = rnd(16, 3), rnd(16), rnd(ns, 16), rnd(ns)
    a = [rnd(c, 3) for _ in range(ns)]                     # out_s(q) = sin(q A_s^T): d out_s / d q_d = cos(q A_s^T) * A_s[:, d]
    q = rnd(n, 3).requires_grad_(True)

    def mixed(qq):
        z = qq @ w1.t() + b1
        w = torch.softmax(torch.relu(z) @ w2.t() + b2, dim=1)
        return sum(w[:, s:s + 1] * torch.sin(qq @ a[s].t()) for s in range(ns)), z, w
    m, z, w = mixed(q)
    ref = torch.stack([torch.autograd.grad(m[:, o].sum(), q, retain_graph=True)[0] for o in range(c)], dim=1)      # [n, c, 3]
    qd = q.detach()
    outs = [torch.sin(qd @ a[s].t()) for s in range(ns)]
    dws = _softmax_weight_tangents(w.detach(), (z.detach() > 0).double(), w1, w2, lambda x, wt: x @ wt.t())
    assert len(dws) == 3 and dws[0].shape == (n, ns)
    for d in range(3):
        assert dws[d].sum(1).abs().max() < 1e-12                                  # the weights sum to one
        got = sum(w.detach()[:, s:s + 1] * torch.cos(qd @ a[s].t()) * a[s][:, d] + dws[d][:, s:s + 1] * outs[s] for s in range(ns))
        assert dws[d].abs().max() > 1e-3
        assert torch.allclose(got, ref[:, :, d], rtol=1e-10, atol=1e-12), (got - ref[:, :, d]).abs().max().item()
