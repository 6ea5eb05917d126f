"""CPU: directional derivatives of the sampled field along PER-QUERY directions are in place -- gaot_gno_fwd_knn_jet2_qd and
gaot_gno_fwd_jet2_qd are declared in the header, bound in _lib.SIGNATURES with the header's argument counts and exported by the
library, with the ABI still version 11; the 24 per-query jet kernels of the built library (1..4 hidden layers x three modes x both
list kinds) use no scratch and carry names of their own; the host layers exist with their signatures; the closed-form references the
GPU tests compare against (tests/gno_qdir_jet2_ref.py) equal the host-direction references when every query carries the same
directions and agree to 1e-9 with fp64 autograd of t -> out(x_q + t v_q) differentiated once and twice at t = 0; the scale mix along
per-row directions (magno._mix_jet2_planes with a direction tensor) equals fp64 autograd differentiated twice and reproduces the
host-direction mix bit for bit when the rows' directions are equal; and a bad ``dirs`` raises ValueError on the host."""
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
import gno_jet2_ref as KREF  # noqa: E402
import gno_qdir_jet2_ref as REF  # noqa: E402
import gno_rows_jac_ref as JREF  # noqa: E402
import gno_rows_jet2_ref as RREF  # noqa: E402
import test_field_hessian_cpu as hc  # noqa: E402  (_kernel_scratch_sizes, _autograd_hessian, the CPU model)

NAMES = {"gaot_gno_fwd_knn_jet2_qd": 15, "gaot_gno_fwd_jet2_qd": 19}           # arguments in the header
MODES = ("linear", "nonlinear", "nonlinear_kernelonly")
GENERIC = ((0.3, -1.7, 0.9), (-2.1, 0.4, 0.6), (0.8, 0.5, -1.3), (1.9, 1.1, 0.2), (-0.4, -0.6, -2.2), (0.05, 2.4, -0.7))


@pytest.mark.parametrize("name", list(NAMES))
def test_per_query_jet_symbols_declared_bound_and_exported(name):
    from gaot_3d_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gaot3d_hip.h")).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
    assert m, f"{name} is not declared in include/gaot3d_hip.h"
    assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == NAMES[name], f"{name}: header and SIGNATURES disagree"
    host = name[:-3]                                   # the host-direction entry point: the same argument list
    assert _lib.SIGNATURES[name] == _lib.SIGNATURES[host]
    lib = _lib.load()
    assert hasattr(lib, name), f"{name} is not exported by libgaot3d_hip.so"
    assert lib.gaot_abi_version() == 11


def test_per_query_jet_kernels_have_no_scratch_and_names_of_their_own():
    """the hard condition of the jet kernels on the library as built, for all 24 instantiations; the host-direction kernels are
    still the only ones whose name contains theirs"""
    from gaot_3d_amd import _lib
    lib = _lib.load()
    sizes = hc._kernel_scratch_sizes(lib._name)
    knn = {k: v for k, v in sizes.items() if "k_gno_qd_jet2_knn" in k}
    rows = {k: v for k, v in sizes.items() if "k_gno_qd_jet2_rows" in k}
    assert len(knn) == 12 and len(rows) == 12, (sorted(knn), sorted(rows))
    assert not any(knn.values()) and not any(rows.values()), {k: v for k, v in {**knn, **rows}.items() if v}
    host = {k for k in sizes if "k_gno_fwd_knn_jet2" in k or "k_gno_fwd_rows_jet2" in k}
    assert len(host) == 24 and not host & (set(knn) | set(rows))


def test_host_layers_exist_with_their_signatures():
    from gaot_3d_amd import ops
    from gaot_3d_amd.model.gaot_3d import GAOT3D
    from gaot_3d_amd.model.layers.integral_transform import IntegralTransform
    from gaot_3d_amd.model.layers.magno import MAGNODecoder
    names = lambda fn: list(inspect.signature(fn).parameters)
    assert names(ops.gno_forward_knn_jet2_qd) == ["mode", "weights", "biases", "y_pos", "x_pos", "f_y", "src_table", "nbr", "k", "qdirs"]
    assert names(ops.gno_forward_jet2_qd) == ["mode", "weights", "biases", "y_pos", "x_pos", "f_y", "src_table", "g", "qdirs"]
    assert names(IntegralTransform.jet2_knn_qd) == ["self", "y_pos", "x_pos", "nbr", "k", "f_y", "qdirs"]
    assert names(IntegralTransform.jet2_rows_qd) == ["self", "y_pos", "x_pos", "f_y", "graph", "qdirs"]
    assert names(MAGNODecoder.sample_directional) == ["self", "rndata_flat", "query_pos", "dirs", "latent_tokens_pos", "chunk_points"]
    assert names(GAOT3D.sample_directional) == ["self", "latent", "query_pos", "dirs", "tokens_pos", "chunk_points"]
    for p in ("tokens_pos", "chunk_points"):
        assert inspect.signature(GAOT3D.sample_directional).parameters[p].default is None


# ---- the references -----------------------------------------------------------------------------------------------------------------------
def _operands(nh, mode, nsrc, nq, seed):
    gen = torch.Generator().manual_seed(seed)
    cin = 0 if mode == "linear" else 32
    dims = [6 + cin] + [64] * nh + [32]
    ws = [torch.randn(dims[i + 1], dims[i], generator=gen, dtype=torch.float64) / math.sqrt(dims[i]) for i in range(len(dims) - 1)]
    bs = [0.1 * torch.randn(dims[i + 1], generator=gen, dtype=torch.float64) for i in range(len(dims) - 1)]
    y = torch.rand(nsrc, 3, generator=gen, dtype=torch.float64) * 2 - 1
    x = torch.rand(nq, 3, generator=gen, dtype=torch.float64) * 2 - 1
    f = torch.randn(nsrc, 32, generator=gen, dtype=torch.float64)
    return gen, ws, bs, y, x, f


def _along_t(fn, x, v):
    """fn: x [N, 3] -> [N, C] row by row; v [N, 3].  -> (d/dt, d^2/dt^2) of fn(x + t v) at t = 0, one t per row, by fp64 autograd
    through the graph of the first derivative: [N, C] each"""
    t = torch.zeros(x.shape[0], dtype=x.dtype, requires_grad=True)
    o = fn(x + t[:, None] * v)
    d1, d2 = torch.zeros_like(o), torch.zeros_like(o)
    for c in range(o.shape[1]):
        (g,) = torch.autograd.grad(o[:, c].sum(), t, create_graph=True)
        d1[:, c] = g.detach()
        (gg,) = torch.autograd.grad(g.sum(), t, retain_graph=True)
        d2[:, c] = gg
    return d1.detach(), d2.detach()


RAGGED = [3, 0, 7, 1, 4]                              # Nq = 5: an empty row, a single edge


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nh", [1, 3])
def test_references_are_autograd_along_each_querys_own_direction(nh, mode):
    nq, nsrc, k, nd = 5, 23, 4, 2
    gen, ws, bs, y, x, f = _operands(nh, mode, nsrc, nq, 70 * nh + len(mode))
    v = torch.randn(nq, nd, 3, generator=gen, dtype=torch.float64) * 1.3       # neither axis-aligned nor unit, different per query
    sd = {}
    for l, (w, b) in enumerate(zip(ws, bs)):
        sd[f"channel_mlp.fcs.{l}.weight"] = w
        sd[f"channel_mlp.fcs.{l}.bias"] = b
    close = lambda a, b: torch.allclose(a, b, rtol=1e-9, atol=1e-9 * float(b.abs().max()))
    nbr = torch.randint(0, nsrc, (nq * k,), generator=gen, dtype=torch.int32)
    rs, rd, rp = JREF.ragged_list(RAGGED, nsrc, gen)
    lists = {"knn": (torch.stack([nbr.long(), torch.arange(nq).repeat_interleave(k)]),
                     REF.gno_knn_jet2_qd(ws, bs, y, x, nbr, k, f, mode, v)),
             "rows": (torch.stack([rs.long(), rd.long()]), REF.gno_rows_jet2_qd(ws, bs, y, x, rs, rd, rp, f, mode, v))}
    for kind, (ei, (out, d1, d2)) in lists.items():
        assert out.shape == (nq, 32) and d1.shape == d2.shape == (nd, nq, 32) and d2.dtype == torch.float64
        fn = lambda xx: orc.integral_transform(sd, "", y, xx, ei, f, mode, False, 3)
        assert close(out, fn(x)), kind
        for i in range(nd):
            a1, a2 = _along_t(fn, x, v[:, i])
            assert a2.abs().max() > 0
            assert close(d1[i], a1), (kind, i, (d1[i] - a1).abs().max().item())
            assert close(d2[i], a2), (kind, i, (d2[i] - a2).abs().max().item())
    empty = torch.tensor(RAGGED) == 0
    for plane in (lists["rows"][1][0][empty], lists["rows"][1][1][:, empty], lists["rows"][1][2][:, empty]):
        assert torch.equal(plane, torch.zeros_like(plane))


@pytest.mark.parametrize("mode", MODES)
def test_uniform_directions_give_the_host_direction_references(mode):
    nq, nsrc, k = 9, 23, 4
    gen, ws, bs, y, x, f = _operands(2, mode, nsrc, nq, 5 + len(mode))
    uni = torch.tensor(GENERIC, dtype=torch.float64)[None].expand(nq, 6, 3)
    nbr = torch.randint(0, nsrc, (nq * k,), generator=gen, dtype=torch.int32)
    for a, b in zip(REF.gno_knn_jet2_qd(ws, bs, y, x, nbr, k, f, mode, uni), KREF.gno_knn_jet2(ws, bs, y, x, nbr, k, f, mode, GENERIC)):
        assert torch.equal(a, b), (a - b).abs().max().item()
    rs, rd, rp = JREF.ragged_list([3, 0, 7, 1, 4, 0, 40, 2, 1], nsrc, gen)
    for a, b in zip(REF.gno_rows_jet2_qd(ws, bs, y, x, rs, rd, rp, f, mode, uni),
                    RREF.gno_rows_jet2(ws, bs, y, x, rs, rd, rp, f, mode, GENERIC)):
        assert torch.equal(a, b), (a - b).abs().max().item()


# ---- the scale mix along per-row directions ---------------------------------------------------------------------------------------------
def _mix_case(ns=2, n=50, c=5):
    gen = torch.Generator().manual_seed(11 + ns)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)
    w1, b1, w2, b2 = rnd(16, 3), rnd(16), rnd(ns, 16), rnd(ns)
    a = [rnd(c, 3) for _ in range(ns)]
    q = rnd(n, 3)
    assert ((q @ w1.t() + b1).abs().amin(1) >= 1e-3).all(), "a query of this seed lies on a ReLU kink: choose another seed"
    return gen, w1, b1, w2, b2, a, q


def _mix_operands(w1, b1, w2, b2, a, q, v):
    """the weights, the axis tangents of the logits and the scales' planes out_s = sin(q A_s^T) along the per-row directions v [n, nd, 3]"""
    from gaot_3d_amd.model.layers.magno import _logit_tangents
    ns = len(a)
    z = q @ w1.t() + b1
    w = torch.softmax(torch.relu(z) @ w2.t() + b2, dim=1)
    dls = _logit_tangents((z > 0).double(), w1, w2, lambda x, wt: x @ wt.t())
    outs = [torch.sin(q @ a[s].t()) for s in range(ns)]
    av = [torch.einsum("nid,cd->inc", v, a[s]) for s in range(ns)]                     # [nd, n, c]: d/dt (q + t v) A_s^T, per row
    d1s = [torch.cos(q @ a[s].t())[None] * av[s] for s in range(ns)]
    d2s = [-torch.sin(q @ a[s].t())[None] * av[s] ** 2 for s in range(ns)]
    return w, dls, outs, d1s, d2s


def test_mix_along_per_row_directions_is_autograd_twice():
    """two scales with softmax weights: D_v and D_v^2 of sum_s softmax(mlp(q))_s sin(q A_s^T) along a direction of every row's own"""
    from gaot_3d_amd.model.layers.magno import _mix_jet2_planes
    gen, w1, b1, w2, b2, a, q = _mix_case()
    nd = 3
    v = torch.randn(q.shape[0], nd, 3, generator=gen, dtype=torch.float64) * 1.5

    def mixed(qq):
        w = torch.softmax(torch.relu(qq @ w1.t() + b1) @ w2.t() + b2, dim=1)
        return sum(w[:, s:s + 1] * torch.sin(qq @ a[s].t()) for s in range(len(a)))
    p1, p2, dws, ddws = _mix_jet2_planes(*_mix_operands(w1, b1, w2, b2, a, q, v), v)
    assert len(p1) == len(p2) == len(dws) == len(ddws) == nd
    for i in range(nd):
        want1, want2 = _along_t(mixed, q, v[:, i])
        assert dws[i].sum(1).abs().max() < 1e-12 and ddws[i].sum(1).abs().max() < 1e-12  # the weights sum to one
        assert torch.allclose(p1[i], want1, rtol=1e-10, atol=1e-12), (i, (p1[i] - want1).abs().max().item())
        assert torch.allclose(p2[i], want2, rtol=1e-10, atol=1e-12), (i, (p2[i] - want2).abs().max().item())
    assert max(x.abs().max().item() for x in ddws) > 1e-3                                # the second-order weight term is not negligible
    # a first-order call forms nothing of second order
    q1, q2, _, none = _mix_jet2_planes(*_mix_operands(w1, b1, w2, b2, a, q, v)[:4], None, v, second=False)
    assert q2 == [] and all(x is None for x in none) and all(torch.equal(x, y_) for x, y_ in zip(q1, p1))


def test_equal_row_directions_reproduce_the_host_direction_mix():
    """the axes (the host path takes an axis tangent as it is: products with 1 and sums with 0 are exact) bit for bit, in fp32 as the
    model runs it; generic directions to fp64 rounding (the host path multiplies by a Python float, the row path by a column)"""
    from gaot_3d_amd.model.layers.magno import MAGNODecoder, _mix_jet2_planes
    gen, w1, b1, w2, b2, a, q = _mix_case()
    n = q.shape[0]
    axes = MAGNODecoder.HESSIAN_DIRS[:3]
    for dtype in (torch.float64, torch.float32):
        cast = lambda ts: [t.to(dtype) for t in ts]
        va = torch.tensor(axes, dtype=dtype)[None].expand(n, 3, 3).contiguous()
        w, dls, outs, d1s, d2s = _mix_operands(w1, b1, w2, b2, a, q, va.double())
        ops_ = (w.to(dtype), cast(dls), cast(outs), cast(d1s), cast(d2s))
        host = _mix_jet2_planes(*ops_, axes)
        rows = _mix_jet2_planes(*ops_, va)
        for hs, rs in zip(host, rows):
            assert all(torch.equal(h, r) for h, r in zip(hs, rs)), dtype
    vg = torch.tensor(GENERIC, dtype=torch.float64)[None].expand(n, 6, 3).contiguous()
    ops_ = _mix_operands(w1, b1, w2, b2, a, q, vg)
    for hs, rs in zip(_mix_jet2_planes(*ops_, GENERIC), _mix_jet2_planes(*ops_, vg)):
        assert all(torch.allclose(h, r, rtol=1e-12, atol=1e-13) for h, r in zip(hs, rs))


# ---- argument rules ---------------------------------------------------------------------------------------------------------------------
def test_bad_dirs_raise_value_errors_on_the_host():
    lat, q = torch.zeros(64, 32), torch.zeros(5, 3)
    good = torch.zeros(5, 2, 3)
    for strategy in ("knn", ["knn", "radius"], "bidirectional"):
        model = hc._model(strategy)
        for bad, msg in ((torch.zeros(4, 2, 3), "5 queries"), (torch.zeros(5, 0, 3), "nd = 0"), (torch.zeros(5, 7, 3), "nd = 7"),
                         (torch.zeros(5, 2, 2), "3 components"), (torch.zeros(5, 2), "3 components"), (torch.zeros(6, 3), "5 queries"),
                         (torch.zeros(5, 2, 3, 1), "5 queries"), (torch.zeros(5, 2, 3, dtype=torch.float64), "float32"),
                         (torch.zeros(5, 2, 3, device="meta"), "device"), ([[1.0, 0.0, 0.0]] * 5, "tensor")):
            with pytest.raises(ValueError, match=msg):
                model.sample_directional(lat, q, bad)
        with pytest.raises(ValueError, match="ONE sample"):
            model.sample_directional(torch.zeros(128, 32), q, good)
        with pytest.raises(ValueError, match="chunk_points"):
            model.sample_directional(lat, q, good, chunk_points=0)
        model.decoder.gno.use_attn = True
        with pytest.raises(NotImplementedError, match="use_attn"):
            model.sample_directional(lat, q, good)
    with pytest.raises(ValueError, match="reverse"):
        hc._model(["knn", "reverse"]).sample_directional(lat, q, good)
