"""CPU: the second derivatives of the sampled field on ROW lists are in place -- gaot_gno_fwd_jet2 (the directional 2-jet kernel on the
ragged by-query list of a 'radius' / 'bidirectional' graph) and its workspace function are declared in the header, bound in
_lib.SIGNATURES with the header's argument counts and exported by the library, with the ABI still version 11; the workspace is
256 (1 + 2 nd) bytes per 32-edge tile; the host layers exist with their signatures; the twelve row jet kernels of the built library
use no scratch and carry a name of their own; the closed-form reference the GPU tests compare against (tests/gno_rows_jet2_ref.py)
equals fp64 autograd DOUBLE backward through the oracle's integral transform on a ragged list with empty rows; the scale mix with the
first and second derivative of its softmax weights (magno._mix_jet2_planes) equals fp64 autograd differentiated twice; and the argument
rules that need no device raise on the host."""
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
import gno_rows_jac_ref as JREF  # noqa: E402
import gno_rows_jet2_ref as REF  # noqa: E402
import test_field_hessian_cpu as hc  # noqa: E402  (_kernel_scratch_sizes, _autograd_hessian, the CPU model)
import test_field_jacobian_rows_cpu as jrc  # noqa: E402  (DEGREES)

NAMES = {"gaot_gno_fwd_jet2_workspace_bytes": 2, "gaot_gno_fwd_jet2": 19}      # arguments in the header
MODES = ("linear", "nonlinear", "nonlinear_kernelonly")
ROW_JET_KERNELS = 12                                                           # 1..4 hidden layers x three modes: no depth is refused
GENERIC = ((0.3, -1.7, 0.9), (-2.1, 0.4, 0.6), (0.8, 0.5, -1.3), (1.9, 1.1, 0.2), (-0.4, -0.6, -2.2), (0.05, 2.4, -0.7))


@pytest.mark.parametrize("name", list(NAMES))
def test_row_jet_symbols_declared_bound_and_exported(name):
    from gaot_3d_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gaot3d_hip.h")).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
    assert m, f"{name} is not declared in include/gaot3d_hip.h"
    assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == NAMES[name], f"{name}: header and SIGNATURES disagree"
    lib = _lib.load()
    assert hasattr(lib, name), f"{name} is not exported by libgaot3d_hip.so"
    assert lib.gaot_abi_version() == 11


def test_workspace_is_256_bytes_per_tile_and_plane():
    from gaot_3d_amd import _lib
    lib = _lib.load()
    for e, tiles in ((1, 1), (32, 1), (33, 2), (36000, 1125)):
        for nd in (1, 3, 6):
            assert lib.gaot_gno_fwd_jet2_workspace_bytes(e, nd) == 256 * (1 + 2 * nd) * tiles, (e, nd)
    assert lib.gaot_gno_fwd_jet2_workspace_bytes(0, 6) == 0


def test_host_layers_exist_with_their_signatures():
    from gaot_3d_amd import ops
    from gaot_3d_amd.model.gaot_3d import GAOT3D
    from gaot_3d_amd.model.layers.integral_transform import IntegralTransform
    from gaot_3d_amd.model.layers.magno import MAGNODecoder
    names = lambda fn: list(inspect.signature(fn).parameters)
    assert names(ops.gno_forward_jet2) == ["mode", "weights", "biases", "y_pos", "x_pos", "f_y", "src_table", "g", "dirs"]
    assert names(IntegralTransform.jet2_rows) == ["self", "y_pos", "x_pos", "f_y", "graph", "dirs"]
    for fn in (MAGNODecoder.sample_hessian_rows, MAGNODecoder.sample_laplacian_rows):
        assert names(fn) == ["self", "rndata_flat", "query_pos", "latent_tokens_pos", "chunk_points"]
        assert inspect.signature(fn).parameters["chunk_points"].default is None
    for fn in (GAOT3D.sample_hessian_rows, GAOT3D.sample_laplacian_rows):
        assert names(fn) == ["self", "latent", "query_pos", "tokens_pos", "chunk_points"]
        assert inspect.signature(fn).parameters["tokens_pos"].default is None


def test_row_jet_kernels_have_no_scratch_and_a_name_of_their_own():
    """the hard condition of the jet kernels on the library as built, for every instantiation that ships; and the regular-list
    kernels are still the only ones whose name contains theirs"""
    from gaot_3d_amd import _lib
    lib = _lib.load()
    sizes = hc._kernel_scratch_sizes(lib._name)
    rows = {k: v for k, v in sizes.items() if "k_gno_fwd_rows_jet2" in k}
    knn = {k: v for k, v in sizes.items() if "k_gno_fwd_knn_jet2" in k}
    fix = {k: v for k, v in sizes.items() if "k_jet2_rows_fixup" in k}
    assert len(rows) == ROW_JET_KERNELS and len(knn) == 12 and len(fix) == 1, (sorted(rows), sorted(knn), sorted(fix))
    assert not set(rows) & set(knn)
    assert not any(rows.values()) and not any(knn.values()) and not any(fix.values()), {k: v for k, v in {**rows, **knn, **fix}.items() if v}
    assert len({k: v for k, v in sizes.items() if "k_mlp2_jet2" in k}) == 9


DEGREES = jrc.DEGREES
assert DEGREES == [0, 3, 1, 0, 0, 7, 2, 40, 1, 0]


@pytest.mark.parametrize("mode", MODES)
def test_ragged_reference_is_double_backward_through_the_oracle(mode):
    """both sides are fp64 evaluations of the same expression; generic directions: D_v = J v, D_v^2 = v^T H v"""
    nsrc, nh = 23, 2
    nq = len(DEGREES)
    gen = torch.Generator().manual_seed(60 + len(mode))
    cin = 0 if mode == "linear" else 32
    dims = [6 + cin] + [64] * nh + [32]
    ws = [torch.randn(dims[i + 1], dims[i], generator=gen, dtype=torch.float64) / math.sqrt(dims[i]) for i in range(len(dims) - 1)]
    bs = [0.1 * torch.randn(dims[i + 1], generator=gen, dtype=torch.float64) for i in range(len(dims) - 1)]
    y = torch.rand(nsrc, 3, generator=gen, dtype=torch.float64) * 2 - 1
    x = torch.rand(nq, 3, generator=gen, dtype=torch.float64) * 2 - 1
    f = torch.randn(nsrc, 32, generator=gen, dtype=torch.float64)
    src, dst, rowptr = JREF.ragged_list(DEGREES, nsrc, gen)
    out, d1, d2 = REF.gno_rows_jet2(ws, bs, y, x, src, dst, rowptr, f, mode, GENERIC)
    assert out.shape == (nq, 32) and d1.shape == d2.shape == (6, nq, 32) and out.dtype == d1.dtype == d2.dtype == torch.float64
    empty = torch.tensor(DEGREES) == 0
    for plane in (out[empty], d1[:, empty], d2[:, empty]):
        assert torch.equal(plane, torch.zeros_like(plane))
    sd = {}
    for l, (w, b) in enumerate(zip(ws, bs)):
        sd[f"channel_mlp.fcs.{l}.weight"] = w
        sd[f"channel_mlp.fcs.{l}.bias"] = b
    ei = torch.stack([src.long(), dst.long()])
    o, jac, hess = hc._autograd_hessian(lambda xx: orc.integral_transform(sd, "", y, xx, ei, f, mode, False, 3), x)
    close = lambda a, b: torch.allclose(a, b, rtol=1e-10, atol=1e-12)
    assert close(out, o), (out - o).abs().max().item()
    assert hess[~empty].abs().amax(dim=(1, 2, 3)).min() > 0
    v = torch.tensor(GENERIC, dtype=torch.float64)
    for n in range(6):
        assert close(d1[n], jac @ v[n]), (n, (d1[n] - jac @ v[n]).abs().max().item())
        want = torch.einsum("i,qcij,j->qc", v[n], hess, v[n])
        assert close(d2[n], want), (n, (d2[n] - want).abs().max().item())
    # and on a regular list the ragged reference is the regular one
    k = 4
    rs, rd, rp = JREF.ragged_list([k] * nq, nsrc, gen)
    a = REF.gno_rows_jet2(ws, bs, y, x, rs, rd, rp, f, mode, GENERIC)
    b = KREF.gno_knn_jet2(ws, bs, y, x, rs, k, f, mode, GENERIC)
    for p, r in zip(a, b):
        assert close(p, r)


@pytest.mark.parametrize("ns", [2, 3])
def test_mix_weight_jets_are_autograd_of_the_softmax_mix_twice(ns):
    """D_v and D_v^2 of sum_s softmax(mlp(q))_s out_s(q), out_s = sin(q A_s^T), from _mix_jet2_planes against fp64 autograd
    differentiated twice, along HESSIAN_DIRS.  The logits are piecewise linear: queries stay 1e-3 clear of the ReLU kinks."""
    from gaot_3d_amd.model.layers.magno import MAGNODecoder, _logit_tangents, _mix_jet2_planes, _softmax_weight_tangents
    dirs = MAGNODecoder.HESSIAN_DIRS
    assert dirs == KREF.HESSIAN_DIRS
    n, c = 50, 5
    gen = torch.Generator().manual_seed(ns)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)
    w1, b1, w2, b2 = rnd(16, 3), rnd(16), rnd(ns, 16), rnd(ns)
    a = [rnd(c, 3) for _ in range(ns)]
    q = rnd(n, 3)
    assert ((q @ w1.t() + b1).abs().amin(1) >= 1e-3).all(), "a query of this seed lies on a ReLU kink: choose another seed"

    def mixed(qq):
        w = torch.softmax(torch.relu(qq @ w1.t() + b1) @ w2.t() + b2, dim=1)
        return sum(w[:, s:s + 1] * torch.sin(qq @ a[s].t()) for s in range(ns))
    _, jac, hess = hc._autograd_hessian(mixed, q)                                       # [n, c, 3], [n, c, 3, 3]
    z = q @ w1.t() + b1
    w = torch.softmax(torch.relu(z) @ w2.t() + b2, dim=1)
    active = (z > 0).double()
    mm = lambda x, wt: x @ wt.t()
    dls = _logit_tangents(active, w1, w2, mm)
    v = torch.tensor(dirs, dtype=torch.float64)
    outs = [torch.sin(q @ a[s].t()) for s in range(ns)]
    av = [v @ a[s].t() for s in range(ns)]                                               # [nd, c]: d/dt (q + t v) A_s^T
    d1s = [torch.cos(q @ a[s].t())[None] * av[s][:, None, :] for s in range(ns)]        # [nd, n, c]
    d2s = [-torch.sin(q @ a[s].t())[None] * av[s][:, None, :] ** 2 for s in range(ns)]
    p1, p2, dws, ddws = _mix_jet2_planes(w, dls, outs, d1s, d2s, dirs)
    assert len(p1) == len(p2) == len(dws) == len(ddws) == 6
    axis = _softmax_weight_tangents(w, active, w1, w2, mm)
    for d in range(3):                                                                   # the axis directions: the Jacobian's weight tangents
        assert torch.equal(dws[d], axis[d])
    for i in range(6):
        assert dws[i].sum(1).abs().max() < 1e-12 and ddws[i].sum(1).abs().max() < 1e-12  # the weights sum to one
        want1 = jac @ v[i]
        want2 = torch.einsum("i,qcij,j->qc", v[i], hess, v[i])
        assert torch.allclose(p1[i], want1, rtol=1e-10, atol=1e-12), (i, (p1[i] - want1).abs().max().item())
        assert torch.allclose(p2[i], want2, rtol=1e-10, atol=1e-12), (i, (p2[i] - want2).abs().max().item())
    assert max(x.abs().max().item() for x in ddws) > 1e-3                                # the second-order weight term is not negligible


@pytest.mark.parametrize("method", ["sample_hessian_rows", "sample_laplacian_rows"])
def test_argument_rules_raise_on_the_host(method):
    with pytest.raises(ValueError, match="reverse"):
        getattr(hc._model(["knn", "reverse"]), method)(torch.zeros(64, 32), torch.zeros(5, 3))
    for strategy in (["knn", "radius"], "bidirectional"):
        model = hc._model(strategy)
        with pytest.raises(ValueError, match="ONE sample"):
            getattr(model, method)(torch.zeros(128, 32), torch.zeros(5, 3))
        with pytest.raises(ValueError, match="chunk_points"):
            getattr(model, method)(torch.zeros(64, 32), torch.zeros(5, 3), chunk_points=0)
        model.decoder.gno.use_attn = True
        with pytest.raises(NotImplementedError, match="use_attn"):
            getattr(model, method)(torch.zeros(64, 32), torch.zeros(5, 3))
