"""CPU: the adjoint of the field's Laplacian is in place -- gaot_gno_adj_jet2, gaot_gno_adj_jet2_workspace_bytes and
gaot_mlp2_lap_cot_mid are declared in the header, bound in _lib.SIGNATURES with the header's argument counts and exported by the
library (ABI 11); the four k_gno_adj_jet2 instantiations (1..4 hidden layers) exist and use no scratch, the element kernel exists;
the host layers exist with their signatures; the fp64 references the GPU tests compare against (tests/gno_jet2_adj_ref.py) agree with
independent ones -- the closed form against torch.autograd.grad through the row-list jet reference's value / D_v / D_v^2 planes
(row degrees [3, 0, 7, 1, 4, 40, 0], nd in {1, 3, 6}, one second-order cotangent plane per direction or ONE for all) within 1e-10 of
the peak; gelu''' against autograd of gelu''; the projection's elementwise middle against autograd of the projection's jets; and
the decoder-level product written out step by step against the fp64 oracle's decoder (oracle/gaot_oracle.py) differentiated twice
in the query (create_graph=True, per output channel) and then in the latent, within 1e-9 of the peak: regular lists ('knn'), ragged
lists with empty rows ('radius', 'bidirectional'), two softmax-weighted scales on DIFFERENT lists per scale, with and without the
cotangents that may be None; and sample_laplacian_vjp / sample_laplacian_autograd refuse on the host what they refuse."""
import inspect
import os
import re
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gaot_oracle as orc  # noqa: E402  (checker only)
import gno_adj_ref as REF  # noqa: E402
import gno_jac_adj_ref as JA  # noqa: E402
import gno_jet2_adj_ref as LA  # noqa: E402
from gno_jet2_ref import gelu, gelu_d1, gelu_d2  # noqa: E402
import test_field_adjoint_cpu as ac  # noqa: E402  (_operands, _cpu_model, the refusal table)
import test_field_hessian_cpu as hc  # noqa: E402  (_kernel_scratch_sizes)
from gaot_3d_amd.model.layers.magno import MAGNODecoder  # noqa: E402

AXES = MAGNODecoder.LAP_VJP_DIRS                # the directions the decoder's adjoint runs along: the references use the same
assert AXES == LA.AXES
NAMES = {"gaot_gno_adj_jet2_workspace_bytes": 1, "gaot_gno_adj_jet2": 21, "gaot_mlp2_lap_cot_mid": 14}    # arguments in the header
GENERIC = ((0.3, -1.7, 0.9), (-2.1, 0.4, 0.6), (0.8, 0.5, -1.3), (1.9, 1.1, 0.2), (-0.4, -0.6, -2.2), (0.05, 2.4, -0.7))


@pytest.mark.parametrize("name", list(NAMES))
def test_symbols_declared_bound_and_exported(name):
    from gaot_3d_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gaot3d_hip.h")).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
    assert m, f"{name} is not declared in include/gaot3d_hip.h"
    assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == NAMES[name], f"{name}: header and SIGNATURES disagree"
    assert hasattr(_lib.load(), name), f"{name} is not exported by libgaot3d_hip.so"
    assert _lib.load().gaot_abi_version() == 11                                    # additive: the version stays


def test_the_four_kernels_exist_without_scratch_and_the_element_kernel_exists():
    from gaot_3d_amd import _lib
    sizes = hc._kernel_scratch_sizes(_lib.load()._name)
    adj = {k: v for k, v in sizes.items() if "k_gno_adj_jet2" in k}
    assert len(adj) == 4, sorted(adj)
    assert not any(adj.values()), adj
    assert not any(s in k for k in adj for s in ("k_gno_fwd", "AdjFwd", "k_gno_adj_jac", "k_gno_qd"))    # names the older tests count
    mid = {k: v for k, v in sizes.items() if "k_mlp2_lap_cot_mid" in k}
    assert len(mid) == 1 and not any(mid.values()), mid
    assert not any("k_mlp2_jet2" in k for k in mid)


def test_host_layers_exist_with_their_signatures():
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd import ops
    from gaot_3d_amd.model.gaot_3d import GAOT3D
    from gaot_3d_amd.model.layers.integral_transform import IntegralTransform
    from gaot_3d_amd.model.layers.magno import MAGNODecoder
    names = lambda fn: list(inspect.signature(fn).parameters)
    assert names(ops.gno_adjoint_jet2) == ["weights", "biases", "y_pos", "x_pos", "dirs", "grad_out", "grad_d1", "grad_d2", "g", "k"]
    assert inspect.signature(ops.gno_adjoint_jet2).parameters["k"].default is None
    assert names(ops.mlp2_lap_cot_mid) == ["zus", "a", "ad", "al", "b1", "out"]
    assert names(IntegralTransform.adjoint_jet2_knn) == ["self", "y_pos", "x_pos", "nbr", "k", "dirs", "grad_out", "grad_d1", "grad_d2",
                                                         "graph"]
    assert names(IntegralTransform.adjoint_jet2_rows) == ["self", "y_pos", "x_pos", "dirs", "grad_out", "grad_d1", "grad_d2", "graph"]
    assert names(MAGNODecoder._project_lap_vjp) == ["self", "planes", "gy", "gj", "gl"]
    assert names(MAGNODecoder.sample_laplacian_vjp) == ["self", "rndata_flat", "query_pos", "cot_pred", "cot_jac", "cot_lap",
                                                        "latent_tokens_pos", "chunk_points"]
    assert names(GAOT3D.sample_laplacian_vjp) == ["self", "latent", "query_pos", "cot_pred", "cot_jac", "cot_lap", "tokens_pos",
                                                  "chunk_points"]
    assert names(GAOT3D.sample_laplacian_autograd) == ["self", "latent", "query_pos", "tokens_pos", "chunk_points"]
    assert issubclass(GF.SampleLaplacianLatentFn, torch.autograd.Function)
    assert MAGNODecoder.LAP_VJP_DIRS == MAGNODecoder.HESSIAN_DIRS[:3] == LA.AXES


# ---- the references -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["plane_per_direction", "one_plane"])
@pytest.mark.parametrize("nd", [1, 3, 6])
@pytest.mark.parametrize("nh", [1, 4])
def test_closed_form_is_autograd_through_the_jet_reference(nh, nd, shared):
    nsrc = 48                                          # more sources than edges leave: some stay without one
    deg = [3, 0, 7, 1, 4, 40, 0]                       # empty rows, a single edge, a row longer than a tile
    gen, ws, bs, y, x = ac._operands(nh, nsrc, len(deg), 41 + 7 * nh + nd)
    src, dst, rowptr = REF.random_list(deg, nsrc, gen)
    dirs = GENERIC[:nd]
    g = torch.randn(len(deg), 32, generator=gen, dtype=torch.float64)
    p = torch.randn(nd, len(deg), 32, generator=gen, dtype=torch.float64)
    s = torch.randn(1 if shared else nd, len(deg), 32, generator=gen, dtype=torch.float64)
    closed = LA.adjoint_jet2_closed(ws, bs, y, x, src, dst, rowptr, dirs, g, p, s, nsrc)
    auto = LA.adjoint_jet2_autograd(ws, bs, y, x, src, dst, rowptr, dirs, g, p, s, nsrc)
    peak = auto.abs().max()
    assert peak > 0
    assert (auto - closed).abs().max() <= 1e-10 * peak, (auto - closed).abs().max() / peak
    # every term is there: dropping S, or S and P, gives other gradients, and without both it is the value adjoint
    no_s = LA.adjoint_jet2_closed(ws, bs, y, x, src, dst, rowptr, dirs, g, p, torch.zeros_like(s), nsrc)
    value_only = LA.adjoint_jet2_closed(ws, bs, y, x, src, dst, rowptr, dirs, g, torch.zeros_like(p), torch.zeros_like(s), nsrc)
    assert (no_s - closed).abs().max() > 1e-2 * peak and (value_only - no_s).abs().max() > 1e-2 * peak
    assert (value_only - REF.gno_adjoint_closed(ws, bs, y, x, src, dst, rowptr, g, nsrc)).abs().max() <= 1e-13 * peak
    used = torch.zeros(nsrc, dtype=torch.bool)
    used[src.long()] = True
    assert (~used).any() and torch.equal(closed[~used], torch.zeros_like(closed[~used]))     # a source without edges: exact zeros
    # duality: <G, out> + sum_i <P_i, d1_i> + sum_i <S_i, d2_i> = <df, f>
    f = torch.randn(nsrc, 32, generator=gen, dtype=torch.float64)
    out, d1, d2 = LA.gno_rows_jet2(ws, bs, y, x, src, dst, rowptr, f, "linear", dirs)
    lhs = (g * out).sum() + (p * d1).sum() + (s.expand_as(d2) * d2).sum()
    assert abs(lhs - (closed * f).sum()) <= 1e-12 * (closed * f).abs().sum()


def test_along_the_axes_the_first_order_part_is_the_jacobian_adjoint():
    nsrc, deg = 23, [3, 0, 7, 1, 4, 40, 0]
    gen, ws, bs, y, x = ac._operands(2, nsrc, len(deg), 77)
    src, dst, rowptr = REF.random_list(deg, nsrc, gen)
    g = torch.randn(len(deg), 32, generator=gen, dtype=torch.float64)
    p = torch.randn(3, len(deg), 32, generator=gen, dtype=torch.float64)
    got = LA.adjoint_jet2_closed(ws, bs, y, x, src, dst, rowptr, LA.AXES, g, p, torch.zeros(1, len(deg), 32, dtype=torch.float64), nsrc)
    ref = JA.adjoint_jac_closed(ws, bs, y, x, src, dst, rowptr, g, p, nsrc)          # d_d K by autograd there, by recurrence here
    assert ref.abs().max() > 0 and (got - ref).abs().max() <= 1e-11 * ref.abs().max()


def test_gelu_third_derivative_is_autograd_of_the_second():
    z = torch.linspace(-5, 5, 401, dtype=torch.float64, requires_grad=True)
    (d3,) = torch.autograd.grad(gelu_d2(z).sum(), z)
    assert d3.abs().max() > 0.5 and (LA.gelu_d3(z.detach()) - d3).abs().max() <= 1e-14


@pytest.mark.parametrize("with_a", [True, False])
def test_the_projection_middle_is_autograd_of_the_projection_jets(with_a):
    gen = torch.Generator().manual_seed(5)
    n, h = 9, 12
    z, s = (torch.randn(n, h, generator=gen, dtype=torch.float64, requires_grad=True) for _ in range(2))
    u = torch.randn(3, n, h, generator=gen, dtype=torch.float64, requires_grad=True)
    a, al = (torch.randn(n, h, generator=gen, dtype=torch.float64) for _ in range(2))
    ad = torch.randn(3, n, h, generator=gen, dtype=torch.float64)
    # the jets at hidden width: a(z), a'(z) u_d, a''(z) sum_d u_d^2 + a'(z) s, contracted with A, A_d, A_L
    loss = (gelu_d1(z) * u * ad).sum() + ((gelu_d2(z) * (u * u).sum(0) + gelu_d1(z) * s) * al).sum()
    if with_a:
        loss = loss + (gelu(z) * a).sum()
    dz, du, ds = torch.autograd.grad(loss, (z, u, s))
    got = LA.lap_cot_mid(z, u, s, a if with_a else None, ad, al)
    for name, x, ref in (("dz", got[0], dz), ("du", got[1:4], du), ("ds", got[4], ds)):
        assert ref.abs().max() > 0 and (x - ref).abs().max() <= 1e-12 * ref.abs().max(), name


DECODERS = {
    "knn": dict(),
    "radius": dict(),
    "bidirectional_four_channels": dict(out=4),
    "two_scales_weighted_radius": dict(out=2, scales=[1.0, 2.0], use_scale_weights=True),
    "two_scales_summed_radius": dict(scales=[1.0, 2.0], use_scale_weights=False),
    "four_layers_knn": dict(out_gno_channel_mlp_hidden_layers=[64, 64, 64, 64]),
}


def _lists(case, ns, nq, m, gen):
    if case.endswith("knn") or case == "knn":          # every scale sees the same regular list
        one = REF.random_list([8] * nq, m, gen)
        return [one] * ns
    # a list of its own per scale (random rows, empty ones from the second list on and in 'bidirectional')
    lo = lambda s: 0 if s or case.startswith("bidirectional") else 1
    return [REF.random_list(torch.randint(lo(s), 9 + 4 * s, (nq,), generator=gen).tolist(), m, gen) for s in range(ns)]


@pytest.mark.parametrize("cots", ["all", "lap_only", "no_pred", "no_jac"])
@pytest.mark.parametrize("case", list(DECODERS))
def test_decoder_lap_vjp_reference_is_the_oracle_differentiated_three_times(case, cots):
    kw = dict(DECODERS[case])
    model, cfg = ac._cpu_model(out=kw.pop("out", 1), **kw)
    sd = {n: v.detach().double() for n, v in model.state_dict().items()}
    gen = torch.Generator().manual_seed(19)
    m, nq = 64, 40
    tok = model.latent_tokens.double()
    q = torch.rand(nq, 3, generator=gen, dtype=torch.float64) * 2.4 - 1.2
    ns = len(cfg.magno.scales)
    lists = _lists(case, ns, nq, m, gen)
    lat = torch.randn(m, 32, generator=gen, dtype=torch.float64, requires_grad=True)
    edges = types.SimpleNamespace(**{f"decoder_edge_index_s{s}": torch.stack([l[0].long(), l[1].long()]) for s, l in enumerate(lists)})
    xg = q.clone().requires_grad_(True)
    pred = orc.magno_decoder(sd, cfg.magno, lat, xg, tok, edges)
    oc = pred.shape[1]
    gy = torch.randn(nq, oc, generator=gen, dtype=torch.float64) if cots in ("all", "no_jac") else None
    gj = torch.randn(nq, oc, 3, generator=gen, dtype=torch.float64) if cots in ("all", "no_pred") else None
    gl = torch.randn(nq, oc, generator=gen, dtype=torch.float64)
    jac = torch.stack([torch.autograd.grad(pred[:, o].sum(), xg, create_graph=True)[0] for o in range(oc)], dim=1)     # [Nq, out, 3]
    # pred[q] depends on x[q] alone: d (sum_q jac[q, o, d]) / d x[q, d] is the second derivative of pred[q, o] along axis d
    lap = torch.stack([sum(torch.autograd.grad(jac[:, o, d].sum(), xg, create_graph=True)[0][:, d] for d in range(3))
                       for o in range(oc)], dim=1)
    loss = (lap * gl).sum() + (0.0 if gy is None else (pred * gy).sum()) + (0.0 if gj is None else (jac * gj).sum())
    (ref,) = torch.autograd.grad(loss, lat)
    got, got_pred, got_jac, got_lap = LA.decoder_lap_vjp(sd, lists, tok, q, lat, gy, gj, gl, cfg.magno.use_scale_weights)
    peak = ref.abs().max()
    assert peak > 0 and lap.abs().max() > 0
    assert (got_pred - pred.detach()).abs().max() <= 1e-12 * pred.abs().max()
    assert (got_jac - jac.detach()).abs().max() <= 1e-11 * jac.abs().max()
    assert (got_lap - lap.detach()).abs().max() <= 1e-10 * lap.abs().max()
    assert (got - ref).abs().max() <= 1e-9 * peak, (got - ref).abs().max() / peak


# ---- refusals that need no device -------------------------------------------------------------------------------------------------------
def _args(nq=5, out=1):
    return torch.zeros(64, 32), torch.zeros(nq, 3), torch.zeros(nq, out), torch.zeros(nq, out, 3), torch.zeros(nq, out)


def test_argument_rules_raise_on_the_host():
    model, _ = ac._cpu_model(neighbor_strategy=["knn", "reverse"])
    lat, q, g, gj, gl = _args()
    with pytest.raises(ValueError, match="reverse"):
        model.sample_laplacian_vjp(lat, q, g, gj, gl)
    with pytest.raises(ValueError, match="reverse"):
        model.sample_laplacian_autograd(lat, q)
    model, _ = ac._cpu_model()
    with pytest.raises(ValueError, match="ONE sample"):
        model.sample_laplacian_vjp(torch.zeros(128, 32), q, g, gj, gl)
    with pytest.raises(ValueError, match="ONE sample"):
        model.sample_laplacian_autograd(torch.zeros(128, 32), q)
    with pytest.raises(ValueError, match="chunk_points"):
        model.sample_laplacian_vjp(lat, q, g, gj, gl, chunk_points=0)
    with pytest.raises(ValueError, match="chunk_points"):
        model.sample_laplacian_autograd(lat, q, chunk_points=0)
    for bad in (g.double(), torch.zeros(5, 2), torch.zeros(4, 1), torch.zeros(5), [[0.0]] * 5):
        with pytest.raises(ValueError, match="cot_pred"):
            model.sample_laplacian_vjp(lat, q, bad, gj, gl)
    for bad in (gj.double(), torch.zeros(5, 1, 2), torch.zeros(4, 1, 3), torch.zeros(5, 3), [[[0.0] * 3]] * 5):
        with pytest.raises(ValueError, match="cot_jac"):
            model.sample_laplacian_vjp(lat, q, g, bad, gl)
    for bad in (gl.double(), torch.zeros(5, 2), torch.zeros(4, 1), torch.zeros(5), None, [[0.0]] * 5):
        with pytest.raises(ValueError, match="cot_lap"):
            model.sample_laplacian_vjp(lat, q, g, gj, bad)
    with pytest.raises(ValueError, match="query_pos requires grad"):
        model.sample_laplacian_autograd(lat, q.clone().requires_grad_(True))


@pytest.mark.parametrize("case", list(ac.REFUSALS))
def test_configurations_are_refused_by_name(case):
    kw, msg = ac.REFUSALS[case]
    model, _ = ac._cpu_model(**kw)
    lat, q, g, gj, gl = _args()
    with pytest.raises(NotImplementedError, match="adjoint of the field's Laplacian.*" + msg):
        model.sample_laplacian_vjp(lat, q, g, gj, gl)
    with pytest.raises(NotImplementedError, match="adjoint of the field's Laplacian.*" + msg):
        model.sample_laplacian_vjp(lat, q, None, None, gl)
    with pytest.raises(NotImplementedError, match="adjoint of the field's Laplacian.*" + msg):
        model.sample_laplacian_autograd(lat.clone().requires_grad_(True), q)


def test_a_projection_outside_the_jet_family_and_a_sharded_model_are_refused():
    model, _ = ac._cpu_model()
    lat, q, g, gj, gl = _args()
    model.decoder.projection.fcs.append(torch.nn.Linear(1, 1))
    with pytest.raises(NotImplementedError, match="projection is not a two-layer erf-GELU MLP"):
        model.sample_laplacian_vjp(lat, q, g, gj, gl)
    model, _ = ac._cpu_model()
    model.decoder.projection.non_linearity = "relu"             # sample_jacobian_vjp covers it; the Laplacian's forward does not
    with pytest.raises(NotImplementedError, match="projection is not a two-layer erf-GELU MLP"):
        model.sample_laplacian_vjp(lat, q, g, gj, gl)
    with pytest.raises(NotImplementedError, match="projection is not a two-layer erf-GELU MLP"):
        model.sample_laplacian_autograd(lat.clone().requires_grad_(True), q)
    model, _ = ac._cpu_model()
    model.decoder._shard_group = object()
    with pytest.raises(NotImplementedError, match="point-sharded"):
        model.sample_laplacian_vjp(lat, q, g, gj, gl)
    model._shard_group = object()
    with pytest.raises(NotImplementedError, match="point-sharded"):
        model.sample_laplacian_autograd(lat, q)
