"""CPU: the adjoint of the field's Jacobian is in place -- gaot_gno_adj_jac and gaot_gno_adj_jac_workspace_bytes are declared in the
header, bound in _lib.SIGNATURES with the header's argument counts and exported by the library; the four k_gno_adj_jac instantiations
(1..4 hidden layers) exist and use no scratch; the host layers exist with their signatures; the fp64 references the GPU tests compare
against (tests/gno_jac_adj_ref.py) agree with one another -- the closed form against torch.autograd.grad of
<G, out> + sum_d <J_d, jac_d> with jac_d a create_graph=True derivative of the transform, within 1e-11 of the peak -- and the
decoder-level product written out step by step equals the fp64 oracle's decoder (oracle/gaot_oracle.py) differentiated first in the
query (create_graph=True, per output channel) and then in the latent, within 1e-10 of the peak: one scale, two scales summed, two
scales softmax-weighted on DIFFERENT lists per scale, four output channels, gelu and relu; and sample_jacobian_vjp /
sample_jacobian_autograd refuse on the host what sample_vjp refuses."""
import inspect
import os
import re
import sys
import types

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gaot_oracle as orc  # noqa: E402  (checker only)
import gno_adj_ref as REF  # noqa: E402
import gno_jac_adj_ref as JA  # noqa: E402
import test_field_adjoint_cpu as ac  # noqa: E402  (_operands, _cpu_model, the refusal table)
import test_field_hessian_cpu as hc  # noqa: E402  (_kernel_scratch_sizes)

NAMES = {"gaot_gno_adj_jac_workspace_bytes": 1, "gaot_gno_adj_jac": 17}           # arguments in the header


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


def test_the_four_kernels_exist_and_use_no_scratch():
    from gaot_3d_amd import _lib
    sizes = hc._kernel_scratch_sizes(_lib.load()._name)
    adj = {k: v for k, v in sizes.items() if "k_gno_adj_jac" in k}
    assert len(adj) == 4, sorted(adj)
    assert not any(adj.values()), adj
    assert not any(s in k for k in adj for s in ("k_gno_fwd", "AdjFwd", "jet2"))   # names the older tests do not count


def test_host_layers_exist_with_their_signatures():
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd import ops
    from gaot_3d_amd.model.gaot_3d import GAOT3D
    from gaot_3d_amd.model.layers.integral_transform import IntegralTransform
    from gaot_3d_amd.model.layers.magno import MAGNODecoder
    names = lambda fn: list(inspect.signature(fn).parameters)
    assert names(ops.gno_adjoint_jac) == ["weights", "biases", "y_pos", "x_pos", "grad_out", "grad_jac", "g", "k"]
    assert inspect.signature(ops.gno_adjoint_jac).parameters["k"].default is None
    assert names(IntegralTransform.adjoint_jac_knn) == ["self", "y_pos", "x_pos", "nbr", "k", "grad_out", "grad_jac", "graph"]
    assert names(IntegralTransform.adjoint_jac_rows) == ["self", "y_pos", "x_pos", "grad_out", "grad_jac", "graph"]
    assert names(MAGNODecoder.sample_jacobian_vjp) == ["self", "rndata_flat", "query_pos", "cot_pred", "cot_jac", "latent_tokens_pos",
                                                       "chunk_points"]
    assert names(GAOT3D.sample_jacobian_vjp) == ["self", "latent", "query_pos", "cot_pred", "cot_jac", "tokens_pos", "chunk_points"]
    assert names(GAOT3D.sample_jacobian_autograd) == ["self", "latent", "query_pos", "tokens_pos", "chunk_points"]
    assert issubclass(GF.SampleJacobianLatentFn, torch.autograd.Function)


# ---- the references -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh", [1, 4])
def test_closed_form_is_autograd_of_the_value_and_its_query_derivative(nh):
    nsrc = 23
    deg = [3, 0, 7, 1, 4, 40, 0]                       # empty rows, a single edge, a row longer than a tile
    gen, ws, bs, y, x = ac._operands(nh, nsrc, len(deg), 31 + nh)
    src, dst, rowptr = REF.random_list(deg, nsrc, gen)
    g = torch.randn(len(deg), 32, generator=gen, dtype=torch.float64)
    gj = torch.randn(3, len(deg), 32, generator=gen, dtype=torch.float64)
    closed = JA.adjoint_jac_closed(ws, bs, y, x, src, dst, rowptr, g, gj, nsrc)
    auto = JA.adjoint_jac_autograd(ws, bs, y, x, src, dst, rowptr, g, gj, nsrc)
    peak = auto.abs().max()
    assert peak > 0
    assert (auto - closed).abs().max() <= 1e-11 * peak, (auto - closed).abs().max() / peak
    # the tangent term is there: without J the closed form is the value adjoint's, and that is a different gradient
    value_only = JA.adjoint_jac_closed(ws, bs, y, x, src, dst, rowptr, g, torch.zeros_like(gj), nsrc)
    assert (value_only - REF.gno_adjoint_closed(ws, bs, y, x, src, dst, rowptr, g, nsrc)).abs().max() <= 1e-13 * peak
    assert (value_only - closed).abs().max() > 1e-2 * peak
    used = torch.zeros(nsrc, dtype=torch.bool)
    used[src.long()] = True
    assert (~used).any() and torch.equal(closed[~used], torch.zeros_like(closed[~used]))     # a source without edges: exact zeros
    # duality: <G, out> + sum_d <J_d, jac_d> = <df, f>
    f = torch.randn(nsrc, 32, generator=gen, dtype=torch.float64)
    out, jac = JA.gno_linear_jets(ws, bs, y, x, src, dst, rowptr, f)
    lhs = (g * out).sum() + (gj * jac).sum()
    rhs = (closed * f).sum()
    assert abs(lhs - rhs) <= 1e-12 * (closed * f).abs().sum()


DECODERS = {
    "one_scale": dict(),
    "one_scale_relu": dict(act="relu"),
    "four_channels": dict(out=4),
    "two_scales_weighted": dict(out=2, scales=[1.0, 2.0], use_scale_weights=True),
    "two_scales_weighted_relu": dict(out=2, scales=[1.0, 2.0], use_scale_weights=True, act="relu"),
    "two_scales_summed": dict(scales=[1.0, 2.0], use_scale_weights=False),
}


def _oracle_decoder(sd, mc, lat, q, tok, edges, act):
    """the oracle's decoder; with another projection activation, assembled from the oracle's own parts (``magno_decoder`` does not
    take one)"""
    if act == "gelu":
        return orc.magno_decoder(sd, mc, lat, q, tok, edges)
    outs = [orc.integral_transform(sd, "decoder.gno.", tok, q, getattr(edges, f"decoder_edge_index_s{si}"), lat,
                                   mc.out_gno_transform_type, mc.use_attn, mc.gno_coord_dim, mc.attention_type)
            for si in range(len(mc.scales))]
    return orc.channel_mlp(sd, "decoder.projection.", orc._scale_sum(sd, "decoder.", outs, q, mc.use_scale_weights), getattr(F, act))


@pytest.mark.parametrize("with_pred", [True, False])
@pytest.mark.parametrize("case", list(DECODERS))
def test_decoder_jac_vjp_reference_is_the_oracle_differentiated_twice(case, with_pred):
    kw = dict(DECODERS[case])
    act = kw.pop("act", "gelu")
    model, cfg = ac._cpu_model(out=kw.pop("out", 1), **kw)
    sd = {n: v.detach().double() for n, v in model.state_dict().items()}
    gen = torch.Generator().manual_seed(11)
    m, nq = 64, 40
    tok = model.latent_tokens.double()
    q = torch.rand(nq, 3, generator=gen, dtype=torch.float64) * 2.4 - 1.2
    ns = len(cfg.magno.scales)
    # a list of its own per scale (random rows, empty ones at the second scale): the case where the weights' tangents matter
    lists = [REF.random_list(torch.randint(0 if s else 1, 9 + 4 * s, (nq,), generator=gen).tolist(), m, gen) for s in range(ns)]
    lat = torch.randn(m, 32, generator=gen, dtype=torch.float64, requires_grad=True)
    edges = types.SimpleNamespace(**{f"decoder_edge_index_s{s}": torch.stack([l[0].long(), l[1].long()]) for s, l in enumerate(lists)})
    xg = q.clone().requires_grad_(True)
    pred = _oracle_decoder(sd, cfg.magno, lat, xg, tok, edges, act)
    gy = torch.randn(pred.shape, generator=gen, dtype=torch.float64) if with_pred else None
    gj = torch.randn(*pred.shape, 3, generator=gen, dtype=torch.float64)
    jac = torch.stack([torch.autograd.grad(pred[:, o].sum(), xg, create_graph=True)[0] for o in range(pred.shape[1])], dim=1)
    loss = (jac * gj).sum() + ((pred * gy).sum() if with_pred else 0.0)
    (ref,) = torch.autograd.grad(loss, lat)
    got, got_pred, got_jac = JA.decoder_jac_vjp(sd, lists, tok, q, lat, gy, gj, cfg.magno.use_scale_weights, act=act)
    peak = ref.abs().max()
    assert peak > 0
    assert (got_pred - pred.detach()).abs().max() <= 1e-12 * pred.abs().max()
    assert (got_jac - jac.detach()).abs().max() <= 1e-11 * jac.abs().max()
    assert (got - ref).abs().max() <= 1e-10 * peak, (got - ref).abs().max() / peak


# ---- refusals that need no device -------------------------------------------------------------------------------------------------------
def _args(nq=5, out=1):
    return torch.zeros(64, 32), torch.zeros(nq, 3), torch.zeros(nq, out), torch.zeros(nq, out, 3)


def test_argument_rules_raise_on_the_host():
    model, _ = ac._cpu_model(neighbor_strategy=["knn", "reverse"])
    lat, q, g, gj = _args()
    with pytest.raises(ValueError, match="reverse"):
        model.sample_jacobian_vjp(lat, q, g, gj)
    with pytest.raises(ValueError, match="reverse"):
        model.sample_jacobian_autograd(lat, q)
    model, _ = ac._cpu_model()
    with pytest.raises(ValueError, match="ONE sample"):
        model.sample_jacobian_vjp(torch.zeros(128, 32), q, g, gj)
    with pytest.raises(ValueError, match="ONE sample"):
        model.sample_jacobian_autograd(torch.zeros(128, 32), q)
    with pytest.raises(ValueError, match="chunk_points"):
        model.sample_jacobian_vjp(lat, q, g, gj, chunk_points=0)
    with pytest.raises(ValueError, match="chunk_points"):
        model.sample_jacobian_autograd(lat, q, chunk_points=0)
    for bad in (g.double(), torch.zeros(5, 2), torch.zeros(4, 1), torch.zeros(5), [[0.0]] * 5):
        with pytest.raises(ValueError, match="cot_pred"):
            model.sample_jacobian_vjp(lat, q, bad, gj)
    for bad in (gj.double(), torch.zeros(5, 1, 2), torch.zeros(4, 1, 3), torch.zeros(5, 3), None, [[[0.0] * 3]] * 5):
        with pytest.raises(ValueError, match="cot_jac"):
            model.sample_jacobian_vjp(lat, q, g, bad)
    with pytest.raises(ValueError, match="query_pos requires grad"):
        model.sample_jacobian_autograd(lat, q.clone().requires_grad_(True))


@pytest.mark.parametrize("case", list(ac.REFUSALS))
def test_configurations_are_refused_by_name(case):
    kw, msg = ac.REFUSALS[case]
    model, _ = ac._cpu_model(**kw)
    lat, q, g, gj = _args()
    with pytest.raises(NotImplementedError, match="adjoint of the field's Jacobian.*" + msg):
        model.sample_jacobian_vjp(lat, q, g, gj)
    with pytest.raises(NotImplementedError, match="adjoint of the field's Jacobian.*" + msg):
        model.sample_jacobian_vjp(lat, q, None, gj)
    with pytest.raises(NotImplementedError, match="adjoint of the field's Jacobian.*" + msg):
        model.sample_jacobian_autograd(lat.clone().requires_grad_(True), q)


def test_a_projection_that_is_not_two_layers_and_a_sharded_model_are_refused():
    model, _ = ac._cpu_model()
    lat, q, g, gj = _args()
    model.decoder.projection.fcs.append(torch.nn.Linear(1, 1))
    with pytest.raises(NotImplementedError, match="projection is not two linear layers"):
        model.sample_jacobian_vjp(lat, q, g, gj)
    model, _ = ac._cpu_model()
    model.decoder.projection.non_linearity = "no_such_activation"
    with pytest.raises(NotImplementedError, match="named activation"):
        model.sample_jacobian_vjp(lat, q, g, gj)
    model, _ = ac._cpu_model()
    model.decoder._shard_group = object()
    with pytest.raises(NotImplementedError, match="point-sharded"):
        model.sample_jacobian_vjp(lat, q, g, gj)
    model._shard_group = object()
    with pytest.raises(NotImplementedError, match="point-sharded"):
        model.sample_jacobian_autograd(lat, q)


def test_an_activation_without_a_second_derivative_is_refused_by_name():
    from gaot_3d_amd.model.layers.magno import MAGNODecoder
    assert {"gelu", "relu"} <= set(MAGNODecoder.JAC_VJP_ACTS)
    z = torch.linspace(-3, 3, 61, dtype=torch.float64)
    for act in ("gelu", "relu"):                                                   # the host formulas against the reference's
        d1, d2 = MAGNODecoder._act_jets(z, act)
        assert (d1 - JA.ACT_GRAD[act](z)).abs().max() <= 1e-15
        assert d2 is None or (d2 - JA.ACT_GRAD2[act](z)).abs().max() <= 1e-15
    # on the host nothing streams, so the refusal that comes first there is the operands'; the activation's own is checked on the device
    model, _ = ac._cpu_model()
    model.decoder.projection.non_linearity = "silu"
    lat, q, g, gj = _args()
    with pytest.raises(NotImplementedError):
        model.sample_jacobian_vjp(lat, q, g, gj)
