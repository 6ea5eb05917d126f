"""CPU: the adjoint of the field's directional derivatives and Hessian is in place -- gaot_gno_adj_jet2_qd, its workspace size and
gaot_mlp2_jet2_cot_mid are declared in the header, bound in _lib.SIGNATURES with the header's argument counts and exported (ABI 11);
the four per-query-direction adjoint kernels (1..4 hidden layers) exist without scratch under a name of their own, the four
host-direction ones are still four, the element kernel exists without scratch; the host layers exist with their signatures; the fp64
references the GPU tests compare against (tests/gno_qdir_jet2_adj_ref.py) agree with independent ones -- the per-query closed form
against torch.autograd.grad through the per-query row-list jets (row degrees [3, 0, 7, 1, 4, 40, 0], 48 sources, nd in {1, 3, 6})
within 1e-10 of the peak, with the duality identity; with one direction set for every query it is adjoint_jet2_closed; the general
middle against autograd of the projection's jets and against lap_cot_mid; the Hessian's cotangent map against autograd through
_polarise's expression; the decoder-level products against the fp64 oracle's decoder differentiated twice in the query and then in
the latent within 1e-9 of the peak ('knn', ragged lists with empty rows, two softmax-weighted scales on different lists, with and
without the optional cotangents); and the new calls refuse on the host what they refuse."""
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
import gno_jet2_adj_ref as LA  # noqa: E402
import gno_qdir_jet2_adj_ref as QA  # noqa: E402
from gno_jet2_ref import gelu, gelu_d1, gelu_d2  # noqa: E402
import test_field_adjoint_cpu as ac  # noqa: E402  (_operands, _cpu_model, the refusal table)
import test_field_hessian_cpu as hc  # noqa: E402  (_kernel_scratch_sizes)
import test_field_laplacian_adjoint_cpu as lc  # noqa: E402  (DECODERS, _lists, GENERIC)
from gaot_3d_amd.model.layers.magno import MAGNODecoder  # noqa: E402

NAMES = {"gaot_gno_adj_jet2_qd_workspace_bytes": 1, "gaot_gno_adj_jet2_qd": 21, "gaot_mlp2_jet2_cot_mid": 12}   # arguments in the header
DEG = [3, 0, 7, 1, 4, 40, 0]                           # empty rows, a single edge, a row longer than a tile
assert MAGNODecoder.HESSIAN_DIRS == QA.HESSIAN_DIRS and MAGNODecoder.HESSIAN_PAIRS == QA.HESSIAN_PAIRS


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
    if name == "gaot_gno_adj_jet2_qd":                 # the host-direction entry point: the same argument list
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES["gaot_gno_adj_jet2"]


def test_the_four_per_query_kernels_and_the_element_kernel_exist_without_scratch():
    from gaot_3d_amd import _lib
    sizes = hc._kernel_scratch_sizes(_lib.load()._name)
    qd = {k: v for k, v in sizes.items() if "k_gno_adjqd_jet2" in k}
    assert len(qd) == 4, sorted(qd)
    assert not any(qd.values()), qd
    host = {k: v for k, v in sizes.items() if "k_gno_adj_jet2" in k}              # the four older names are still counted as four
    assert len(host) == 4 and not any(host.values()) and not set(host) & set(qd), sorted(host)
    assert not any(s in k for k in qd for s in ("k_gno_fwd", "AdjFwd", "k_gno_adj_jac", "k_gno_qd"))    # names the older tests count
    mid = {k: v for k, v in sizes.items() if "k_mlp2_cot_jet2_mid" in k}
    assert len(mid) == 6 and not any(mid.values()), mid                           # one instantiation per nd = 1..6
    assert not any(s in k for k in mid for s in ("k_mlp2_jet2", "k_mlp2_lap_cot_mid"))


def test_host_layers_exist_with_their_signatures():
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd import ops
    from gaot_3d_amd.model.gaot_3d import GAOT3D
    from gaot_3d_amd.model.layers.integral_transform import IntegralTransform
    names = lambda fn: list(inspect.signature(fn).parameters)
    assert names(ops.gno_adjoint_jet2_qd) == ["weights", "biases", "y_pos", "x_pos", "qdirs", "grad_out", "grad_d1", "grad_d2", "g", "k"]
    assert inspect.signature(ops.gno_adjoint_jet2_qd).parameters["k"].default is None
    assert names(ops.mlp2_jet2_cot_mid) == ["zus", "a", "ab", "b1", "out"]
    assert names(IntegralTransform.adjoint_jet2_knn_qd) == ["self", "y_pos", "x_pos", "nbr", "k", "qdirs", "grad_out", "grad_d1",
                                                            "grad_d2", "graph"]
    assert names(IntegralTransform.adjoint_jet2_rows_qd) == ["self", "y_pos", "x_pos", "qdirs", "grad_out", "grad_d1", "grad_d2", "graph"]
    assert names(MAGNODecoder.sample_directional_vjp) == ["self", "rndata_flat", "query_pos", "dirs", "cot_pred", "cot_d1", "cot_d2",
                                                          "latent_tokens_pos", "chunk_points"]
    assert names(MAGNODecoder.sample_hessian_vjp) == ["self", "rndata_flat", "query_pos", "cot_pred", "cot_jac", "cot_hess",
                                                      "latent_tokens_pos", "chunk_points"]
    assert names(GAOT3D.sample_directional_vjp) == ["self", "latent", "query_pos", "dirs", "cot_pred", "cot_d1", "cot_d2", "tokens_pos",
                                                    "chunk_points"]
    assert names(GAOT3D.sample_directional_autograd) == ["self", "latent", "query_pos", "dirs", "tokens_pos", "chunk_points"]
    assert names(GAOT3D.sample_hessian_vjp) == ["self", "latent", "query_pos", "cot_pred", "cot_jac", "cot_hess", "tokens_pos",
                                                "chunk_points"]
    assert names(GAOT3D.sample_hessian_autograd) == ["self", "latent", "query_pos", "tokens_pos", "chunk_points"]
    for fn in (GAOT3D.sample_directional_vjp, GAOT3D.sample_directional_autograd, GAOT3D.sample_hessian_vjp,
               GAOT3D.sample_hessian_autograd):
        for p in ("tokens_pos", "chunk_points"):
            assert inspect.signature(fn).parameters[p].default is None
    assert issubclass(GF.SampleDirectionalLatentFn, torch.autograd.Function)
    assert issubclass(GF.SampleHessianLatentFn, torch.autograd.Function)


# ---- the references -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["plane_per_direction", "one_plane"])
@pytest.mark.parametrize("nd", [1, 3, 6])
@pytest.mark.parametrize("nh", [1, 4])
def test_per_query_closed_form_is_autograd_through_the_per_query_jets(nh, nd, shared):
    nsrc = 48                                          # more sources than edges leave: some stay without one
    gen, ws, bs, y, x = ac._operands(nh, nsrc, len(DEG), 63 + 7 * nh + nd)
    src, dst, rowptr = REF.random_list(DEG, nsrc, gen)
    v = torch.randn(len(DEG), nd, 3, generator=gen, dtype=torch.float64)          # different for every query
    g = torch.randn(len(DEG), 32, generator=gen, dtype=torch.float64)
    p = torch.randn(nd, len(DEG), 32, generator=gen, dtype=torch.float64)
    s = torch.randn(1 if shared else nd, len(DEG), 32, generator=gen, dtype=torch.float64)
    closed = QA.adjoint_jet2_qd_closed(ws, bs, y, x, src, dst, rowptr, v, g, p, s, nsrc)
    auto = QA.adjoint_jet2_qd_autograd(ws, bs, y, x, src, dst, rowptr, v, g, p, s, nsrc)
    peak = auto.abs().max()
    assert peak > 0
    assert (auto - closed).abs().max() <= 1e-10 * peak, (auto - closed).abs().max() / peak
    # the directions are read per query: one query's directions on all of them give another gradient
    same = QA.adjoint_jet2_qd_closed(ws, bs, y, x, src, dst, rowptr, v[:1].expand_as(v), g, p, s, nsrc)
    assert (same - closed).abs().max() > 1e-2 * peak
    used = torch.zeros(nsrc, dtype=torch.bool)
    used[src.long()] = True
    assert (~used).any() and torch.equal(closed[~used], torch.zeros_like(closed[~used]))     # a source without edges: exact zeros
    # duality: <G, out> + sum_i <P_i, d1_i> + sum_i <S_i, d2_i> = <df, f>
    f = torch.randn(nsrc, 32, generator=gen, dtype=torch.float64)
    out, d1, d2 = QA.gno_rows_jet2_qd(ws, bs, y, x, src, dst, rowptr, f, "linear", v)
    lhs = (g * out).sum() + (p * d1).sum() + (s.expand_as(d2) * d2).sum()
    assert abs(lhs - (closed * f).sum()) <= 1e-12 * (closed * f).abs().sum()


@pytest.mark.parametrize("nd", [1, 3, 6])
def test_with_one_direction_set_for_every_query_it_is_the_host_direction_closed_form(nd):
    nsrc = 48
    gen, ws, bs, y, x = ac._operands(2, nsrc, len(DEG), 91 + nd)
    src, dst, rowptr = REF.random_list(DEG, nsrc, gen)
    dirs = lc.GENERIC[:nd]
    v = torch.tensor(dirs, dtype=torch.float64)[None].expand(len(DEG), nd, 3)
    g = torch.randn(len(DEG), 32, generator=gen, dtype=torch.float64)
    p, s = (torch.randn(nd, len(DEG), 32, generator=gen, dtype=torch.float64) for _ in range(2))
    got = QA.adjoint_jet2_qd_closed(ws, bs, y, x, src, dst, rowptr, v, g, p, s, nsrc)
    ref = LA.adjoint_jet2_closed(ws, bs, y, x, src, dst, rowptr, dirs, g, p, s, nsrc)
    assert ref.abs().max() > 0 and (got - ref).abs().max() <= 1e-13 * ref.abs().max()


@pytest.mark.parametrize("with_a", [True, False])
@pytest.mark.parametrize("nd", [1, 3, 6])
def test_the_general_middle_is_autograd_of_the_projection_jets(nd, with_a):
    gen = torch.Generator().manual_seed(5 + nd)
    n, h = 9, 12
    z = torch.randn(n, h, generator=gen, dtype=torch.float64, requires_grad=True)
    u, s = (torch.randn(nd, n, h, generator=gen, dtype=torch.float64, requires_grad=True) for _ in range(2))
    a = torch.randn(n, h, generator=gen, dtype=torch.float64)
    ad, bd = (torch.randn(nd, n, h, generator=gen, dtype=torch.float64) for _ in range(2))
    # the jets at hidden width: a(z), a'(z) u_i, a''(z) u_i^2 + a'(z) s_i, contracted with A, A_i, B_i
    loss = (gelu_d1(z) * u * ad).sum() + ((gelu_d2(z) * u * u + gelu_d1(z) * s) * bd).sum()
    if with_a:
        loss = loss + (gelu(z) * a).sum()
    dz, du, ds = torch.autograd.grad(loss, (z, u, s))
    got = QA.jet2_cot_mid(z, u, s, a if with_a else None, ad, bd)
    assert got.shape[0] == 1 + 2 * nd
    for name, x, ref in (("dz", got[0], dz), ("du", got[1:1 + nd], du), ("ds", got[1 + nd:], ds)):
        assert ref.abs().max() > 0 and (x - ref).abs().max() <= 1e-12 * ref.abs().max(), name


def test_the_general_middle_with_one_second_order_plane_is_the_laplacian_middle():
    gen = torch.Generator().manual_seed(17)
    n, h = 9, 12
    z, a, al = (torch.randn(n, h, generator=gen, dtype=torch.float64) for _ in range(3))
    u, s, ad = (torch.randn(3, n, h, generator=gen, dtype=torch.float64) for _ in range(3))
    got = QA.jet2_cot_mid(z, u, s, a, ad, al[None].expand(3, n, h))
    ref = LA.lap_cot_mid(z, u, s.sum(0), a, ad, al)
    assert (got[:4] - ref[:4]).abs().max() <= 1e-13 * ref[:4].abs().max()          # dz and the three du_d
    for i in range(3):                                 # every ds_i is the one ds: x''_0 + x''_1 + x''_2 gets it on each term
        assert (got[4 + i] - ref[4]).abs().max() <= 1e-13 * ref[4].abs().max()


def test_the_hessian_cotangent_map_is_autograd_through_the_polarisation():
    gen = torch.Generator().manual_seed(23)
    n, oc = 11, 3
    d1, d2 = (torch.randn(n, oc, 6, generator=gen, dtype=torch.float64, requires_grad=True) for _ in range(2))
    cj = torch.randn(n, oc, 3, generator=gen, dtype=torch.float64)
    ch = torch.randn(n, oc, 3, 3, generator=gen, dtype=torch.float64)              # NOT symmetric
    jac, hess = QA.polarise(d1, d2)
    # the expression is the decoder's: the same numbers through MAGNODecoder._polarise
    j2, h2 = torch.empty(n, oc, 3, dtype=torch.float64), torch.empty(n, oc, 3, 3, dtype=torch.float64)
    MAGNODecoder._polarise(types.SimpleNamespace(HESSIAN_PAIRS=MAGNODecoder.HESSIAN_PAIRS), d1.detach(), d2.detach(), j2, h2)
    assert torch.equal(j2, jac.detach()) and torch.equal(h2, hess.detach())
    p_ref, s_ref = torch.autograd.grad((jac * cj).sum() + (hess * ch).sum(), (d1, d2))
    p, s = QA.hessian_cot(cj, ch)
    assert (p - p_ref).abs().max() <= 1e-14 and (s - s_ref).abs().max() <= 1e-14 * s_ref.abs().max()
    assert s_ref[:, :, 3:].abs().max() > 0 and torch.equal(p[:, :, 3:], torch.zeros(n, oc, 3, dtype=torch.float64))
    # the decoder's map is the same one
    pm, sm = MAGNODecoder._polarise_cot(types.SimpleNamespace(HESSIAN_PAIRS=MAGNODecoder.HESSIAN_PAIRS), cj, ch)
    assert (pm - p_ref).abs().max() <= 1e-14 and (sm - s_ref).abs().max() <= 1e-14 * s_ref.abs().max()
    assert MAGNODecoder._polarise_cot(None, None, None) == (None, None)


def _oracle(case, seed, nq=40, m=64):
    kw = dict(lc.DECODERS[case])
    model, cfg = ac._cpu_model(out=kw.pop("out", 1), **kw)
    sd = {n: v.detach().double() for n, v in model.state_dict().items()}
    gen = torch.Generator().manual_seed(seed)
    tok = model.latent_tokens.double()
    q = torch.rand(nq, 3, generator=gen, dtype=torch.float64) * 2.4 - 1.2
    lists = lc._lists(case, len(cfg.magno.scales), nq, m, gen)
    lat = torch.randn(m, 32, generator=gen, dtype=torch.float64, requires_grad=True)
    edges = types.SimpleNamespace(**{f"decoder_edge_index_s{s}": torch.stack([l[0].long(), l[1].long()]) for s, l in enumerate(lists)})
    xg = q.clone().requires_grad_(True)
    pred = orc.magno_decoder(sd, cfg.magno, lat, xg, tok, edges)
    oc = pred.shape[1]
    jac = torch.stack([torch.autograd.grad(pred[:, o].sum(), xg, create_graph=True)[0] for o in range(oc)], dim=1)     # [Nq, out, 3]
    # pred[q] depends on x[q] alone: d (sum_q jac[q, o, i]) / d x[q, j] is d^2 pred[q, o] / d x_i d x_j
    hess = torch.stack([torch.stack([torch.autograd.grad(jac[:, o, i].sum(), xg, create_graph=True)[0] for i in range(3)], dim=1)
                        for o in range(oc)], dim=1)                                                                     # [Nq, out, 3, 3]
    return sd, cfg, gen, tok, q, lists, lat, pred, jac, hess


@pytest.mark.parametrize("cots", ["all", "d2_only", "no_pred", "no_d1", "d1_only"])
@pytest.mark.parametrize("case,nd", [("knn", 1), ("radius", 3), ("bidirectional_four_channels", 2), ("two_scales_weighted_radius", 3),
                                     ("two_scales_weighted_radius", 1), ("two_scales_summed_radius", 6), ("four_layers_knn", 6)])
def test_decoder_directional_vjp_reference_is_the_oracle_differentiated_three_times(case, nd, cots):
    sd, cfg, gen, tok, q, lists, lat, pred, jac, hess = _oracle(case, 29 + nd)
    nq, oc = pred.shape
    v = torch.randn(nq, nd, 3, generator=gen, dtype=torch.float64)                 # every query's own directions, not unit
    d1 = torch.einsum("qod,qnd->qon", jac, v)
    d2 = torch.einsum("qoij,qni,qnj->qon", hess, v, v)
    gy = torch.randn(nq, oc, generator=gen, dtype=torch.float64) if cots in ("all", "no_d1") else None
    g1 = torch.randn(nq, oc, nd, generator=gen, dtype=torch.float64) if cots in ("all", "no_pred", "d1_only") else None
    g2 = torch.randn(nq, oc, nd, generator=gen, dtype=torch.float64) if cots != "d1_only" else None
    loss = sum((t * g).sum() for t, g in ((pred, gy), (d1, g1), (d2, g2)) if g is not None)
    (ref,) = torch.autograd.grad(loss, lat)
    got, got_pred, got_d1, got_d2 = QA.decoder_dir_vjp(sd, lists, tok, q, lat.detach(), v, gy, g1, g2, cfg.magno.use_scale_weights)
    peak = ref.abs().max()
    assert peak > 0 and d2.abs().max() > 0
    assert (got_pred - pred.detach()).abs().max() <= 1e-12 * pred.abs().max()
    assert (got_d1 - d1.detach()).abs().max() <= 1e-11 * d1.abs().max()
    assert (got_d2 - d2.detach()).abs().max() <= 1e-10 * d2.abs().max()
    assert (got - ref).abs().max() <= 1e-9 * peak, (got - ref).abs().max() / peak


@pytest.mark.parametrize("cots", ["all", "hess_only", "no_pred", "no_jac"])
@pytest.mark.parametrize("case", ["knn", "bidirectional_four_channels", "two_scales_weighted_radius"])
def test_decoder_hessian_vjp_reference_is_the_oracle_differentiated_three_times(case, cots):
    sd, cfg, gen, tok, q, lists, lat, pred, jac, hess = _oracle(case, 37)
    nq, oc = pred.shape
    gy = torch.randn(nq, oc, generator=gen, dtype=torch.float64) if cots in ("all", "no_jac") else None
    gj = torch.randn(nq, oc, 3, generator=gen, dtype=torch.float64) if cots in ("all", "no_pred") else None
    gh = torch.randn(nq, oc, 3, 3, generator=gen, dtype=torch.float64)             # NOT symmetric
    loss = sum((t * g).sum() for t, g in ((pred, gy), (jac, gj), (hess, gh)) if g is not None)
    (ref,) = torch.autograd.grad(loss, lat)
    got, got_pred, got_jac, got_hess = QA.decoder_hess_vjp(sd, lists, tok, q, lat.detach(), gy, gj, gh, cfg.magno.use_scale_weights)
    peak = ref.abs().max()
    assert peak > 0 and hess.abs().max() > 0
    off = hess.detach()[:, :, 0, 1]
    assert off.abs().max() > 0 and (hess.detach() - hess.detach().transpose(2, 3)).abs().max() <= 1e-10 * hess.abs().max()
    assert (got_jac - jac.detach()).abs().max() <= 1e-11 * jac.abs().max()
    assert (got_hess - hess.detach()).abs().max() <= 1e-10 * hess.abs().max()
    assert (got - ref).abs().max() <= 1e-9 * peak, (got - ref).abs().max() / peak


# ---- refusals that need no device -------------------------------------------------------------------------------------------------------
def _args(nq=5, out=1, nd=2):
    return (torch.zeros(64, 32), torch.zeros(nq, 3), torch.zeros(nq, nd, 3), torch.zeros(nq, out), torch.zeros(nq, out, nd),
            torch.zeros(nq, out, 3), torch.zeros(nq, out, 3, 3))


def test_argument_rules_raise_on_the_host():
    model, _ = ac._cpu_model(neighbor_strategy=["knn", "reverse"])
    lat, q, v, g, gd, gj, gh = _args()
    with pytest.raises(ValueError, match="reverse"):
        model.sample_directional_vjp(lat, q, v, g, gd, gd)
    with pytest.raises(ValueError, match="reverse"):
        model.sample_hessian_vjp(lat, q, g, gj, gh)
    with pytest.raises(ValueError, match="reverse"):
        model.sample_directional_autograd(lat, q, v)
    with pytest.raises(ValueError, match="reverse"):
        model.sample_hessian_autograd(lat, q)
    model, _ = ac._cpu_model()
    for call in (lambda **kw: model.sample_directional_vjp(torch.zeros(128, 32), q, v, g, gd, gd, **kw),
                 lambda **kw: model.sample_hessian_vjp(torch.zeros(128, 32), q, g, gj, gh, **kw),
                 lambda **kw: model.sample_directional_autograd(torch.zeros(128, 32), q, v, **kw),
                 lambda **kw: model.sample_hessian_autograd(torch.zeros(128, 32), q, **kw)):
        with pytest.raises(ValueError, match="ONE sample"):
            call()
    for call in (lambda **kw: model.sample_directional_vjp(lat, q, v, g, gd, gd, **kw),
                 lambda **kw: model.sample_hessian_vjp(lat, q, g, gj, gh, **kw),
                 lambda **kw: model.sample_directional_autograd(lat, q, v, **kw),
                 lambda **kw: model.sample_hessian_autograd(lat, q, **kw)):
        with pytest.raises(ValueError, match="chunk_points"):
            call(chunk_points=0)
    # the directions: _query_dirs's rules
    for bad in (v.double(), torch.zeros(4, 2, 3), torch.zeros(5, 2, 2), torch.zeros(5, 7, 3), torch.zeros(5, 0, 3), [[0.0] * 3] * 5):
        with pytest.raises(ValueError, match="dirs|directions per query"):
            model.sample_directional_vjp(lat, q, bad, g, gd, gd)
        with pytest.raises(ValueError, match="dirs|directions per query"):
            model.sample_directional_autograd(lat, q, bad)
    # [Nq, 3] is one direction per query: the cotangents are [Nq, out, 1] then
    with pytest.raises(ValueError, match="cot_d1"):
        model.sample_directional_vjp(lat, q, v[:, 0], g, gd, None)
    for bad in (g.double(), torch.zeros(5, 2), torch.zeros(4, 1), torch.zeros(5), [[0.0]] * 5):
        with pytest.raises(ValueError, match="cot_pred"):
            model.sample_directional_vjp(lat, q, v, bad, gd, gd)
        with pytest.raises(ValueError, match="cot_pred"):
            model.sample_hessian_vjp(lat, q, bad, gj, gh)
    for name, args in (("cot_d1", lambda b: (g, b, gd)), ("cot_d2", lambda b: (g, gd, b))):
        for bad in (gd.double(), torch.zeros(5, 1, 3), torch.zeros(4, 1, 2), torch.zeros(5, 2), [[[0.0] * 2]] * 5):
            with pytest.raises(ValueError, match=name):
                model.sample_directional_vjp(lat, q, v, *args(bad))
    for bad in (gj.double(), torch.zeros(5, 1, 2), torch.zeros(4, 1, 3), torch.zeros(5, 3)):
        with pytest.raises(ValueError, match="cot_jac"):
            model.sample_hessian_vjp(lat, q, g, bad, gh)
    for bad in (gh.double(), torch.zeros(5, 1, 3), torch.zeros(5, 1, 3, 2), torch.zeros(4, 1, 3, 3), torch.zeros(5, 1, 6)):
        with pytest.raises(ValueError, match="cot_hess"):
            model.sample_hessian_vjp(lat, q, g, gj, bad)
    # all three None: nothing to pull back
    with pytest.raises(ValueError, match="all None"):
        model.sample_directional_vjp(lat, q, v, None, None, None)
    with pytest.raises(ValueError, match="all None"):
        model.sample_hessian_vjp(lat, q, None, None, None)
    # gradients flow to the latent only
    with pytest.raises(ValueError, match="query_pos requires grad"):
        model.sample_directional_autograd(lat, q.clone().requires_grad_(True), v)
    with pytest.raises(ValueError, match="query_pos requires grad"):
        model.sample_hessian_autograd(lat, q.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="dirs requires grad"):
        model.sample_directional_autograd(lat, q, v.clone().requires_grad_(True))


@pytest.mark.parametrize("case", list(ac.REFUSALS))
def test_configurations_are_refused_by_name(case):
    kw, msg = ac.REFUSALS[case]
    model, _ = ac._cpu_model(**kw)
    lat, q, v, g, gd, gj, gh = _args()
    what = "adjoint of the field's directional derivatives.*"
    with pytest.raises(NotImplementedError, match=what + msg):
        model.sample_directional_vjp(lat, q, v, g, gd, gd)
    with pytest.raises(NotImplementedError, match=what + msg):
        model.sample_directional_vjp(lat, q, v, None, None, gd)
    with pytest.raises(NotImplementedError, match=what + msg):
        model.sample_directional_autograd(lat.clone().requires_grad_(True), q, v)
    what = "adjoint of the field's Hessian.*"
    with pytest.raises(NotImplementedError, match=what + msg):
        model.sample_hessian_vjp(lat, q, g, gj, gh)
    with pytest.raises(NotImplementedError, match=what + msg):
        model.sample_hessian_vjp(lat, q, None, None, gh)
    with pytest.raises(NotImplementedError, match=what + msg):
        model.sample_hessian_autograd(lat.clone().requires_grad_(True), q)


def test_a_projection_outside_the_jet_family_and_a_sharded_model_are_refused():
    lat, q, v, g, gd, gj, gh = _args()

    def calls(model):
        return (lambda: model.sample_directional_vjp(lat, q, v, g, gd, gd), lambda: model.sample_hessian_vjp(lat, q, g, gj, gh),
                lambda: model.sample_directional_autograd(lat.clone().requires_grad_(True), q, v),
                lambda: model.sample_hessian_autograd(lat.clone().requires_grad_(True), q))

    model, _ = ac._cpu_model()
    model.decoder.projection.fcs.append(torch.nn.Linear(1, 1))
    for call in calls(model):
        with pytest.raises(NotImplementedError, match="projection is not a two-layer erf-GELU MLP"):
            call()
    model, _ = ac._cpu_model()
    model.decoder.projection.non_linearity = "relu"
    for call in calls(model):
        with pytest.raises(NotImplementedError, match="projection is not a two-layer erf-GELU MLP"):
            call()
    model, _ = ac._cpu_model()
    model.decoder._shard_group = object()
    for call in calls(model)[:2]:
        with pytest.raises(NotImplementedError, match="point-sharded"):
            call()
    model._shard_group = object()
    for call in calls(model)[2:]:
        with pytest.raises(NotImplementedError, match="point-sharded"):
            call()
