"""GPU: the adjoint of the field's Jacobian -- gaot_gno_adj_jac (ops.gno_adjoint_jac), IntegralTransform.adjoint_jac_knn / adjoint_jac_rows,
MAGNODecoder / GAOT3D.sample_jacobian_vjp and GAOT3D.sample_jacobian_autograd (functional.SampleJacobianLatentFn).

Op level (211 sources, 1..4 hidden layers): regular lists Nq in {1, 7, 33, 1000} x k in {1, 4, 8, 32} against the fp64 closed form
(tests/gno_jac_adj_ref.py); with grad_jac = 0 no further from fp64 than max(4 x ops.gno_adjoint on the same operands, 1e-6 of the
peak); the duality <G, out> + sum_d <J_d, jac_d> = <grad_f, f> with out, jac from the tangent kernels on the same lists, both sides
summed in fp64, within 1e-3 of sum |terms|; two launches per call.  Rows built by hand (200 queries on one token; rows ending / starting
on tile boundaries with E = 69) through the raw ABI over a NaN pre-fill: unused tokens exact zeros; E = 0 is the fix-up alone; zero
queries.  The ragged lists a-e of the row-list tests take the degree from rowptr_dst; on a regular list the k form and the rowptr_dst
form agree bit for bit; two calls and bf16 mode give the same bits; bad operands raise GaotError before any launch.

Model level (hb._setup: 4096 points, latent 8^3, k = 8, r = 0.45, 300 + 300 queries partly outside the box): sample_jacobian_vjp with
random cot_pred and cot_jac against the fp64 oracle's decoder differentiated first in the query and then in the latent, on the lists
the streamed routes use, for 'knn' / 'radius' / 'bidirectional' and the SHAPES of the adjoint test (two softmax-weighted scales on
'radius' among them: the case where the tangents of the weights matter); cot_jac = 0 meets sample_vjp within 1e-5 of the peak;
cot_pred = None; chunkings None / 250 / 64 each at the bar, within 1e-5 of the peak of one another, bit-reproducible, the same bits
in bf16 mode; sample_jacobian_autograd's forward is sample_jacobian(row_lists=True) and its backward sample_jacobian_vjp, bit for
bit, and a normal-derivative loss chained through model.latent gives an encoder parameter the gradient of the fp64 oracle of the
whole model; timing keys; memory; refusals; the row route in a capture.

Bars: the project's fp32 bar for derivatives (FP32_BAR: max error <= 1e-3 of the reference's peak, cosine >= 0.99999), every peak
asserted > 0.  Distances measured on an MI355X are quoted in DESIGN.md 3.2f."""
import copy
import ctypes as C
import os
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
import gno_rows_jac_ref as JREF  # noqa: E402  (ragged_list)
import test_coord_grad_gpu as cg  # noqa: E402  (_batch64)
import test_field_adjoint_gpu as ag  # noqa: E402  (the regular and hand-built lists, the models, SHAPES, the refusal table)
import test_field_hessian_gpu as hb  # noqa: E402  (the model fixture, the watcher, check(), the bar, the queries)
import test_field_jacobian_rows_gpu as jr  # noqa: E402  (the lists a-e, the device operands)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NSRC = jr.NSRC
FP32_BAR = hb.FP32_BAR


def _cot_jac(nq, gen):
    return torch.randn(3, nq, 32, generator=gen)


# ---- op level: regular lists ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh", [1, 2, 3, 4])
def test_regular_lists_meet_fp64_the_value_adjoint_and_the_duality(nh):
    from gaot_3d_amd import graph, ops
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(nh, "linear")
    worst_identity = worst = 0.0
    for nq in ag.NQS:
        for k in ag.KS:
            src, dst, rowptr, x, g = ag._regular(nq, k, gen)
            gj = _cot_jac(nq, gen)
            xd, gd, gjd, nbr = x.to(DEV), g.to(DEV), gj.to(DEV), src.to(DEV)
            gs = graph.by_source((nbr, k), NSRC)
            n0 = ops.launch_count()
            got = ops.gno_adjoint_jac(wd, bd, yd, xd, gd, gjd, gs, k)
            assert ops.launch_count() == n0 + 2, (nq, k)                                   # the kernel and its fix-up
            assert got.shape == (NSRC, 32) and got.dtype == torch.float32
            jets = JA.kernel_jets(ws, bs, y, x, src, dst)
            ref = JA.adjoint_jac_closed(ws, bs, y, x, src, dst, rowptr, g, gj, NSRC, jets)
            rel, _ = hb.check(f"gno_adj_jac/nh{nh}/nq{nq}/k{k}", got, ref, quiet=True)
            worst = max(worst, rel)
            # grad_jac = 0: the value adjoint, no further from fp64 than gno_adjoint
            ref0 = REF.gno_adjoint_closed(ws, bs, y, x, src, dst, rowptr, g, NSRC)
            peak0 = ref0.abs().max().item()
            assert peak0 > 0
            d_new = ag._dist(ops.gno_adjoint_jac(wd, bd, yd, xd, gd, torch.zeros_like(gjd), gs, k), ref0)
            d_old = ag._dist(ops.gno_adjoint(wd, bd, yd, xd, gd, gs, k), ref0)
            print(f"[adjoint_jac] nh{nh} nq{nq} k{k}: rel_to_peak {rel:.3e}; grad_jac = 0: |adj_jac - fp64| = {d_new:.3e}, "
                  f"|gno_adj - fp64| = {d_old:.3e}, peak {peak0:.3e}")
            assert d_new <= max(4.0 * d_old, 1e-6 * peak0), (nq, k, d_new, d_old, peak0)
            # <G, out> + sum_d <J_d, jac_d> against <grad_f, f>, both sides in fp64
            out, jac = ops.gno_forward_knn_jac("linear", wd, bd, yd, xd, fd, None, nbr, k)
            lhs = (g.double() * out.double().cpu()).sum().item() + (gj.double() * jac.double().cpu()).sum().item()
            rhs = (got.double().cpu() * f.double()).sum().item()
            scale = (JA.adjoint_jac_terms(ws, bs, y, x, src, dst, rowptr, g, gj, jets) * f.double()[src.long()]).abs().sum().item()
            assert scale > 0
            worst_identity = max(worst_identity, abs(lhs - rhs) / scale)
            assert abs(lhs - rhs) <= 1e-3 * scale, (nq, k, lhs, rhs, scale)
    print(f"[adjoint_jac] nh{nh}: worst kernel / fp64 = {worst:.3e} of the peak; worst |<G, out> + <J, jac> - <A^T, f>| / sum|terms| "
          f"= {worst_identity:.3e}")


def _raw(wd, bd, yd, xd, gd, gjd, g, k, fill):
    """gaot_gno_adj_jac through the C ABI into a result pre-filled with ``fill``"""
    from gaot_3d_amd import _lib, ops
    lib = _lib.load()
    m, keep = ops._mlp_struct(wd, bd)
    out = torch.full((g.num_src, 32), fill, dtype=torch.float32, device=DEV)
    e = g.by_src.num_edges
    ws = ops._ws(lib.gaot_gno_adj_jac_workspace_bytes(e), DEV)
    rc = lib.gaot_gno_adj_jac(C.byref(m), ops._ptr(yd), ops._ptr(xd), ops._ptr(gd), ops._ptr(gjd),
                              ops._ptr(None if k else g.by_dst.rowptr), int(k or 0), ops._ptr(g.by_src.key), ops._ptr(g.by_src.other),
                              ops._ptr(g.by_src.rowptr), e, g.num_src, g.num_dst, ops._ptr(out), ops._ptr(ws), ws.numel(), ops._stream())
    assert rc == 0, lib.gaot_last_error()
    return out


@pytest.mark.parametrize("nh", [1, 2, 3, 4])
def test_row_shapes_built_by_hand(nh):
    from gaot_3d_amd import ops
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(nh, "linear")
    for name, (src, dst, nq) in ag._hand_lists(gen).items():
        assert src.numel() % 32 != 0
        x = torch.rand(nq, 3, generator=gen) * 2 - 1
        g, gj = torch.randn(nq, 32, generator=gen), _cot_jac(nq, gen)
        gr = ag._both_lists(src, dst, nq)
        rs = gr.by_src.rowptr.cpu()
        if name == "long_row":
            assert int(rs[8] - rs[7]) == 200 and (int(rs[8]) - 1) // 32 - int(rs[7]) // 32 >= 5
        else:
            assert rs[:5].tolist() == [0, 32, 42, 64, 69]
        xd, gd, gjd = x.to(DEV), g.to(DEV), gj.to(DEV)
        got = _raw(wd, bd, yd, xd, gd, gjd, gr, None, float("nan"))
        ref = JA.adjoint_jac_closed(ws, bs, y, x, src, dst, gr.by_dst.rowptr.cpu(), g, gj, NSRC)
        assert not torch.isnan(got).any(), name
        unused = torch.ones(NSRC, dtype=torch.bool)
        unused[src.long()] = False
        assert unused.any() and torch.equal(got[unused.to(DEV)], torch.zeros(int(unused.sum()), 32, device=DEV)), name
        hb.check(f"gno_adj_jac/nh{nh}/{name}", got, ref)
        assert torch.equal(got, ops.gno_adjoint_jac(wd, bd, yd, xd, gd, gjd, gr)), name


def test_no_edges_and_no_queries():
    from gaot_3d_amd import graph, ops
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(2, "linear")
    empty = lambda: torch.empty(0, dtype=torch.int32, device=DEV)
    zeros = torch.zeros(NSRC, 32, device=DEV)
    for nq in (5, 0):
        rows = ops.BipartiteGraph(ops.SortedEdges(torch.zeros(nq + 1, dtype=torch.int32, device=DEV), None, empty(), empty(), nq),
                                  None, NSRC, nq)
        gr = graph.by_source(rows, NSRC)
        xd, gd, gjd = torch.zeros(nq, 3, device=DEV), torch.ones(nq, 32, device=DEV), torch.ones(3, nq, 32, device=DEV)
        n0 = ops.launch_count()
        got = ops.gno_adjoint_jac(wd, bd, yd, xd, gd, gjd, gr)
        assert ops.launch_count() == n0 + 1                                                # the fix-up alone writes the zeros
        assert torch.equal(got, zeros)
        assert torch.equal(_raw(wd, bd, yd, xd, gd, gjd, gr, None, float("nan")), zeros)
    gr = graph.by_source((empty(), 8), NSRC)                                               # zero queries of a regular list
    assert torch.equal(ops.gno_adjoint_jac(wd, bd, yd, torch.zeros(0, 3, device=DEV), torch.zeros(0, 32, device=DEV),
                                           torch.zeros(3, 0, 32, device=DEV), gr, 8), zeros)


@pytest.mark.parametrize("nh", [1, 2, 3, 4])
def test_ragged_lists_take_the_degree_from_rowptr_dst(nh):
    from gaot_3d_amd import graph, ops
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(nh, "linear")
    for name, deg in jr.DEGREES.items():
        nq = len(deg)
        x = torch.rand(nq, 3, generator=gen) * 2 - 1
        g, gj = torch.randn(nq, 32, generator=gen), _cot_jac(nq, gen)
        src, dst, rowptr = JREF.ragged_list(deg, NSRC, gen)
        rows = jr._graph(src, dst, rowptr, NSRC)                                           # the forward-only graph query_lists returns
        gr = graph.by_source(rows, NSRC)
        xd, gd, gjd = x.to(DEV), g.to(DEV), gj.to(DEV)
        n0 = ops.launch_count()
        got = ops.gno_adjoint_jac(wd, bd, yd, xd, gd, gjd, gr)
        assert ops.launch_count() == n0 + 2, name
        jets = JA.kernel_jets(ws, bs, y, x, src, dst)
        ref = JA.adjoint_jac_closed(ws, bs, y, x, src, dst, rowptr, g, gj, NSRC, jets)
        hb.check(f"gno_adj_jac/nh{nh}/list_{name}", got, ref)
        assert torch.equal(got, ops.gno_adjoint_jac(wd, bd, yd, xd, gd, gjd, gr)), name    # reproducible
        with hb._precision("bf16"):
            assert torch.equal(got, ops.gno_adjoint_jac(wd, bd, yd, xd, gd, gjd, gr)), name   # exact fp32 in both modes
        # the duality on ragged rows, out and jac from the tangent kernel on the same by-query list
        out, jac = ops.gno_forward_jac("linear", wd, bd, yd, xd, fd, None, rows)
        lhs = (g.double() * out.double().cpu()).sum().item() + (gj.double() * jac.double().cpu()).sum().item()
        rhs = (got.double().cpu() * f.double()).sum().item()
        scale = (JA.adjoint_jac_terms(ws, bs, y, x, src, dst, rowptr, g, gj, jets) * f.double()[src.long()]).abs().sum().item()
        assert scale > 0 and abs(lhs - rhs) <= 1e-3 * scale, (name, lhs, rhs, scale)
        print(f"[adjoint_jac] nh{nh} list_{name}: |<G, out> + <J, jac> - <A^T, f>| / sum|terms| = {abs(lhs - rhs) / scale:.3e}")


def test_on_a_regular_list_k_and_rowptr_dst_agree_bit_for_bit():
    from gaot_3d_amd import graph, ops
    for nh in (1, 2, 3, 4):
        gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(nh, "linear")
        for nq, k in ((7, 4), (33, 32), (1000, 8), (33, 1)):
            src, dst, rowptr, x, g = ag._regular(nq, k, gen)
            xd, gd, gjd = x.to(DEV), g.to(DEV), _cot_jac(nq, gen).to(DEV)
            by_k = ops.gno_adjoint_jac(wd, bd, yd, xd, gd, gjd, graph.by_source((src.to(DEV), k), NSRC), k)
            by_rowptr = ops.gno_adjoint_jac(wd, bd, yd, xd, gd, gjd, graph.by_source(jr._graph(src, dst, rowptr, NSRC), NSRC))
            assert torch.equal(by_k, by_rowptr), (nh, nq, k)
            assert torch.equal(by_k, ops.gno_adjoint_jac(wd, bd, yd, xd, gd, gjd, ag._both_lists(src, dst, nq))), (nh, nq, k)


def test_bad_operands_raise_before_any_launch():
    from gaot_3d_amd import _lib, graph, ops
    from gaot_3d_amd._lib import GaotError
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(2, "linear")
    src, dst, rowptr, x, g = ag._regular(33, 8, gen)
    xd, gd, gjd = x.to(DEV), g.to(DEV), _cot_jac(33, gen).to(DEV)
    gr = graph.by_source((src.to(DEV), 8), NSRC)
    rows = jr._graph(src, dst, rowptr, NSRC)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    run = ops.gno_adjoint_jac
    bad = [
        lambda: run(wd, bd, yd, xd, gd, gjd[:, :, :16].contiguous(), gr, 8),               # cotangent planes: channels
        lambda: run(wd, bd, yd, xd, gd, gjd[:, :20].contiguous(), gr, 8),                  # rows
        lambda: run(wd, bd, yd, xd, gd, gjd[:2].contiguous(), gr, 8),                      # two planes
        lambda: run(wd, bd, yd, xd, gd, gjd.permute(1, 0, 2).contiguous(), gr, 8),         # [Nq, 3, 32]
        lambda: run(wd, bd, yd, xd, gd, gjd.permute(1, 0, 2).contiguous().permute(1, 0, 2), gr, 8),   # not contiguous
        lambda: run(wd, bd, yd, xd, gd, gjd.double(), gr, 8),                              # dtype
        lambda: run(wd, bd, yd, xd, gd, gjd.cpu(), gr, 8),                                 # host tensor
        lambda: run(wd, bd, yd, xd, gd, None, gr, 8),
        lambda: run(wd, bd, yd, xd, gd[:, :16].contiguous(), gjd, gr, 8),                  # gno_adjoint's rules
        lambda: run(wd, bd, yd, xd, gd.double(), gjd, gr, 8),
        lambda: run(wd, bd, yd, xd, gd.cpu(), gjd, gr, 8),
        lambda: run(wd, bd, yd[:100].contiguous(), xd, gd, gjd, gr, 8),
        lambda: run(wd, bd, yd, xd[:, :2].contiguous(), gd, gjd, gr, 8),
        lambda: run(wd, bd, yd, xd, gd, gjd, gr),                                          # neither rowptr_dst nor k
        lambda: run(wd, bd, yd, xd, gd, gjd, gr, 4),                                       # k that does not match the list
        lambda: run(wd, bd, yd, xd, gd, gjd, gr, 0),
        lambda: run(wd, bd, yd, xd, gd, gjd, rows),                                        # no by-source list
        lambda: run(wd[:1], bd[:1], yd, xd, gd, gjd, gr, 8),                               # one linear layer
        lambda: run([wd[0][:32].contiguous(), wd[1][:32, :32].contiguous(), wd[2][:, :32].contiguous()],
                    [bd[0][:32].contiguous(), bd[1][:32].contiguous(), bd[2]], yd, xd, gd, gjd, gr, 8),   # hidden width 32
    ]
    for i, call in enumerate(bad):
        with pytest.raises(GaotError):
            call()
        assert ops.launch_count() == n0, i
    # the C ABI's own check: a null grad_jac is an argument error, before any launch
    lib = _lib.load()
    m, keep = ops._mlp_struct(wd, bd)
    out = torch.zeros(NSRC, 32, device=DEV)
    wsp = ops._ws(lib.gaot_gno_adj_jac_workspace_bytes(gr.by_src.num_edges), DEV)
    rc = lib.gaot_gno_adj_jac(C.byref(m), ops._ptr(yd), ops._ptr(xd), ops._ptr(gd), ops._ptr(None), ops._ptr(None), 8,
                              ops._ptr(gr.by_src.key), ops._ptr(gr.by_src.other), ops._ptr(gr.by_src.rowptr), gr.by_src.num_edges, NSRC, 33,
                              ops._ptr(out), ops._ptr(wsp), wsp.numel(), ops._stream())
    assert rc != 0 and "grad_jac" in lib.gaot_last_error().decode() and ops.launch_count() == n0


# ---- model level ------------------------------------------------------------------------------------------------------------------------
CHUNKS = ag.CHUNKS
MODELS = ag.MODELS
SHAPES = ag.SHAPES
assert SHAPES["two_scales_weighted_radius"] == ("radius", dict(out=2, scales=[1.0, 2.0], use_scale_weights=True))


def _cots(nq, out, seed=29, device=DEV):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(nq, out, generator=gen).to(device), torch.randn(nq, out, 3, generator=gen).to(device)


def _route_edges(model, cfg, lat, q):
    """the edge lists of the streamed routes for these queries on the CPU, one per scale (knn_to_grid's ids, or graph.query_lists)"""
    from gaot_3d_amd import graph as device_graph
    dec = model.decoder
    tok = model._tokens(1, q.device, None, None)[0]
    with torch.no_grad():
        grid = dec._stream_grid(lat, q, tok)
    assert grid is not None
    edges = {}
    for si, scale in enumerate(cfg.magno.scales):
        if dec.decoder_strategy == "knn":
            ids = device_graph.knn_to_grid(q, grid, 8).reshape(-1).long().cpu()
            ei = torch.stack([ids, torch.arange(q.shape[0]).repeat_interleave(8)])
        else:
            rows = device_graph.query_lists(dec.decoder_strategy, q, grid, dec.gno_radius * scale, int(dec.k_neighbors))
            ei = torch.stack([rows.by_dst.other.long(), rows.by_dst.key.long()]).cpu()
        edges[f"decoder_edge_index_s{si}"] = ei
    return edges, tok


_REFS = {}


def _oracle_jac_vjp(key, model, cfg, lat, q, gy, gj):
    """-> (pred, jac, grad of sum(gy * pred) + sum(gj * jac) with respect to the latent, the same with gy = 0, the same with gj = 0):
    the fp64 oracle's decoder on the CPU on the lists the streamed routes use, differentiated in the query (create_graph=True, per
    output channel) and then in the latent; once per key"""
    if key in _REFS:
        return _REFS[key]
    edges, tok = _route_edges(model, cfg, lat, q)
    sd = {n: v.detach().double().cpu() for n, v in model.state_dict().items()}
    lat64 = lat.detach().double().cpu().requires_grad_(True)
    xg = q.detach().double().cpu().requires_grad_(True)
    p = orc.magno_decoder(sd, cfg.magno, lat64, xg, tok.double().cpu(), types.SimpleNamespace(**edges))
    jac = torch.stack([torch.autograd.grad(p[:, o].sum(), xg, create_graph=True)[0] for o in range(p.shape[1])], dim=1)
    (from_jac,) = torch.autograd.grad((jac * gj.double().cpu()).sum(), lat64, retain_graph=True)
    (from_pred,) = torch.autograd.grad((p * gy.double().cpu()).sum(), lat64)
    _REFS[key] = (p.detach(), jac.detach(), from_pred + from_jac, from_jac, from_pred)
    return _REFS[key]


def _keys_ok(seen, rows):
    keys = seen["keys"]
    fwd = "gno_fwd_jac_nh" if rows else "gno_fwd_knn_jac_nh"
    return (any(k.startswith("gno_adj_jac_nh") for k in keys) and any(k.startswith(fwd) for k in keys)
            and not any(k.startswith("gno_bwd") or k.startswith("gno_adj_nh") for k in keys))


@pytest.mark.parametrize("strategy", list(MODELS))
def test_sample_jacobian_vjp_meets_the_oracle_at_every_chunking(strategy, monkeypatch):
    key, (model, batch, tokens, cfg) = ag._model(strategy)
    q = hb._queries(batch)
    lat = ag._latent(model, batch, tokens)
    gy, gj = _cots(q.shape[0], 1)
    ref_p, ref_j, ref, ref_jac_only, ref_pred_only = _oracle_jac_vjp(key, model, cfg, lat, q, gy, gj)
    got = {}
    for chunk in CHUNKS:
        with hb._watch(monkeypatch) as seen:
            got[chunk] = model.sample_jacobian_vjp(lat, q, gy, gj, chunk_points=chunk)
        assert _keys_ok(seen, strategy != "knn"), seen
        assert got[chunk].shape == lat.shape and got[chunk].dtype == torch.float32
        assert not got[chunk].requires_grad and got[chunk].grad_fn is None
        hb.check(f"sample_jacobian_vjp/{strategy}/chunk{chunk}", got[chunk], ref)
        assert torch.equal(got[chunk], model.sample_jacobian_vjp(lat, q, gy, gj, chunk_points=chunk)), chunk     # reproducible
    peak = ref.abs().max().item()
    for chunk in CHUNKS[1:]:
        d = (got[chunk] - got[None]).abs().max().item()
        print(f"[chunking] sample_jacobian_vjp/{strategy}: chunk {chunk} against one piece: max |d| = {d:.3e} = {d / peak:.3e} of the peak {peak:.3e}")
        assert d <= 1e-5 * peak, (chunk, d, peak)
    with hb._precision("bf16"):
        assert torch.equal(model.sample_jacobian_vjp(lat, q, gy, gj, chunk_points=250), got[250])               # the same bits in both modes
    # a loss on the derivative alone
    hb.check(f"sample_jacobian_vjp/{strategy}/cot_pred_none", model.sample_jacobian_vjp(lat, q, None, gj, chunk_points=250), ref_jac_only)
    # cot_jac = 0 is sample_vjp
    zero = model.sample_jacobian_vjp(lat, q, gy, torch.zeros_like(gj), chunk_points=250)
    vjp = model.sample_vjp(lat, q, gy, chunk_points=250)
    peak0 = ref_pred_only.abs().max().item()
    d = (zero - vjp).abs().max().item()
    print(f"[value] sample_jacobian_vjp/{strategy}: cot_jac = 0 against sample_vjp: max |d| = {d:.3e} = {d / peak0:.3e} of the peak {peak0:.3e}")
    assert peak0 > 0 and d <= 1e-5 * peak0, (d, peak0)
    # a latent that requires grad: still outside autograd
    out = model.sample_jacobian_vjp(model.latent(batch, tokens), q[:100], gy[:100].contiguous(), gj[:100].contiguous())
    assert not out.requires_grad


@pytest.mark.parametrize("case", list(SHAPES))
def test_other_shapes_meet_the_oracle(case, monkeypatch):
    strategy, kw = SHAPES[case]
    kw = dict(kw)
    out = kw.pop("out", 1)
    key, (model, batch, tokens, cfg) = ag._model(strategy, out=out, **kw)
    q = hb._queries(batch, 150, 150)
    lat = ag._latent(model, batch, tokens)
    gy, gj = _cots(q.shape[0], out)
    ref_p, ref_j, ref, ref_jac_only, _ = _oracle_jac_vjp(key + "/150", model, cfg, lat, q, gy, gj)
    with hb._watch(monkeypatch) as seen:
        got = model.sample_jacobian_vjp(lat, q, gy, gj, chunk_points=128)
    assert _keys_ok(seen, strategy != "knn"), seen
    hb.check(f"sample_jacobian_vjp/{case}", got, ref)
    hb.check(f"sample_jacobian_vjp/{case}/cot_pred_none", model.sample_jacobian_vjp(lat, q, None, gj, chunk_points=128), ref_jac_only)


def test_a_relu_projection_meets_the_reference_written_out():
    """relu'' = 0: the projection cotangent's second term drops out; against tests/gno_jac_adj_ref.decoder_jac_vjp on the route's lists"""
    key, (model, batch, tokens, cfg) = ag._model("radius", out=2, scales=[1.0, 2.0], use_scale_weights=True)
    q = hb._queries(batch, 150, 150)
    lat = ag._latent(model, batch, tokens)
    gy, gj = _cots(q.shape[0], 2, seed=31)
    edges, tok = _route_edges(model, cfg, lat, q)
    lists = []
    for si in range(2):
        ei = edges[f"decoder_edge_index_s{si}"]
        rowptr = torch.zeros(q.shape[0] + 1, dtype=torch.int64)
        rowptr[1:] = torch.cumsum(torch.bincount(ei[1], minlength=q.shape[0]), 0)
        lists.append((ei[0].int(), ei[1].int(), rowptr.int()))
    sd = {n: v.detach().double().cpu() for n, v in model.state_dict().items()}
    model.decoder.projection.non_linearity = "relu"
    try:
        got = model.sample_jacobian_vjp(lat, q, gy, gj, chunk_points=128)
        pred, jac = model.sample_jacobian(lat, q, chunk_points=128, row_lists=True)
    finally:
        model.decoder.projection.non_linearity = "gelu"
    ref, ref_p, ref_j = JA.decoder_jac_vjp(sd, lists, tok, q, lat, gy, gj, True, act="relu")
    hb.check("sample_jacobian/relu/pred", pred, ref_p)
    hb.check("sample_jacobian/relu/jac", jac, ref_j)
    hb.check("sample_jacobian_vjp/relu", got, ref)


@pytest.mark.parametrize("strategy", list(MODELS))
def test_sample_jacobian_autograd_is_sample_jacobian_forward_and_its_vjp_backward(strategy):
    key, (model, batch, tokens, cfg) = ag._model(strategy)
    q = hb._queries(batch)
    lat = ag._latent(model, batch, tokens)
    gy, gj = _cots(q.shape[0], 1, seed=17)
    with torch.no_grad():
        p0, j0 = model.sample_jacobian(lat, q, chunk_points=250, row_lists=True)            # fp32 mode
    for mode in ("fp32", "bf16"):
        with hb._precision(mode):
            leaf = lat.clone().requires_grad_(True)
            pred, jac = model.sample_jacobian_autograd(leaf, q, chunk_points=250)
            assert pred.requires_grad and jac.requires_grad and torch.equal(pred.detach(), p0) and torch.equal(jac.detach(), j0), mode
            (grad,) = torch.autograd.grad((pred * gy).sum() + (jac * gj).sum(), leaf, retain_graph=True)
            assert torch.equal(grad, model.sample_jacobian_vjp(lat, q, gy, gj, chunk_points=250)), mode
            (grad,) = torch.autograd.grad((jac * gj).sum(), leaf, retain_graph=True)        # pred got no gradient: cot_pred = None
            assert torch.equal(grad, model.sample_jacobian_vjp(lat, q, None, gj, chunk_points=250)), mode
            (grad,) = torch.autograd.grad((pred * gy).sum(), leaf)                           # jac got none: a zero cotangent
            assert torch.equal(grad, model.sample_jacobian_vjp(lat, q, gy, torch.zeros_like(gj), chunk_points=250)), mode
    with pytest.raises(ValueError, match="query_pos requires grad"):
        model.sample_jacobian_autograd(lat.clone().requires_grad_(True), q.clone().requires_grad_(True))


@pytest.mark.parametrize("strategy", ["knn", "bidirectional"])
def test_a_normal_derivative_loss_reaches_an_encoder_parameter(strategy):
    """the loss sum(w * d pred / d n) through sample_jacobian_autograd + the autograd of model.latent, against the fp64 oracle of the
    whole model on the route's decoder lists, differentiated in the query and then in the parameter"""
    key, (model, batch, tokens, cfg) = ag._model(strategy)
    q = hb._queries(batch)
    gen = torch.Generator().manual_seed(37)
    n = torch.nn.functional.normalize(torch.randn(q.shape[0], 3, generator=gen), dim=1).to(DEV)
    w = torch.randn(q.shape[0], 1, generator=gen).to(DEV)
    name = "encoder.gno.channel_mlp.fcs.0.weight"
    param = dict(model.named_parameters())[name]
    pred, jac = model.sample_jacobian_autograd(model.latent(batch, tokens), q, chunk_points=250)
    (got,) = torch.autograd.grad(((jac * n[:, None, :]).sum(-1) * w).sum(), param)
    edges, tok = _route_edges(model, cfg, ag._latent(model, batch, tokens), q)
    sd = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    sd[name].requires_grad_(True)
    b64 = cg._batch64(batch.to("cpu"))
    for k, v in edges.items():
        setattr(b64, k, v)
    xg = q.detach().double().cpu().requires_grad_(True)
    p = orc.gaot3d_forward(sd, cfg, b64, tok.double().cpu(), query_coord_pos=xg)
    (dq,) = torch.autograd.grad(p.sum(), xg, create_graph=True)                             # out = 1: d pred[q, 0] / d q
    (ref,) = torch.autograd.grad(((dq * n.double().cpu()).sum(-1, keepdim=True) * w.double().cpu()).sum(), sd[name])
    hb.check(f"sample_jacobian_autograd/{strategy}/normal_derivative/encoder_parameter", got, ref)


@pytest.mark.parametrize("strategy", ["knn", "radius"])
def test_nothing_sized_by_the_queries_survives_the_call(strategy):
    key, (model, batch, tokens, cfg) = ag._model(strategy)
    gen = torch.Generator().manual_seed(23)
    q = (torch.rand(20000, 3, generator=gen) * 2.4 - 1.2).to(DEV)
    lat = ag._latent(model, batch, tokens)
    gy, gj = _cots(q.shape[0], 1)
    model.sample_jacobian_vjp(lat, q[:2000].contiguous(), gy[:2000].contiguous(), gj[:2000].contiguous(), chunk_points=1000)   # the grid, the allocator
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    out = model.sample_jacobian_vjp(lat, q, gy, gj, chunk_points=4096)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - m0
    assert grown <= (out.numel() * 4 + 511) // 512 * 512, grown                             # back to the start plus the [M, C] result


@pytest.mark.parametrize("case", list(ag.REFUSALS))
def test_other_configurations_are_refused_before_any_launch(case):
    from gaot_3d_amd import ops
    strategy, k, kw, msg = ag.REFUSALS[case]
    model, batch, tokens, cfg = hb._setup(f"adjoint/refuse/{case}", k=k, **MODELS[strategy], **kw)
    lat = ag._latent(model, batch, tokens)
    q = batch.pos[:200].contiguous()
    gy, gj = _cots(200, 1)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    with pytest.raises(NotImplementedError, match="adjoint of the field's Jacobian.*" + msg):
        model.sample_jacobian_vjp(lat, q, gy, gj)
    with pytest.raises(NotImplementedError, match="adjoint of the field's Jacobian.*" + msg):
        model.sample_jacobian_autograd(lat.clone().requires_grad_(True), q)
    assert ops.launch_count() == n0


def test_argument_rules_raise_on_the_device():
    from gaot_3d_amd import ops
    key, (model, batch, tokens, cfg) = ag._model("knn")
    lat = ag._latent(model, batch, tokens)
    q = batch.pos[:100].contiguous()
    gy, gj = _cots(100, 1)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    for bad in (gy.double(), gy.cpu(), gy[:50], torch.zeros(100, 2, device=DEV), torch.zeros(100, device=DEV)):
        with pytest.raises(ValueError, match="cot_pred"):
            model.sample_jacobian_vjp(lat, q, bad, gj)
    for bad in (gj.double(), gj.cpu(), gj[:50], torch.zeros(100, 1, 2, device=DEV), torch.zeros(100, 3, device=DEV), None):
        with pytest.raises(ValueError, match="cot_jac"):
            model.sample_jacobian_vjp(lat, q, gy, bad)
    with pytest.raises(ValueError, match="chunk_points"):
        model.sample_jacobian_vjp(lat, q, gy, gj, chunk_points=0)
    model.decoder.decoder_strategy = "reverse"
    try:
        with pytest.raises(ValueError, match="reverse"):
            model.sample_jacobian_vjp(lat, q, gy, gj)
        with pytest.raises(ValueError, match="reverse"):
            model.sample_jacobian_autograd(lat, q)
    finally:
        model.decoder.decoder_strategy = "knn"
    model.decoder._shard_group = object()
    try:
        with pytest.raises(NotImplementedError, match="point-sharded"):
            model.sample_jacobian_vjp(lat, q, gy, gj)
    finally:
        del model.decoder._shard_group
    model.decoder.projection.non_linearity = "silu"                                        # in ops.ACT, but without a second derivative here
    try:
        with pytest.raises(NotImplementedError, match="second derivative.*'silu'"):
            model.sample_jacobian_vjp(lat, q, gy, gj)
        with pytest.raises(NotImplementedError, match="second derivative.*'silu'"):
            model.sample_jacobian_autograd(lat.clone().requires_grad_(True), q)
    finally:
        model.decoder.projection.non_linearity = "gelu"
    assert ops.launch_count() == n0
    tok = model._tokens(1, q.device, None, None)[0]
    with pytest.raises(NotImplementedError, match="do not stream"):                         # tokens off the regular grid
        model.sample_jacobian_vjp(lat, q, gy, gj, tokens_pos=(tok + 0.01 * torch.rand_like(tok)))


def test_in_a_capture_the_row_route_raises_before_any_launch():
    from gaot_3d_amd import ops
    from gaot_3d_amd._lib import GaotError
    key, (model, batch, tokens, cfg) = ag._model("bidirectional")
    q = batch.pos[:300].contiguous()
    lat = ag._latent(model, batch, tokens)
    gy, gj = _cots(300, 1)
    eager = model.sample_jacobian_vjp(lat, q, gy, gj)            # describes the grid, warms the allocator
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(GaotError, match="captured"):
        with torch.cuda.graph(graph):
            model.sample_jacobian_vjp(lat, q, gy, gj)
    assert ops.launch_count() == n0
    torch.cuda.synchronize()
    assert torch.equal(model.sample_jacobian_vjp(lat, q, gy, gj), eager)
