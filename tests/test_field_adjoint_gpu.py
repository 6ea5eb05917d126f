"""The adjoint of the sampled field: gaot_gno_adj (the linear transform's adjoint with respect to f_y -- the forward kernel on the
by-SOURCE list, reduced by token), ops.gno_adjoint, graph.by_source, IntegralTransform.adjoint_knn / adjoint_rows,
MAGNODecoder / GAOT3D.sample_vjp and GAOT3D.sample_autograd (functional.SampleLatentFn).

Bars: the project's fp32 bar for derivatives (tests/test_coord_grad_gpu.py FP32_BAR: max error <= 1e-3 of the reference's peak,
cosine >= 0.99999), every peak asserted > 0; references in fp64 on the CPU (tests/gno_adj_ref.py, oracle/gaot_oracle.py).

  * op level (211 sources, 'linear', 1..4 hidden layers): regular lists Nq in {1, 7, 33, 1000} x k in {1, 4, 8, 32} with repeats --
    the bar against fp64; beside ops.gno_backward(precision=0)'s grad_f_y on build_graph of the same lists (1..3 hidden layers: the
    exact-fp32 backward has no four-layer instantiation), both sum the same fp32 terms in different orders: the new kernel's distance
    to fp64 is at most max(4 x the existing kernel's, 1e-6 of the peak); the adjoint identity <g, A f> = <A^T g, f> within 1e-3 of
    sum |terms|;
  * rows that can go wrong, built by hand: sources without an edge (exact zeros over a NaN pre-fill), 200 queries on one token (a row
    over seven 32-edge tiles), a row that ends and a row that starts exactly on a tile boundary with E no multiple of 32, E = 0 (the
    fix-up alone), zero queries;
  * the ragged by-query lists a-e of tests/test_field_jacobian_rows_gpu.py with empty query rows (1/deg from rowptr_dst); on a regular
    list the k form is torch.equal to the rowptr_dst form; two calls are torch.equal; bf16 mode is torch.equal; two launches per
    call; bad operands raise GaotError with the launch count unchanged; by_source is csr_build of the explicit edge_index;
  * model level (4096 points, latent 8 x 8 x 8, k = 8, 'knn' / 'radius' / 'bidirectional' with r = 0.45; 300 sample points and 300 random
    queries partly outside the box): sample_vjp with a random cotangent against torch.autograd.grad of the fp64 oracle's decoder on the
    lists actually used; four output channels, two scales weighted and summed, four hidden layers; chunkings None / 250 / 64 meet the
    bar, agree within 1e-5 of the peak and are reproducible bit for bit; sample_autograd's forward is sample's in fp32 mode,
    its backward is sample_vjp bit for bit, and chained through model.latent it meets forward(query_coord_pos=...)'s gradients of an
    encoder parameter and of batch.pos at the bar; timing keys; memory; refusals; the capture error on a row route.

Measured on an MI355X: kernel against fp64 at most 4.8e-7 of the peak (gno_bwd on the same lists: 5.0e-7), hand-built and ragged rows
4.9e-7; the adjoint identity to 1.7e-8 of sum |terms|; sample_vjp against the oracle 3.1e-7 - 5.6e-7 of the peak; chunkings 6.3e-8 -
2.6e-7 of the peak apart; chained gradients 6.5e-7 (encoder weight) and 8.2e-7 (batch.pos) of the peak from forward's."""
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
import gno_rows_jac_ref as JREF  # noqa: E402  (ragged_list)
import test_field_hessian_gpu as hb  # noqa: E402  (the model fixture with its config, the watcher, check(), the bar, the queries)
import test_field_jacobian_rows_gpu as jr  # noqa: E402  (the lists a-e, the device operands, the row-list decoders)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NSRC = jr.NSRC
FP32_BAR = hb.FP32_BAR
NQS = (1, 7, 33, 1000)
KS = (1, 4, 8, 32)


def _regular(nq, k, gen):
    """a regular list with random sources (repeats allowed) as (src, dst, rowptr) and the query coordinates / cotangent"""
    src = torch.randint(0, NSRC, (nq * k,), generator=gen).int()
    dst = torch.arange(nq).repeat_interleave(k).int()
    rowptr = (torch.arange(nq + 1) * k).int()
    x = torch.rand(nq, 3, generator=gen) * 2 - 1
    g = torch.randn(nq, 32, generator=gen)
    return src, dst, rowptr, x, g


def _both_lists(src, dst, nq, nsrc=NSRC):
    from gaot_3d_amd import ops
    return ops.build_graph(torch.stack([src, dst]).to(DEV), nsrc, nq)


def _dist(got, ref):
    return (got.detach().double().cpu() - ref).abs().max().item()


# ---- op level: regular lists ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh", [1, 2, 3, 4])
def test_regular_lists_meet_fp64_the_backward_kernel_and_the_adjoint_identity(nh):
    from gaot_3d_amd import graph, ops
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(nh, "linear")
    worst_identity = 0.0
    for nq in NQS:
        for k in KS:
            src, dst, rowptr, x, g = _regular(nq, k, gen)
            xd, gd, nbr = x.to(DEV), g.to(DEV), src.to(DEV)
            gs = graph.by_source((nbr, k), NSRC)
            n0 = ops.launch_count()
            got = ops.gno_adjoint(wd, bd, yd, xd, gd, gs, k)
            assert ops.launch_count() == n0 + 2, (nq, k)                                   # the kernel and its fix-up
            assert got.shape == (NSRC, 32) and got.dtype == torch.float32
            ref = REF.gno_adjoint_closed(ws, bs, y, x, src, dst, rowptr, g, NSRC)
            hb.check(f"gno_adj/nh{nh}/nq{nq}/k{k}", got, ref, quiet=True)
            peak = ref.abs().max().item()
            d_new = _dist(got, ref)
            if nh <= 3:                                  # the exact-fp32 backward kernel exists for 1..3 hidden layers
                old = ops.gno_backward(wd, bd, yd, xd, fd, gd, _both_lists(src, dst, nq), precision=0)[0]
                d_old = _dist(old, ref)
                print(f"[adjoint] nh{nh} nq{nq} k{k}: |adj - fp64| = {d_new:.3e}, |gno_bwd - fp64| = {d_old:.3e}, peak {peak:.3e}")
                assert d_new <= max(4.0 * d_old, 1e-6 * peak), (nq, k, d_new, d_old, peak)
            # <g, A f> against <A^T g, f>, both dot products in fp64
            out = ops.gno_forward_knn("linear", wd, bd, yd, xd, fd, None, nbr, k, precision=0)
            lhs = (g.double() * out.double().cpu()).sum().item()
            rhs = (got.double().cpu() * f.double()).sum().item()
            scale = (REF.adjoint_terms(ws, bs, y, x, src, dst, rowptr, g) * f.double()[src.long()]).abs().sum().item()
            assert scale > 0
            worst_identity = max(worst_identity, abs(lhs - rhs) / scale)
            assert abs(lhs - rhs) <= 1e-3 * scale, (nq, k, lhs, rhs, scale)
    print(f"[adjoint] nh{nh}: worst |<g, A f> - <A^T g, f>| / sum|terms| = {worst_identity:.3e}")


def _raw_adjoint(wd, bd, yd, xd, gd, g, k, fill):
    """gaot_gno_adj through the C ABI into a result pre-filled with ``fill``"""
    from gaot_3d_amd import _lib, ops
    lib = _lib.load()
    m, keep = ops._mlp_struct(wd, bd)
    out = torch.full((g.num_src, 32), fill, dtype=torch.float32, device=DEV)
    e = g.by_src.num_edges
    ws = ops._ws(lib.gaot_gno_adj_workspace_bytes(e, 32), DEV)
    rc = lib.gaot_gno_adj(C.byref(m), ops._ptr(yd), ops._ptr(xd), ops._ptr(gd), ops._ptr(None if k else g.by_dst.rowptr), int(k or 0),
                          ops._ptr(g.by_src.key), ops._ptr(g.by_src.other), ops._ptr(g.by_src.rowptr), e, g.num_src, g.num_dst,
                          ops._ptr(out), ops._ptr(ws), ws.numel(), ops._stream())
    assert rc == 0, _lib.load().gaot_last_error()
    return out


def _hand_lists(gen):
    """by-query lists whose by-SOURCE rows are the shapes that can go wrong: {name: (src, dst, nq)} with dst ascending"""
    lists = {}
    # 200 queries on token 7 (its row spans seven 32-edge tiles) among 20 queries of three tokens from [100, 150)
    src = torch.cat([torch.full((200,), 7), torch.randint(100, 150, (60,), generator=gen)])
    dst = torch.cat([torch.arange(200), 200 + torch.arange(20).repeat_interleave(3)])
    lists["long_row"] = (src.int(), dst.int(), 220)
    # source rows of 32, 10, 22 and 5 edges: row 0 ends and row 1 starts on a tile boundary, row 2 ends on the next, E = 69
    src = torch.tensor([0] * 32 + [1] * 10 + [2] * 22 + [3] * 5)
    dst = torch.randint(0, 40, (69,), generator=gen)
    order = torch.argsort(dst, stable=True)
    lists["tile_boundaries"] = (src[order].int(), dst[order].int(), 40)
    return lists


@pytest.mark.parametrize("nh", [1, 2, 3, 4])
def test_row_shapes_built_by_hand(nh):
    from gaot_3d_amd import ops
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(nh, "linear")
    for name, (src, dst, nq) in _hand_lists(gen).items():
        assert src.numel() % 32 != 0
        x = torch.rand(nq, 3, generator=gen) * 2 - 1
        g = torch.randn(nq, 32, generator=gen)
        gr = _both_lists(src, dst, nq)
        rs = gr.by_src.rowptr.cpu()
        if name == "long_row":
            assert int(rs[8] - rs[7]) == 200 and (int(rs[8]) - 1) // 32 - int(rs[7]) // 32 >= 5
        else:
            assert rs[:5].tolist() == [0, 32, 42, 64, 69]
        got = _raw_adjoint(wd, bd, yd, x.to(DEV), g.to(DEV), gr, None, float("nan"))
        ref = REF.gno_adjoint_closed(ws, bs, y, x, src, dst, gr.by_dst.rowptr.cpu(), g, NSRC)
        assert not torch.isnan(got).any(), name
        unused = torch.ones(NSRC, dtype=torch.bool)
        unused[src.long()] = False
        assert unused.any() and torch.equal(got[unused.to(DEV)], torch.zeros(int(unused.sum()), 32, device=DEV)), name
        hb.check(f"gno_adj/nh{nh}/{name}", got, ref)
        assert torch.equal(got, ops.gno_adjoint(wd, bd, yd, x.to(DEV), g.to(DEV), gr)), name


def test_no_edges_and_no_queries():
    from gaot_3d_amd import graph, ops
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(2, "linear")
    empty = lambda: torch.empty(0, dtype=torch.int32, device=DEV)
    for nq in (5, 0):
        rows = ops.BipartiteGraph(ops.SortedEdges(torch.zeros(nq + 1, dtype=torch.int32, device=DEV), None, empty(), empty(), nq),
                                  None, NSRC, nq)
        gr = graph.by_source(rows, NSRC)
        assert gr.by_src.num_edges == 0 and gr.num_dst == nq and torch.equal(gr.by_src.rowptr, torch.zeros(NSRC + 1, dtype=torch.int32, device=DEV))
        xd, gd = torch.zeros(nq, 3, device=DEV), torch.ones(nq, 32, device=DEV)
        n0 = ops.launch_count()
        got = ops.gno_adjoint(wd, bd, yd, xd, gd, gr)
        assert ops.launch_count() == n0 + 1                                                # the fix-up alone writes the zeros
        assert torch.equal(got, torch.zeros(NSRC, 32, device=DEV))
        got = _raw_adjoint(wd, bd, yd, xd, gd, gr, None, float("nan"))
        assert torch.equal(got, torch.zeros(NSRC, 32, device=DEV))
    gr = graph.by_source((empty(), 8), NSRC)                                               # zero queries of a regular list
    assert torch.equal(ops.gno_adjoint(wd, bd, yd, torch.zeros(0, 3, device=DEV), torch.zeros(0, 32, device=DEV), gr, 8),
                       torch.zeros(NSRC, 32, device=DEV))


@pytest.mark.parametrize("nh", [1, 2, 3, 4])
def test_ragged_lists_take_the_degree_from_rowptr_dst(nh):
    from gaot_3d_amd import graph, ops
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(nh, "linear")
    for name, deg in jr.DEGREES.items():
        nq = len(deg)
        x = torch.rand(nq, 3, generator=gen) * 2 - 1
        g = torch.randn(nq, 32, generator=gen)
        src, dst, rowptr = JREF.ragged_list(deg, NSRC, gen)
        rows = jr._graph(src, dst, rowptr, NSRC)                                           # the forward-only graph query_lists returns
        gr = graph.by_source(rows, NSRC)
        assert gr.by_dst is rows.by_dst
        both = _both_lists(src, dst, nq)
        for a, b in ((gr.by_src.rowptr, both.by_src.rowptr), (gr.by_src.key, both.by_src.key), (gr.by_src.other, both.by_src.other)):
            assert torch.equal(a, b), name                                                 # by_source IS csr_build of the edge_index
        xd, gd = x.to(DEV), g.to(DEV)
        n0 = ops.launch_count()
        got = ops.gno_adjoint(wd, bd, yd, xd, gd, gr)
        assert ops.launch_count() == n0 + 2, name
        ref = REF.gno_adjoint_closed(ws, bs, y, x, src, dst, rowptr, g, NSRC)
        hb.check(f"gno_adj/nh{nh}/list_{name}", got, ref)
        assert torch.equal(got, ops.gno_adjoint(wd, bd, yd, xd, gd, gr)), name             # reproducible
        with hb._precision("bf16"):
            assert torch.equal(got, ops.gno_adjoint(wd, bd, yd, xd, gd, gr)), name         # exact fp32 in both modes


def test_on_a_regular_list_k_and_rowptr_dst_agree_bit_for_bit():
    from gaot_3d_amd import graph, ops
    for nh in (1, 2, 3, 4):
        gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(nh, "linear")
        for nq, k in ((7, 4), (33, 32), (1000, 8), (33, 1)):
            src, dst, rowptr, x, g = _regular(nq, k, gen)
            xd, gd = x.to(DEV), g.to(DEV)
            by_k = ops.gno_adjoint(wd, bd, yd, xd, gd, graph.by_source((src.to(DEV), k), NSRC), k)
            by_rowptr = ops.gno_adjoint(wd, bd, yd, xd, gd, graph.by_source(jr._graph(src, dst, rowptr, NSRC), NSRC))
            assert torch.equal(by_k, by_rowptr), (nh, nq, k)
            assert torch.equal(by_k, ops.gno_adjoint(wd, bd, yd, xd, gd, _both_lists(src, dst, nq))), (nh, nq, k)


def test_by_source_of_both_kinds_of_list_is_csr_build_of_the_edge_index():
    from gaot_3d_amd import graph, ops
    gen = torch.Generator().manual_seed(5)
    src, dst, rowptr, x, g = _regular(33, 8, gen)
    ei = torch.stack([src, dst]).to(DEV)
    want = ops.csr_build(ei, 0, NSRC)
    for lists in ((src.to(DEV), 8), (src.to(DEV).view(33, 8), 8), jr._graph(src, dst, rowptr, NSRC)):
        got = graph.by_source(lists, NSRC)
        assert got.num_src == NSRC and got.num_dst == 33
        assert torch.equal(got.by_src.rowptr, want.rowptr) and torch.equal(got.by_src.key, want.key) and torch.equal(got.by_src.other, want.other)
        rp = got.by_src.rowptr.cpu()
        oth = got.by_src.other.cpu()
        assert all(bool((oth[rp[t]:rp[t + 1]][1:] >= oth[rp[t]:rp[t + 1]][:-1]).all()) for t in range(NSRC))   # queries ascending


def test_bad_operands_raise_before_any_launch():
    from gaot_3d_amd import graph, ops
    from gaot_3d_amd._lib import GaotError
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(2, "linear")
    src, dst, rowptr, x, g = _regular(33, 8, gen)
    xd, gd = x.to(DEV), g.to(DEV)
    gr = graph.by_source((src.to(DEV), 8), NSRC)
    rows = jr._graph(src, dst, rowptr, NSRC)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    bad = [
        lambda: ops.gno_adjoint(wd, bd, yd, xd, gd[:, :16].contiguous(), gr, 8),           # cotangent channels
        lambda: ops.gno_adjoint(wd, bd, yd, xd, gd[:20].contiguous(), gr, 8),              # cotangent rows
        lambda: ops.gno_adjoint(wd, bd, yd, xd, gd.double(), gr, 8),                       # dtype
        lambda: ops.gno_adjoint(wd, bd, yd, xd, gd.cpu(), gr, 8),                          # host tensor
        lambda: ops.gno_adjoint(wd, bd, yd[:100].contiguous(), xd, gd, gr, 8),             # source rows
        lambda: ops.gno_adjoint(wd, bd, yd, xd[:, :2].contiguous(), gd, gr, 8),            # coordinates
        lambda: ops.gno_adjoint(wd, bd, yd, xd, gd, gr),                                   # neither rowptr_dst nor k
        lambda: ops.gno_adjoint(wd, bd, yd, xd, gd, gr, 4),                                # k that does not match the list
        lambda: ops.gno_adjoint(wd, bd, yd, xd, gd, gr, 0),
        lambda: ops.gno_adjoint(wd, bd, yd, xd, gd, rows),                                 # no by-source list
        lambda: ops.gno_adjoint(wd[:1], bd[:1], yd, xd, gd, gr, 8),                        # one linear layer
        lambda: ops.gno_adjoint([wd[0][:32].contiguous(), wd[1][:32, :32].contiguous(), wd[2][:, :32].contiguous()],
                                [bd[0][:32].contiguous(), bd[1][:32].contiguous(), bd[2]], yd, xd, gd, gr, 8),   # hidden width 32
        lambda: graph.by_source((src.to(DEV).long(), 8), NSRC),
        lambda: graph.by_source((src.to(DEV), 5), NSRC),
        lambda: graph.by_source(rows, NSRC + 1),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(GaotError):
            call()
        assert ops.launch_count() == n0, i


# ---- model level ------------------------------------------------------------------------------------------------------------------------
CHUNKS = (None, 250, 64)
MODELS = {
    "knn": dict(),
    "radius": dict(jr.DECODERS["radius"]),
    "bidirectional": dict(jr.DECODERS["bidirectional"]),
}
SHAPES = {
    "four_channels": ("knn", dict(out=4)),
    "four_channels_radius": ("radius", dict(out=4)),
    "two_scales_weighted": ("knn", dict(out=2, scales=[1.0, 2.0], use_scale_weights=True)),
    "two_scales_weighted_radius": ("radius", dict(out=2, scales=[1.0, 2.0], use_scale_weights=True)),
    "two_scales_summed": ("knn", dict(scales=[1.0, 2.0], use_scale_weights=False)),
    "two_scales_summed_bidirectional": ("bidirectional", dict(scales=[1.0, 2.0], use_scale_weights=False)),
    "four_layers": ("knn", dict(out_gno_channel_mlp_hidden_layers=[64, 64, 64, 64])),
    "four_layers_bidirectional": ("bidirectional", dict(out_gno_channel_mlp_hidden_layers=[64, 64, 64, 64])),
}


def _model(strategy, out=1, **more):
    key = f"adjoint/{strategy}/out{out}/" + ",".join(f"{a}={b}" for a, b in sorted(more.items()))
    return key, hb._setup(key, k=8, out=out, **MODELS[strategy], **more)


def _latent(model, batch, tokens):
    with torch.no_grad():
        return model.latent(batch, tokens)


def _cotangent(nq, out, seed=13):
    return torch.randn(nq, out, generator=torch.Generator().manual_seed(seed)).to(DEV)


_REFS = {}


def _oracle_vjp(key, model, cfg, lat, q, g):
    """grad of sum(g * decoder(latent)) with respect to the latent, by fp64 autograd of the oracle's decoder on the CPU, on the edges
    of the lists the streamed routes use (knn_to_grid's ids, or graph.query_lists per scale); once per key"""
    if key in _REFS:
        return _REFS[key]
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
    sd = {n: v.detach().double().cpu() for n, v in model.state_dict().items()}
    lat64 = lat.detach().double().cpu().requires_grad_(True)
    p = orc.magno_decoder(sd, cfg.magno, lat64, q.detach().double().cpu(), tok.double().cpu(), types.SimpleNamespace(**edges))
    (ref,) = torch.autograd.grad((p * g.double().cpu()).sum(), lat64)
    _REFS[key] = (p.detach(), ref)
    return _REFS[key]


def _adjoint_keys(seen, rows):
    keys = seen["keys"]
    fwd = "gno_fwd_nh" if rows else "gno_fwd_knn_nh"
    return (any(k.startswith("gno_adj_nh") for k in keys) and any(k.startswith(fwd) for k in keys)
            and all(k.startswith("gno_adj_nh") or k.startswith(fwd) for k in keys) and not any(k.startswith("gno_bwd") for k in keys))


@pytest.mark.parametrize("strategy", list(MODELS))
def test_sample_vjp_meets_the_oracle_at_every_chunking(strategy, monkeypatch):
    key, (model, batch, tokens, cfg) = _model(strategy)
    q = hb._queries(batch)
    lat = _latent(model, batch, tokens)
    g = _cotangent(q.shape[0], 1)
    ref_p, ref = _oracle_vjp(key, model, cfg, lat, q, g)
    got = {}
    for chunk in CHUNKS:
        with hb._watch(monkeypatch) as seen:
            got[chunk] = model.sample_vjp(lat, q, g, chunk_points=chunk)
        assert _adjoint_keys(seen, strategy != "knn"), seen
        assert got[chunk].shape == lat.shape and got[chunk].dtype == torch.float32
        assert not got[chunk].requires_grad and got[chunk].grad_fn is None
        hb.check(f"sample_vjp/{strategy}/chunk{chunk}", got[chunk], ref)
        assert torch.equal(got[chunk], model.sample_vjp(lat, q, g, chunk_points=chunk)), chunk        # reproducible
    peak = ref.abs().max().item()
    for chunk in CHUNKS[1:]:
        d = (got[chunk] - got[None]).abs().max().item()
        print(f"[chunking] sample_vjp/{strategy}: chunk {chunk} against one piece: max |d| = {d:.3e} = {d / peak:.3e} of the peak {peak:.3e}")
        assert d <= 1e-5 * peak, (chunk, d, peak)
    with hb._precision("bf16"):
        assert torch.equal(model.sample_vjp(lat, q, g, chunk_points=250), got[250])                   # the same bits in both modes
    # a latent that requires grad: still outside autograd
    out = model.sample_vjp(model.latent(batch, tokens), q[:100], g[:100].contiguous())
    assert not out.requires_grad


@pytest.mark.parametrize("case", list(SHAPES))
def test_other_shapes_meet_the_oracle(case, monkeypatch):
    strategy, kw = SHAPES[case]
    kw = dict(kw)
    out = kw.pop("out", 1)
    key, (model, batch, tokens, cfg) = _model(strategy, out=out, **kw)
    q = hb._queries(batch, 150, 150)
    lat = _latent(model, batch, tokens)
    g = _cotangent(q.shape[0], out)
    ref_p, ref = _oracle_vjp(key, model, cfg, lat, q, g)
    with hb._watch(monkeypatch) as seen:
        got = model.sample_vjp(lat, q, g, chunk_points=128)
    assert _adjoint_keys(seen, strategy != "knn"), seen
    hb.check(f"sample_vjp/{case}", got, ref)


@pytest.mark.parametrize("strategy", list(MODELS))
def test_sample_autograd_is_sample_forward_and_sample_vjp_backward(strategy):
    key, (model, batch, tokens, cfg) = _model(strategy)
    q = hb._queries(batch)
    lat = _latent(model, batch, tokens)
    w = _cotangent(q.shape[0], 1, seed=17)
    with torch.no_grad():
        smp = model.sample(lat, q, chunk_points=250)                                       # fp32 mode
    for mode in ("fp32", "bf16"):
        with hb._precision(mode):
            leaf = lat.clone().requires_grad_(True)
            pred = model.sample_autograd(leaf, q, chunk_points=250)
            assert pred.requires_grad and torch.equal(pred.detach(), smp), mode
            (grad,) = torch.autograd.grad((pred * w).sum(), leaf)
            assert torch.equal(grad, model.sample_vjp(lat, q, w, chunk_points=250)), mode
    with pytest.raises(ValueError, match="query_pos requires grad"):
        model.sample_autograd(lat.clone().requires_grad_(True), q.clone().requires_grad_(True))


@pytest.mark.parametrize("strategy", ["knn", "bidirectional"])
def test_chained_through_the_latent_it_meets_the_route_it_replaces(strategy):
    """the loss sum(w * pred) reaches an encoder parameter and batch.pos through sample_autograd + the autograd of model.latent, and
    through forward(query_coord_pos=q) -- edge list, decoder graph, gno_bwd -- with the same values at the fp32 bar"""
    key, (model, batch, tokens, cfg) = _model(strategy)
    q = hb._queries(batch)
    w = _cotangent(q.shape[0], 1, seed=19)
    param = model.encoder.gno.channel_mlp.fcs[0].weight
    b2 = copy.copy(batch)
    b2.pos = batch.pos.detach().clone().requires_grad_(True)
    model.decoder.precompute_edges = False
    try:
        p_ref = model(b2, tokens, query_coord_pos=q, query_coord_batch_idx=torch.zeros(q.shape[0], dtype=torch.long, device=DEV))
    finally:
        model.decoder.precompute_edges = True
    ref_param, ref_pos = torch.autograd.grad((p_ref * w).sum(), [param, b2.pos])
    b3 = copy.copy(batch)
    b3.pos = batch.pos.detach().clone().requires_grad_(True)
    pred = model.sample_autograd(model.latent(b3, tokens), q, chunk_points=250)
    got_param, got_pos = torch.autograd.grad((pred * w).sum(), [param, b3.pos])
    assert torch.allclose(pred.detach(), p_ref.detach(), rtol=1e-4, atol=1e-5)
    hb.check(f"sample_autograd/{strategy}/encoder_parameter", got_param, ref_param.double().cpu())
    hb.check(f"sample_autograd/{strategy}/batch_pos", got_pos, ref_pos.double().cpu())


@pytest.mark.parametrize("strategy", ["knn", "radius"])
def test_nothing_sized_by_the_queries_survives_the_call(strategy):
    key, (model, batch, tokens, cfg) = _model(strategy)
    gen = torch.Generator().manual_seed(23)
    q = (torch.rand(20000, 3, generator=gen) * 2.4 - 1.2).to(DEV)
    lat = _latent(model, batch, tokens)
    g = _cotangent(q.shape[0], 1)
    model.sample_vjp(lat, q[:2000].contiguous(), g[:2000].contiguous(), chunk_points=1000)           # the grid's description, the allocator
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    out = model.sample_vjp(lat, q, g, chunk_points=4096)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - m0
    assert grown <= (out.numel() * 4 + 511) // 512 * 512, grown                             # back to the start plus the [M, C] result


REFUSALS = {
    "use_attn": ("knn", 8, dict(use_attn=True), "use_attn"),
    "geoembed": ("knn", 8, dict(use_geoembed=[True, True], embedding_method="pointnet"), "GeoEmbed"),
    "k3": ("knn", 3, {}, "k_neighbors = 3"),
    "nonlinear": ("knn", 8, dict(out_gno_transform_type="nonlinear"), "'nonlinear'"),
    "kernelonly_radius": ("radius", 8, dict(out_gno_transform_type="nonlinear_kernelonly"), "nonlinear_kernelonly"),
    "use_attn_radius": ("radius", 8, dict(use_attn=True), "on row lists.*use_attn"),
    "bidirectional_k64": ("bidirectional", 64, {}, "k_neighbors = 64"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_other_configurations_are_refused_before_any_launch(case):
    from gaot_3d_amd import ops
    strategy, k, kw, msg = REFUSALS[case]
    key = f"adjoint/refuse/{case}"
    model, batch, tokens, cfg = hb._setup(key, k=k, **MODELS[strategy], **kw)
    lat = _latent(model, batch, tokens)
    q = batch.pos[:200].contiguous()
    g = _cotangent(200, 1)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    with pytest.raises(NotImplementedError, match="adjoint of the sampled field.*" + msg):
        model.sample_vjp(lat, q, g)
    with pytest.raises(NotImplementedError, match="adjoint of the sampled field.*" + msg):
        model.sample_autograd(lat.clone().requires_grad_(True), q)
    assert ops.launch_count() == n0


def test_argument_rules_raise_on_the_device():
    from gaot_3d_amd import ops
    key, (model, batch, tokens, cfg) = _model("knn")
    lat = _latent(model, batch, tokens)
    q = batch.pos[:100].contiguous()
    g = _cotangent(100, 1)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    for bad in (g.double(), g.cpu(), g[:50], torch.zeros(100, 2, device=DEV), torch.zeros(100, device=DEV)):
        with pytest.raises(ValueError, match="cotangent"):
            model.sample_vjp(lat, q, bad)
    with pytest.raises(ValueError, match="chunk_points"):
        model.sample_vjp(lat, q, g, chunk_points=0)
    model.decoder.decoder_strategy = "reverse"
    try:
        with pytest.raises(ValueError, match="reverse"):
            model.sample_vjp(lat, q, g)
        with pytest.raises(ValueError, match="reverse"):
            model.sample_autograd(lat, q)
    finally:
        model.decoder.decoder_strategy = "knn"
    model.decoder._shard_group = object()
    try:
        with pytest.raises(NotImplementedError, match="point-sharded"):
            model.sample_vjp(lat, q, g)
    finally:
        del model.decoder._shard_group
    assert ops.launch_count() == n0
    tok = model._tokens(1, q.device, None, None)[0]
    with pytest.raises(NotImplementedError, match="do not stream"):                         # tokens off the regular grid
        model.sample_vjp(lat, q, g, tokens_pos=(tok + 0.01 * torch.rand_like(tok)))


def test_in_a_capture_the_row_route_raises_before_any_launch():
    from gaot_3d_amd import ops
    from gaot_3d_amd._lib import GaotError
    key, (model, batch, tokens, cfg) = _model("bidirectional")
    q = batch.pos[:300].contiguous()
    lat = _latent(model, batch, tokens)
    g = _cotangent(300, 1)
    eager = model.sample_vjp(lat, q, g)                          # describes the grid, warms the allocator
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(GaotError, match="captured"):
        with torch.cuda.graph(graph):
            model.sample_vjp(lat, q, g)
    assert ops.launch_count() == n0
    torch.cuda.synchronize()
    assert torch.equal(model.sample_vjp(lat, q, g), eager)
