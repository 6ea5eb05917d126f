"""GPU: the adjoint of the field's directional derivatives and Hessian -- gaot_gno_adj_jet2_qd (ops.gno_adjoint_jet2_qd),
gaot_mlp2_jet2_cot_mid (ops.mlp2_jet2_cot_mid), IntegralTransform.adjoint_jet2_knn_qd / adjoint_jet2_rows_qd, MAGNODecoder /
GAOT3D.sample_directional_vjp, sample_hessian_vjp and their autograd forms (functional.SampleDirectionalLatentFn,
SampleHessianLatentFn).  Small shapes: the smallest at which the kernels can go wrong, not workloads.

Op level (211 sources, 1..4 hidden layers, nd in {1, 3, 6}, directions DIFFERENT for every query so that one 32-edge tile holds several
and a token's segment sums edges with different directions): regular lists of 37 queries x k in {1, 8, 32} (a partial last tile, a
query's edges straddling a tile at k = 8, 37 tiles at k = 32) and the ragged list [3, 0, 7, 1, 4, 40, 0] (an empty query, a 40-edge row
across two tiles, tokens without edges: exact zeros) against the fp64 closed form (tests/gno_qdir_jet2_adj_ref.py).  Bit-equality the
design guarantees: with every query given the same directions the call is ops.gno_adjoint_jet2 on those host directions; stride 0 is
three copies of the plane; k and an explicit rowptr_dst agree; two runs and bf16 mode give the same bits.  No edges, no queries, no
sources; bad operands raise before any launch.  The element kernel: hidden in {64, 128, 256} x nd in {1, 3, 6}, 33 and 1000 rows (1000
rows x 64: not a multiple of the block), with and without A, out of place and over either stack, against fp64 plane by plane.

Model level (hb._setup: 4096 points, latent 8^3, k = 8, r = 0.45; 150 + 150 queries partly outside the box): both calls against the
fp64 oracle's decoder differentiated twice in the query and then in the latent on the lists the streamed routes use, for 'knn' /
'radius' / 'bidirectional' / two softmax-weighted scales on 'radius', at chunkings None / 250 / 64, with each optional cotangent None;
the autograd forms; losses on d2 along per-query normals and on an off-diagonal Hessian entry through model.latent into an encoder
weight against the whole-model fp64 oracle; consistency with sample_laplacian_vjp; refusals; the row route in a capture.

Bars: the project's fp32 bar for derivatives (FP32_BAR: max error <= 1e-3 of the reference's peak, cosine >= 0.99999), every peak
asserted > 0.  Distances measured on an MI355X are quoted in DESIGN.md 3.2i."""
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
import gno_qdir_jet2_adj_ref as QA  # noqa: E402
import test_coord_grad_gpu as cg  # noqa: E402  (_batch64)
import test_field_adjoint_gpu as ag  # noqa: E402  (the regular lists, the models, SHAPES, the refusal table)
import test_field_hessian_gpu as hb  # noqa: E402  (the model fixture, the watcher, check(), the bar, the queries)
import test_field_jacobian_adjoint_gpu as jg  # noqa: E402  (_route_edges)
import test_field_jacobian_rows_gpu as jr  # noqa: E402  (the device operands, _graph)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NSRC = jr.NSRC
NDS = (1, 3, 6)
DEG = [3, 0, 7, 1, 4, 40, 0]
NQ = 37


def _cots(nd, nq, gen, shared=False):
    return torch.randn(nd, nq, 32, generator=gen), torch.randn(1 if shared else nd, nq, 32, generator=gen)


def _lists(gen):
    """name -> (src, dst, rowptr, k or None): the regular lists and the ragged one"""
    out = {}
    for k in (1, 8, 32):
        src, dst, rowptr, _, _ = ag._regular(NQ, k, gen)
        out[f"k{k}"] = (src, dst, rowptr, k)
    out["ragged"] = (*REF.random_list(DEG, NSRC, gen), None)
    return out


def _by_source(src, dst, rowptr, k):
    from gaot_3d_amd import graph
    if k is not None:
        return graph.by_source((src.to(DEV), k), NSRC)
    return graph.by_source(jr._graph(src.int(), dst.int(), rowptr.int(), NSRC), NSRC)


# ---- op level: the kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh", [1, 2, 3, 4])
def test_the_kernel_meets_fp64_with_directions_of_every_query(nh):
    from gaot_3d_amd import ops
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(nh, "linear")
    worst = 0.0
    for name, (src, dst, rowptr, k) in _lists(gen).items():
        nq = rowptr.numel() - 1
        assert name != "k8" or (src.numel() > 4 * 32 and 32 % 8 == 0 and NQ * 8 % 32 != 0)      # more than four tiles, a partial one
        x = torch.rand(nq, 3, generator=gen) * 2 - 1
        g = torch.randn(nq, 32, generator=gen)
        gs = _by_source(src, dst, rowptr, k)
        xd, gd = x.to(DEV), g.to(DEV)
        unused = torch.ones(NSRC, dtype=torch.bool)
        unused[src.long()] = False
        for nd in NDS:
            v = torch.randn(nq, nd, 3, generator=gen)                                           # different for every query
            p, s = _cots(nd, nq, gen)
            vd, pd, sd = v.to(DEV), p.to(DEV), s.to(DEV)
            n0 = ops.launch_count()
            got = ops.gno_adjoint_jet2_qd(wd, bd, yd, xd, vd, gd, pd, sd, gs, k)
            assert ops.launch_count() == n0 + 2, (name, nd)                                     # the kernel and its fix-up
            assert got.shape == (NSRC, 32) and got.dtype == torch.float32
            ref = QA.adjoint_jet2_qd_closed(ws, bs, y, x, src, dst, rowptr, v, g, p, s, NSRC)
            rel, _ = hb.check(f"gno_adj_jet2_qd/nh{nh}/{name}/nd{nd}", got, ref, quiet=True)
            worst = max(worst, rel)
            if unused.any():                                                                    # tokens without edges: exact zeros
                assert torch.equal(got[unused.to(DEV)], torch.zeros(int(unused.sum()), 32, device=DEV)), (name, nd)
            # the directions are read per query: one query's directions on all of them are far from this reference
            same = ops.gno_adjoint_jet2_qd(wd, bd, yd, xd, vd[:1].expand_as(vd).contiguous(), gd, pd, sd, gs, k)
            assert nq == 1 or (same.double().cpu() - ref).abs().max() > 1e-2 * ref.abs().max(), (name, nd)
        assert name != "ragged" or unused.any()
    print(f"[adjoint_jet2_qd] nh{nh}: worst kernel / fp64 = {worst:.3e} of the peak")


@pytest.mark.parametrize("nh", [1, 2, 3, 4])
def test_bit_equalities_the_design_guarantees(nh):
    from gaot_3d_amd import ops
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(nh, "linear")
    for name, (src, dst, rowptr, k) in _lists(gen).items():
        nq = rowptr.numel() - 1
        x = torch.rand(nq, 3, generator=gen) * 2 - 1
        g = torch.randn(nq, 32, generator=gen)
        gs = _by_source(src, dst, rowptr, k)
        xd, gd = x.to(DEV), g.to(DEV)
        for nd in NDS:
            dirs = hb.GENERIC[:nd]
            vd = torch.tensor(dirs)[None].expand(nq, nd, 3).contiguous().to(DEV)                # every query: the same directions
            p, s = _cots(nd, nq, gen)
            pd, sd = p.to(DEV), s.to(DEV)
            got = ops.gno_adjoint_jet2_qd(wd, bd, yd, xd, vd, gd, pd, sd, gs, k)
            assert torch.equal(got, ops.gno_adjoint_jet2(wd, bd, yd, xd, dirs, gd, pd, sd, gs, k)), (name, nd)   # the host-direction kernel
            assert torch.equal(got, ops.gno_adjoint_jet2_qd(wd, bd, yd, xd, vd, gd, pd, sd, gs, k)), (name, nd)  # two runs
            with hb._precision("bf16"):
                assert torch.equal(got, ops.gno_adjoint_jet2_qd(wd, bd, yd, xd, vd, gd, pd, sd, gs, k)), (name, nd)
        # per-query directions: stride 0 reads ONE plane where stride Nq * 32 reads three equal ones; k and rowptr_dst agree
        vd = torch.randn(nq, 3, 3, generator=gen).to(DEV)
        p, s = _cots(3, nq, gen, shared=True)
        pd, sd = p.to(DEV), s.to(DEV)
        one = ops.gno_adjoint_jet2_qd(wd, bd, yd, xd, vd, gd, pd, sd, gs, k)
        assert torch.equal(one, ops.gno_adjoint_jet2_qd(wd, bd, yd, xd, vd, gd, pd, sd.expand(3, -1, -1).contiguous(), gs, k)), name
        if k is not None:
            both = ag._both_lists(src, dst, nq)
            assert torch.equal(one, ops.gno_adjoint_jet2_qd(wd, bd, yd, xd, vd, gd, pd, sd, both)), name
            assert torch.equal(one, ops.gno_adjoint_jet2_qd(wd, bd, yd, xd, vd, gd, pd, sd, _by_source(src, dst, rowptr, None))), name


def _raw(m, yd, xd, vd, nd, gd, pd, sd, stride, rowptr_dst, k, gr, nsrc, nq, out, wsp):
    from gaot_3d_amd import _lib, ops
    return _lib.load().gaot_gno_adj_jet2_qd(C.byref(m), ops._ptr(yd), ops._ptr(xd), vd, nd, ops._ptr(gd), ops._ptr(pd), ops._ptr(sd),
                                            stride, ops._ptr(rowptr_dst), k, ops._ptr(gr.by_src.key), ops._ptr(gr.by_src.other),
                                            ops._ptr(gr.by_src.rowptr), gr.by_src.num_edges, nsrc, nq, ops._ptr(out), ops._ptr(wsp),
                                            wsp.numel(), ops._stream())


def test_no_edges_no_queries_no_sources():
    from gaot_3d_amd import _lib, graph, ops
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(2, "linear")
    empty = lambda: torch.empty(0, dtype=torch.int32, device=DEV)
    zeros = torch.zeros(NSRC, 32, device=DEV)
    for nq in (5, 0):
        rows = ops.BipartiteGraph(ops.SortedEdges(torch.zeros(nq + 1, dtype=torch.int32, device=DEV), None, empty(), empty(), nq),
                                  None, NSRC, nq)
        gr = graph.by_source(rows, NSRC)
        xd, gd, vd = torch.zeros(nq, 3, device=DEV), torch.ones(nq, 32, device=DEV), torch.ones(nq, 3, 3, device=DEV)
        pd, sd = torch.ones(3, nq, 32, device=DEV), torch.ones(1, nq, 32, device=DEV)
        n0 = ops.launch_count()
        got = ops.gno_adjoint_jet2_qd(wd, bd, yd, xd, vd, gd, pd, sd, gr)
        assert ops.launch_count() == n0 + 1                                                # the fix-up alone writes the zeros
        assert torch.equal(got, zeros)
    gr = graph.by_source((empty(), 8), NSRC)                                               # zero queries of a regular list
    assert torch.equal(ops.gno_adjoint_jet2_qd(wd, bd, yd, torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, 3, device=DEV),
                                               torch.zeros(0, 32, device=DEV), torch.zeros(3, 0, 32, device=DEV),
                                               torch.zeros(3, 0, 32, device=DEV), gr, 8), zeros)
    # no sources: nothing to write, nothing launched
    m, keep = ops._mlp_struct(wd, bd)
    gr0 = types.SimpleNamespace(by_src=types.SimpleNamespace(key=empty(), other=empty(), rowptr=torch.zeros(1, dtype=torch.int32, device=DEV),
                                                             num_edges=0))
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    rc = _raw(m, None, None, None, 3, None, None, None, 0, torch.zeros(1, dtype=torch.int32, device=DEV), 0, gr0, 0, 0, None,
              ops._ws(_lib.load().gaot_gno_adj_jet2_qd_workspace_bytes(0), DEV))
    assert rc == 0, _lib.load().gaot_last_error()
    assert ops.launch_count() == n0


def test_bad_operands_raise_before_any_launch():
    from gaot_3d_amd import _lib, graph, ops
    from gaot_3d_amd._lib import GaotError
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(2, "linear")
    src, dst, rowptr, x, g = ag._regular(33, 8, gen)
    p, s = _cots(3, 33, gen)
    v = torch.randn(33, 3, 3, generator=gen)
    xd, gd, pd, sd, vd = x.to(DEV), g.to(DEV), p.to(DEV), s.to(DEV), v.to(DEV)
    gr = graph.by_source((src.to(DEV), 8), NSRC)
    rows = jr._graph(src, dst, rowptr, NSRC)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    run = ops.gno_adjoint_jet2_qd
    bad = [
        lambda: run(wd, bd, yd, xd, v, gd, pd, sd, gr, 8),                                  # directions on the host
        lambda: run(wd, bd, yd, xd, hb.GENERIC[:3], gd, pd, sd, gr, 8),                     # host values: the other entry point's
        lambda: run(wd, bd, yd, xd, vd.double(), gd, pd, sd, gr, 8),
        lambda: run(wd, bd, yd, xd, vd[:20].contiguous(), gd, pd, sd, gr, 8),               # not one row per query
        lambda: run(wd, bd, yd, xd, vd[:, :, :2].contiguous(), gd, pd, sd, gr, 8),          # directions of two components
        lambda: run(wd, bd, yd, xd, vd[:, 0], gd, pd, sd, gr, 8),                           # [Nq, 3]
        lambda: run(wd, bd, yd, xd, vd[:, :0].contiguous(), gd, pd[:0].contiguous(), sd[:0].contiguous(), gr, 8),   # no direction
        lambda: run(wd, bd, yd, xd, torch.zeros(33, 7, 3, device=DEV), gd, torch.zeros(7, 33, 32, device=DEV), sd[:1].contiguous(), gr, 8),
        lambda: run(wd, bd, yd, xd, vd, gd, pd[:2].contiguous(), sd, gr, 8),                # two planes for three directions
        lambda: run(wd, bd, yd, xd, vd, gd, pd[:, :, :16].contiguous(), sd, gr, 8),
        lambda: run(wd, bd, yd, xd, vd, gd, pd.double(), sd, gr, 8),
        lambda: run(wd, bd, yd, xd, vd, gd, pd.cpu(), sd, gr, 8),
        lambda: run(wd, bd, yd, xd, vd, gd, None, sd, gr, 8),
        lambda: run(wd, bd, yd, xd, vd, gd, pd, sd[:2].contiguous(), gr, 8),                # grad_d2: neither nd nor one plane
        lambda: run(wd, bd, yd, xd, vd, gd, pd, sd[0], gr, 8),
        lambda: run(wd, bd, yd, xd, vd, gd, pd, None, gr, 8),
        lambda: run(wd, bd, yd, xd, vd, gd[:, :16].contiguous(), pd, sd, gr, 8),            # gno_adjoint's rules
        lambda: run(wd, bd, yd, xd, vd, gd.cpu(), pd, sd, gr, 8),
        lambda: run(wd, bd, yd[:100].contiguous(), xd, vd, gd, pd, sd, gr, 8),
        lambda: run(wd, bd, yd, xd, vd, gd, pd, sd, gr),                                    # neither rowptr_dst nor k
        lambda: run(wd, bd, yd, xd, vd, gd, pd, sd, gr, 4),                                 # k that does not match the list
        lambda: run(wd, bd, yd, xd, vd, gd, pd, sd, rows),                                  # no by-source list
        lambda: run(wd[:1], bd[:1], yd, xd, vd, gd, pd, sd, gr, 8),                         # one linear layer
    ]
    for i, call in enumerate(bad):
        with pytest.raises(GaotError):
            call()
        assert ops.launch_count() == n0, i
    # the C ABI's own checks, before any launch
    lib = _lib.load()
    m, keep = ops._mlp_struct(wd, bd)
    out = torch.zeros(NSRC, 32, device=DEV)
    wsp = ops._ws(lib.gaot_gno_adj_jet2_qd_workspace_bytes(gr.by_src.num_edges), DEV)
    assert wsp.numel() == lib.gaot_gno_adj_jet2_workspace_bytes(gr.by_src.num_edges)
    host = (C.c_float * (33 * 9))(*v.reshape(-1).tolist())
    plane = 33 * 32

    def raw(dirs=ops._ptr(vd), nd=3, g1=pd, g2=sd, stride=plane):
        return _raw(m, yd, xd, dirs, nd, gd, g1, g2, stride, None, 8, gr, NSRC, 33, out, wsp)
    for kw, word in ((dict(g1=None), "grad_d1"), (dict(g2=None), "grad_d2"), (dict(stride=32), "grad_d2_stride"),
                     (dict(stride=2 * plane), "grad_d2_stride"), (dict(nd=0), "nd must be"), (dict(nd=7), "nd must be"),
                     (dict(dirs=None), "null dirs"), (dict(dirs=host), "device pointer")):
        assert raw(**kw) != 0 and word in lib.gaot_last_error().decode(), (kw, lib.gaot_last_error())
        assert ops.launch_count() == n0, kw
    assert raw(stride=0) == 0 and raw() == 0


# ---- op level: the element kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", NDS)
@pytest.mark.parametrize("hidden", [64, 128, 256])
def test_the_element_kernel_meets_fp64_plane_by_plane(hidden, nd):
    from gaot_3d_amd import ops
    from gaot_3d_amd._lib import GaotError
    gen = torch.Generator().manual_seed(hidden + nd)
    npl = 1 + 2 * nd
    worst = 0.0
    for rows in (33, 1000):                                    # 33 x 64 / 4 = 528 vectors: two blocks and a part of a third
        zus = torch.randn(npl, rows, hidden, generator=gen)
        zus[0] *= 2.0                                          # pre-activations over the range where phi matters and beyond it
        acot = torch.randn(npl, rows, hidden, generator=gen)
        b1 = 0.3 * torch.randn(hidden, generator=gen)
        zd, ad, bd = zus.to(DEV), acot.to(DEV), b1.to(DEV)
        for with_a in (True, False):
            ref = QA.jet2_cot_mid(zus[0].double() + b1.double(), zus[1:1 + nd], zus[1 + nd:], acot[0] if with_a else None,
                                  acot[1:1 + nd], acot[1 + nd:])
            n0 = ops.launch_count()
            got = ops.mlp2_jet2_cot_mid(zd, ad[0] if with_a else None, ad[1:], bd)
            assert ops.launch_count() == n0 + 1                # one launch for every nd
            assert got.shape == (npl, rows, hidden) and got.dtype == torch.float32 and got.data_ptr() not in (zd.data_ptr(), ad.data_ptr())
            for pl in range(npl):
                rel, _ = hb.check(f"mlp2_jet2_cot_mid/h{hidden}/nd{nd}/rows{rows}/{'A' if with_a else 'noA'}/plane{pl}", got[pl], ref[pl],
                                  quiet=True)
                worst = max(worst, rel)
            # over the z stack, and (with A) over the cotangent stack: the same bits
            zc = zd.clone()
            assert torch.equal(ops.mlp2_jet2_cot_mid(zc, ad[0] if with_a else None, ad[1:], bd, out=zc), got)
            if with_a:
                ac = ad.clone()
                assert torch.equal(ops.mlp2_jet2_cot_mid(zd, ac[0], ac[1:], bd, out=ac), got)
        no_bias = ops.mlp2_jet2_cot_mid(zd, ad[0], ad[1:])
        hb.check(f"mlp2_jet2_cot_mid/h{hidden}/nd{nd}/rows{rows}/no_bias", no_bias,
                 QA.jet2_cot_mid(zus[0], zus[1:1 + nd], zus[1 + nd:], acot[0], acot[1:1 + nd], acot[1 + nd:]), quiet=True)
    print(f"[jet2_cot_mid] hidden {hidden}, nd {nd}: worst plane / fp64 = {worst:.3e} of the plane's peak")
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    for call in (lambda: ops.mlp2_jet2_cot_mid(zd[:npl - 1], ad[0], ad[1:]), lambda: ops.mlp2_jet2_cot_mid(zd, ad[0], ad[2:]),
                 lambda: ops.mlp2_jet2_cot_mid(zd, ad[0, :5], ad[1:]), lambda: ops.mlp2_jet2_cot_mid(zd.double(), ad[0], ad[1:]),
                 lambda: ops.mlp2_jet2_cot_mid(zd, ad[0].cpu(), ad[1:]), lambda: ops.mlp2_jet2_cot_mid(zd, ad[0], ad[1:], bd[:8]),
                 lambda: ops.mlp2_jet2_cot_mid(zd.transpose(1, 2), ad[0], ad[1:]),
                 lambda: ops.mlp2_jet2_cot_mid(torch.zeros(15, 4, hidden, device=DEV), None, torch.zeros(14, 4, hidden, device=DEV)),
                 lambda: ops.mlp2_jet2_cot_mid(zd[:, :, :6].contiguous(), ad[0, :, :6].contiguous(), ad[1:, :, :6].contiguous())):
        with pytest.raises(GaotError):
            call()
    assert ops.launch_count() == n0


# ---- model level ------------------------------------------------------------------------------------------------------------------------
CHUNKS = ag.CHUNKS
CASES = {
    "knn": ("knn", dict()),
    "radius": ("radius", dict()),
    "bidirectional": ("bidirectional", dict()),
    "two_scales_weighted_radius": ag.SHAPES["two_scales_weighted_radius"],
}
ND = 3


def _case(case):
    strategy, kw = CASES[case]
    kw = dict(kw)
    out = kw.pop("out", 1)
    key, (model, batch, tokens, cfg) = ag._model(strategy, out=out, **kw)
    q = hb._queries(batch, 150, 150)
    return key + "/dir150", strategy, model, batch, tokens, cfg, q, ag._latent(model, batch, tokens), out


def _frame(nq, seed=59):
    """an orthonormal frame (n, t1, t2) per query [nq, 3, 3], by Gram-Schmidt in fp64"""
    gen = torch.Generator().manual_seed(seed)
    a, b = (torch.randn(nq, 3, generator=gen, dtype=torch.float64) for _ in range(2))
    n = torch.nn.functional.normalize(a, dim=1)
    t1 = torch.nn.functional.normalize(b - (b * n).sum(1, keepdim=True) * n, dim=1)
    return torch.stack([n, t1, torch.linalg.cross(n, t1)], dim=1).float()


def _jac_hess(p, xg):
    """(jac [Nq, out, 3], hess [Nq, out, 3, 3]) of p [Nq, out] whose row q depends on xg[q] alone, both still differentiable"""
    oc = p.shape[1]
    jac = torch.stack([torch.autograd.grad(p[:, o].sum(), xg, create_graph=True)[0] for o in range(oc)], dim=1)
    hess = torch.stack([torch.stack([torch.autograd.grad(jac[:, o, i].sum(), xg, create_graph=True)[0] for i in range(3)], dim=1)
                        for o in range(oc)], dim=1)
    return jac, hess


_REFS = {}


def _oracle(key, model, cfg, lat, q):
    """-> (pred, jac, hess, the latent leaf): the fp64 oracle's decoder on the CPU on the lists the streamed routes use, differentiated
    twice in the query with its graph kept, so that a test takes the gradient of its own loss with respect to the latent; once per key"""
    if key not in _REFS:
        edges, tok = jg._route_edges(model, cfg, lat, q)
        sd = {n: v.detach().double().cpu() for n, v in model.state_dict().items()}
        lat64 = lat.detach().double().cpu().requires_grad_(True)
        xg = q.detach().double().cpu().requires_grad_(True)
        p = orc.magno_decoder(sd, cfg.magno, lat64, xg, tok.double().cpu(), types.SimpleNamespace(**edges))
        _REFS[key] = (p, *_jac_hess(p, xg), lat64)
    return _REFS[key]


def _grad(loss, lat64):
    return torch.autograd.grad(loss, lat64, retain_graph=True)[0]


def _dir_jets(jac, hess, v):
    v = v.double().cpu()
    return torch.einsum("qod,qnd->qon", jac, v), torch.einsum("qoij,qni,qnj->qon", hess, v, v)


def _keys_ok(seen, rows, qd, nd):
    keys = seen["keys"]
    fwd = ("gno_jet2_rows" if rows else "gno_jet2_knn") + ("_qd_nh" if qd else "_nh")
    adj, other = ("gno_adj_jet2_qd_nh", "gno_adj_jet2_nh") if qd else ("gno_adj_jet2_nh", "gno_adj_jet2_qd_nh")
    return (any(k.startswith(adj) for k in keys) and any(k.startswith(fwd) and k.endswith(f"_d{nd}") for k in keys)
            and any(k.startswith("mlp2_jet2_cot_mid_h") and k.endswith(f"_d{nd}") for k in keys)
            and not any(k.startswith(s) for k in keys for s in ("gno_bwd", "gno_adj_nh", "gno_adj_jac_nh", "mlp2_lap_cot_mid", other)))


@pytest.mark.parametrize("case", list(CASES))
def test_sample_directional_vjp_meets_the_oracle_at_every_chunking(case, monkeypatch):
    key, strategy, model, batch, tokens, cfg, q, lat, out = _case(case)
    nq = q.shape[0]
    gen = torch.Generator().manual_seed(61)
    v = torch.randn(nq, ND, 3, generator=gen).to(DEV)                                       # every query's own directions, not unit
    gy, g1, g2 = (torch.randn(nq, out, *t, generator=gen).to(DEV) for t in ((), (ND,), (ND,)))
    p, jac, hess, lat64 = _oracle(key, model, cfg, lat, q)
    d1, d2 = _dir_jets(jac, hess, v)
    r_pred, r_d1, r_d2 = (_grad((t * c.double().cpu()).sum(), lat64) for t, c in ((p, gy), (d1, g1), (d2, g2)))
    ref = r_pred + r_d1 + r_d2
    assert r_d2.abs().max() > 1e-3 * ref.abs().max()                                        # the second-order part is there to be seen
    got = {}
    for chunk in CHUNKS:
        with hb._watch(monkeypatch) as seen:
            got[chunk] = model.sample_directional_vjp(lat, q, v, gy, g1, g2, chunk_points=chunk)
        assert _keys_ok(seen, strategy != "knn", True, ND), seen
        assert got[chunk].shape == lat.shape and got[chunk].dtype == torch.float32 and not got[chunk].requires_grad
        hb.check(f"sample_directional_vjp/{case}/chunk{chunk}", got[chunk], ref)
    assert torch.equal(got[64], model.sample_directional_vjp(lat, q, v, gy, g1, g2, chunk_points=64))                 # reproducible
    peak = ref.abs().max().item()
    for chunk in CHUNKS[1:]:
        d = (got[chunk] - got[None]).abs().max().item()
        print(f"[chunking] sample_directional_vjp/{case}: chunk {chunk} against one piece: max |d| = {d:.3e} = {d / peak:.3e} of the peak")
        assert d <= 1e-5 * peak, (chunk, d, peak)           # close, not equal: a token's sum is split at the chunk boundaries
    with hb._precision("bf16"):
        assert torch.equal(model.sample_directional_vjp(lat, q, v, gy, g1, g2, chunk_points=250), got[250])           # the same bits
    # each optional cotangent None
    for name, cots, r in (("d2_only", (None, None, g2), r_d2), ("cot_pred_none", (None, g1, g2), r_d1 + r_d2),
                          ("cot_d1_none", (gy, None, g2), r_pred + r_d2), ("cot_d2_none", (gy, g1, None), r_pred + r_d1)):
        hb.check(f"sample_directional_vjp/{case}/{name}", model.sample_directional_vjp(lat, q, v, *cots, chunk_points=250), r)
    # one direction per query given as [Nq, 3]
    one = model.sample_directional_vjp(lat, q, v[:, 0].contiguous(), None, None, g2[:, :, :1].contiguous(), chunk_points=250)
    hb.check(f"sample_directional_vjp/{case}/one_direction", one, _grad((d2[:, :, :1] * g2[:, :, :1].double().cpu()).sum(), lat64))


@pytest.mark.parametrize("case", list(CASES))
def test_sample_hessian_vjp_meets_the_oracle_at_every_chunking(case, monkeypatch):
    key, strategy, model, batch, tokens, cfg, q, lat, out = _case(case)
    nq = q.shape[0]
    gen = torch.Generator().manual_seed(67)
    gy, gj, gh = (torch.randn(nq, out, *t, generator=gen).to(DEV) for t in ((), (3,), (3, 3)))       # cot_hess NOT symmetric
    p, jac, hess, lat64 = _oracle(key, model, cfg, lat, q)
    r_pred, r_jac, r_hess = (_grad((t * c.double().cpu()).sum(), lat64) for t, c in ((p, gy), (jac, gj), (hess, gh)))
    ref = r_pred + r_jac + r_hess
    assert r_hess.abs().max() > 1e-3 * ref.abs().max()
    got = {}
    for chunk in CHUNKS:
        with hb._watch(monkeypatch) as seen:
            got[chunk] = model.sample_hessian_vjp(lat, q, gy, gj, gh, chunk_points=chunk)
        assert _keys_ok(seen, strategy != "knn", False, 6), seen
        assert got[chunk].shape == lat.shape and got[chunk].dtype == torch.float32 and not got[chunk].requires_grad
        hb.check(f"sample_hessian_vjp/{case}/chunk{chunk}", got[chunk], ref)
    assert torch.equal(got[64], model.sample_hessian_vjp(lat, q, gy, gj, gh, chunk_points=64))
    peak = ref.abs().max().item()
    for chunk in CHUNKS[1:]:
        d = (got[chunk] - got[None]).abs().max().item()
        print(f"[chunking] sample_hessian_vjp/{case}: chunk {chunk} against one piece: max |d| = {d:.3e} = {d / peak:.3e} of the peak")
        assert d <= 1e-5 * peak, (chunk, d, peak)
    for name, cots, r in (("hess_only", (None, None, gh), r_hess), ("cot_pred_none", (None, gj, gh), r_jac + r_hess),
                          ("cot_jac_none", (gy, None, gh), r_pred + r_hess), ("cot_hess_none", (gy, gj, None), r_pred + r_jac)):
        hb.check(f"sample_hessian_vjp/{case}/{name}", model.sample_hessian_vjp(lat, q, *cots, chunk_points=250), r)
    # an off-diagonal entry alone
    off = torch.zeros_like(gh)
    off[:, :, 0, 1] = gh[:, :, 0, 1]
    hb.check(f"sample_hessian_vjp/{case}/off_diagonal", model.sample_hessian_vjp(lat, q, None, None, off, chunk_points=250),
             _grad((hess[:, :, 0, 1] * gh[:, :, 0, 1].double().cpu()).sum(), lat64))


@pytest.mark.parametrize("case", ["knn", "bidirectional", "two_scales_weighted_radius"])
def test_the_autograd_forms_are_the_forward_calls_and_their_vjp_backward(case):
    key, strategy, model, batch, tokens, cfg, q, lat, out = _case(case)
    nq = q.shape[0]
    gen = torch.Generator().manual_seed(71)
    v = torch.randn(nq, ND, 3, generator=gen).to(DEV)
    gy, g1, g2, gj, gh = (torch.randn(nq, out, *t, generator=gen).to(DEV) for t in ((), (ND,), (ND,), (3,), (3, 3)))
    with torch.no_grad():                                                                     # fp32 mode
        p0, a0, b0 = model.sample_directional(lat, q, v, chunk_points=250)
        _, j0, h0 = model.sample_hessian_rows(lat, q, chunk_points=250)                       # on 'knn' the call IS sample_hessian
    for mode in ("fp32", "bf16"):
        with hb._precision(mode):
            leaf = lat.clone().requires_grad_(True)
            pred, d1, d2 = model.sample_directional_autograd(leaf, q, v, chunk_points=250)
            assert pred.requires_grad and d1.requires_grad and d2.requires_grad
            assert torch.equal(pred.detach(), p0) and torch.equal(d1.detach(), a0) and torch.equal(d2.detach(), b0), mode
            (grad,) = torch.autograd.grad((pred * gy).sum() + (d1 * g1).sum() + (d2 * g2).sum(), leaf, retain_graph=True)
            assert torch.equal(grad, model.sample_directional_vjp(lat, q, v, gy, g1, g2, chunk_points=250)), mode
            (grad,) = torch.autograd.grad((d2 * g2).sum(), leaf)                              # pred and d1 got no gradient: None
            assert torch.equal(grad, model.sample_directional_vjp(lat, q, v, None, None, g2, chunk_points=250)), mode
            leaf = lat.clone().requires_grad_(True)
            pred, jac, hess = model.sample_hessian_autograd(leaf, q, chunk_points=250)
            assert torch.equal(pred.detach(), p0) and torch.equal(jac.detach(), j0) and torch.equal(hess.detach(), h0), mode
            (grad,) = torch.autograd.grad((pred * gy).sum() + (jac * gj).sum() + (hess * gh).sum(), leaf, retain_graph=True)
            assert torch.equal(grad, model.sample_hessian_vjp(lat, q, gy, gj, gh, chunk_points=250)), mode
            (grad,) = torch.autograd.grad((hess * gh).sum(), leaf)
            assert torch.equal(grad, model.sample_hessian_vjp(lat, q, None, None, gh, chunk_points=250)), mode
    with pytest.raises(ValueError, match="query_pos requires grad"):
        model.sample_directional_autograd(lat.clone().requires_grad_(True), q.clone().requires_grad_(True), v)
    with pytest.raises(ValueError, match="dirs requires grad"):
        model.sample_directional_autograd(lat.clone().requires_grad_(True), q, v.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="query_pos requires grad"):
        model.sample_hessian_autograd(lat.clone().requires_grad_(True), q.clone().requires_grad_(True))


@pytest.mark.parametrize("strategy", ["knn", "bidirectional"])
def test_second_order_losses_reach_an_encoder_parameter(strategy):
    """((d2[..., 0] - target)^2).mean() with per-query normals through sample_directional_autograd, and a loss on an off-diagonal
    Hessian entry through sample_hessian_autograd, each with the autograd of model.latent, against the fp64 oracle of the whole
    model on the route's decoder lists differentiated twice in the query and then in the parameter"""
    key, (model, batch, tokens, cfg) = ag._model(strategy)
    q = hb._queries(batch, 150, 150)
    gen = torch.Generator().manual_seed(73)
    n = torch.nn.functional.normalize(torch.randn(q.shape[0], 3, generator=gen), dim=1).to(DEV)
    target = torch.randn(q.shape[0], 1, generator=gen).to(DEV)
    name = "encoder.gno.channel_mlp.fcs.0.weight"
    param = dict(model.named_parameters())[name]
    _, _, d2 = model.sample_directional_autograd(model.latent(batch, tokens), q, n, chunk_points=250)
    (got_dir,) = torch.autograd.grad(((d2[..., 0] - target) ** 2).mean(), param)
    _, _, hess = model.sample_hessian_autograd(model.latent(batch, tokens), q, chunk_points=250)
    (got_off,) = torch.autograd.grad(((hess[:, :, 0, 1] - target) ** 2).mean(), param)
    edges, tok = jg._route_edges(model, cfg, ag._latent(model, batch, tokens), q)
    sd = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    sd[name].requires_grad_(True)
    b64 = cg._batch64(batch.to("cpu"))
    for k, v in edges.items():
        setattr(b64, k, v)
    xg = q.detach().double().cpu().requires_grad_(True)
    p = orc.gaot3d_forward(sd, cfg, b64, tok.double().cpu(), query_coord_pos=xg)
    jac64, hess64 = _jac_hess(p, xg)
    n64, t64 = n.double().cpu(), target.double().cpu()
    dnn = torch.einsum("qoij,qi,qj->qo", hess64, n64, n64)
    (ref_dir,) = torch.autograd.grad(((dnn - t64) ** 2).mean(), sd[name], retain_graph=True)
    (ref_off,) = torch.autograd.grad(((hess64[:, :, 0, 1] - t64) ** 2).mean(), sd[name])
    hb.check(f"sample_directional_autograd/{strategy}/normal_curvature_loss/encoder_parameter", got_dir, ref_dir)
    hb.check(f"sample_hessian_autograd/{strategy}/off_diagonal_loss/encoder_parameter", got_off, ref_off)


@pytest.mark.parametrize("case", list(CASES))
def test_a_frame_and_the_identity_give_the_laplacian_adjoint(case):
    """sum_i D^2_{v_i} over an orthonormal frame is the Laplacian, and so is the trace of the Hessian: the three calls are three fp32
    routes to one number.  The margin is fp32 rounding, measured here as the distance between sample_laplacian_vjp at two chunkings
    on the same inputs; 10 x that is allowed, because the summation order differs in the middle and in the kernel."""
    key, strategy, model, batch, tokens, cfg, q, lat, out = _case(case)
    nq = q.shape[0]
    gl = torch.randn(nq, out, generator=torch.Generator().manual_seed(79)).to(DEV)
    frame = _frame(nq).to(DEV)
    lap = model.sample_laplacian_vjp(lat, q, None, None, gl, chunk_points=None)
    margin = (lap - model.sample_laplacian_vjp(lat, q, None, None, gl, chunk_points=64)).abs().max().item()
    peak = lap.abs().max().item()
    assert peak > 0 and margin > 0
    by_dir = model.sample_directional_vjp(lat, q, frame, None, None, gl[:, :, None].expand(nq, out, 3).contiguous())
    eye = torch.eye(3, device=DEV)
    by_hess = model.sample_hessian_vjp(lat, q, None, None, (gl[:, :, None, None] * eye).contiguous())
    dd, dh = (by_dir - lap).abs().max().item(), (by_hess - lap).abs().max().item()
    print(f"[laplacian] {case}: |lap_vjp(None) - lap_vjp(64)| = {margin:.3e} = {margin / peak:.3e} of the peak; frame: {dd:.3e} "
          f"({dd / margin:.2f} x); Hessian: {dh:.3e} ({dh / margin:.2f} x)")
    assert dd <= 10.0 * margin, (dd, margin, peak)
    assert dh <= 10.0 * margin, (dh, margin, peak)


@pytest.mark.parametrize("case", list(ag.REFUSALS))
def test_other_configurations_are_refused_before_any_launch(case):
    from gaot_3d_amd import ops
    strategy, k, kw, msg = ag.REFUSALS[case]
    model, batch, tokens, cfg = hb._setup(f"adjoint/refuse/{case}", k=k, **ag.MODELS[strategy], **kw)
    lat = ag._latent(model, batch, tokens)
    q = batch.pos[:200].contiguous()
    v = torch.ones(200, 2, 3, device=DEV)
    gy, gd, gj, gh = (torch.ones(200, 1, *t, device=DEV) for t in ((), (2,), (3,), (3, 3)))
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    what = "adjoint of the field's directional derivatives.*"
    with pytest.raises(NotImplementedError, match=what + msg):
        model.sample_directional_vjp(lat, q, v, gy, gd, gd)
    with pytest.raises(NotImplementedError, match=what + msg):
        model.sample_directional_autograd(lat.clone().requires_grad_(True), q, v)
    what = "adjoint of the field's Hessian.*"
    with pytest.raises(NotImplementedError, match=what + msg):
        model.sample_hessian_vjp(lat, q, gy, gj, gh)
    with pytest.raises(NotImplementedError, match=what + msg):
        model.sample_hessian_autograd(lat.clone().requires_grad_(True), q)
    assert ops.launch_count() == n0


def test_argument_rules_raise_on_the_device():
    from gaot_3d_amd import ops
    key, (model, batch, tokens, cfg) = ag._model("knn")
    lat = ag._latent(model, batch, tokens)
    q = batch.pos[:100].contiguous()
    v = torch.ones(100, 2, 3, device=DEV)
    gy, gd, gj, gh = (torch.ones(100, 1, *t, device=DEV) for t in ((), (2,), (3,), (3, 3)))
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    for bad in (v.double(), v.cpu(), v[:50], torch.zeros(100, 7, 3, device=DEV), torch.zeros(100, 2, 2, device=DEV)):
        with pytest.raises(ValueError, match="dirs|directions per query"):
            model.sample_directional_vjp(lat, q, bad, gy, gd, gd)
        with pytest.raises(ValueError, match="dirs|directions per query"):
            model.sample_directional_autograd(lat, q, bad)
    for bad in (gy.double(), gy.cpu(), gy[:50], torch.zeros(100, 2, device=DEV)):
        with pytest.raises(ValueError, match="cot_pred"):
            model.sample_directional_vjp(lat, q, v, bad, gd, gd)
        with pytest.raises(ValueError, match="cot_pred"):
            model.sample_hessian_vjp(lat, q, bad, gj, gh)
    for bad in (gd.double(), gd.cpu(), gd[:50], torch.zeros(100, 1, 3, device=DEV), torch.zeros(100, 2, device=DEV)):
        with pytest.raises(ValueError, match="cot_d1"):
            model.sample_directional_vjp(lat, q, v, gy, bad, gd)
        with pytest.raises(ValueError, match="cot_d2"):
            model.sample_directional_vjp(lat, q, v, gy, gd, bad)
    for bad in (gj.double(), gj.cpu(), gj[:50], torch.zeros(100, 1, 2, device=DEV)):
        with pytest.raises(ValueError, match="cot_jac"):
            model.sample_hessian_vjp(lat, q, gy, bad, gh)
    for bad in (gh.double(), gh.cpu(), gh[:50], torch.zeros(100, 1, 3, device=DEV), torch.zeros(100, 1, 6, device=DEV)):
        with pytest.raises(ValueError, match="cot_hess"):
            model.sample_hessian_vjp(lat, q, gy, gj, bad)
    with pytest.raises(ValueError, match="all None"):
        model.sample_directional_vjp(lat, q, v, None, None, None)
    with pytest.raises(ValueError, match="all None"):
        model.sample_hessian_vjp(lat, q, None, None, None)
    with pytest.raises(ValueError, match="chunk_points"):
        model.sample_directional_vjp(lat, q, v, gy, gd, gd, chunk_points=0)
    with pytest.raises(ValueError, match="chunk_points"):
        model.sample_hessian_vjp(lat, q, gy, gj, gh, chunk_points=0)
    model.decoder._shard_group = object()
    try:
        with pytest.raises(NotImplementedError, match="point-sharded"):
            model.sample_directional_vjp(lat, q, v, gy, gd, gd)
        with pytest.raises(NotImplementedError, match="point-sharded"):
            model.sample_hessian_vjp(lat, q, gy, gj, gh)
    finally:
        del model.decoder._shard_group
    model.decoder.projection.non_linearity = "relu"
    try:
        with pytest.raises(NotImplementedError, match="adjoint of the field's directional derivatives.*erf-GELU"):
            model.sample_directional_vjp(lat, q, v, gy, gd, gd)
        with pytest.raises(NotImplementedError, match="adjoint of the field's Hessian.*erf-GELU"):
            model.sample_hessian_autograd(lat.clone().requires_grad_(True), q)
    finally:
        model.decoder.projection.non_linearity = "gelu"
    assert ops.launch_count() == n0
    tok = model._tokens(1, q.device, None, None)[0]
    with pytest.raises(NotImplementedError, match="do not stream"):                         # tokens off the regular grid
        model.sample_directional_vjp(lat, q, v, gy, gd, gd, tokens_pos=(tok + 0.01 * torch.rand_like(tok)))


def test_in_a_capture_the_row_route_raises_before_any_launch():
    from gaot_3d_amd import ops
    from gaot_3d_amd._lib import GaotError
    key, (model, batch, tokens, cfg) = ag._model("bidirectional")
    q = batch.pos[:300].contiguous()
    lat = ag._latent(model, batch, tokens)
    v = torch.ones(300, 1, 3, device=DEV)
    gd, gh = torch.ones(300, 1, 1, device=DEV), torch.ones(300, 1, 3, 3, device=DEV)
    eager_d = model.sample_directional_vjp(lat, q, v, None, None, gd)      # describes the grid, warms the allocator
    eager_h = model.sample_hessian_vjp(lat, q, None, None, gh)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    for call in (lambda: model.sample_directional_vjp(lat, q, v, None, None, gd), lambda: model.sample_hessian_vjp(lat, q, None, None, gh)):
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(GaotError, match="captured"):
            with torch.cuda.graph(graph):
                call()
        assert ops.launch_count() == n0
        torch.cuda.synchronize()
    assert torch.equal(model.sample_directional_vjp(lat, q, v, None, None, gd), eager_d)
    assert torch.equal(model.sample_hessian_vjp(lat, q, None, None, gh), eager_h)
