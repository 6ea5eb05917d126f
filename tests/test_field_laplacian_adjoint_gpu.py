"""GPU: the adjoint of the field's Laplacian -- gaot_gno_adj_jet2 (ops.gno_adjoint_jet2), gaot_mlp2_lap_cot_mid (ops.mlp2_lap_cot_mid),
IntegralTransform.adjoint_jet2_knn / adjoint_jet2_rows, MAGNODecoder / GAOT3D.sample_laplacian_vjp and GAOT3D.sample_laplacian_autograd
(functional.SampleLaplacianLatentFn).

Op level (211 sources, 1..4 hidden layers): regular lists Nq in {1, 7, 33, 1000} x k in {1, 4, 8, 32} x nd in {1, 3, 6} (generic and
axis directions mixed) x both strides of grad_d2 against the fp64 closed form (tests/gno_jet2_adj_ref.py); with grad_d1 = grad_d2 = 0
no further from fp64 than max(4 x ops.gno_adjoint on the same operands, 1e-6 of the peak); along the axes with grad_d2 = 0 the same
against ops.gno_adjoint_jac; the duality <G, out> + sum <P_i, d1_i> + sum <S_i, d2_i> = <grad_f, f> with the jets from
ops.gno_forward_knn_jet2 on the same list, both sides summed in fp64, within 1e-3 of sum |terms|; two launches per call.  Rows built
by hand (200 queries on one token; rows ending / starting on tile boundaries with E = 69) through the raw ABI over a NaN pre-fill:
unused tokens exact zeros; E = 0 is the fix-up alone; zero queries.  The ragged lists a-e of the row-list tests take the degree from
rowptr_dst; on a regular list the k form and the rowptr_dst form agree bit for bit; two calls and bf16 mode give the same bits; bad
operands raise GaotError before any launch.  The element kernel: rows in {1, 33, 1000} x hidden in {64, 128, 256}, with and without A,
out of place and over either input stack, against fp64 plane by plane.

Model level (hb._setup: 4096 points, latent 8^3, k = 8, r = 0.45, 300 + 300 queries partly outside the box): sample_laplacian_vjp with
random cotangents against the fp64 oracle's decoder differentiated twice in the query and then in the latent, on the lists the
streamed routes use, for 'knn' / 'radius' / 'bidirectional' and the SHAPES of the adjoint test (two softmax-weighted scales on
'radius' among them: the case where the Laplacian of the weights matters); cot_lap = 0 meets sample_jacobian_vjp within 1e-5 of the
peak; cot_pred / cot_jac = None; chunkings None / 250 / 64 each at the bar, within 1e-5 of the peak of one another, bit-reproducible,
the same bits in bf16 mode; sample_laplacian_autograd's forward is sample_laplacian(_rows) / sample_hessian(_rows) and its backward
sample_laplacian_vjp, bit for bit; a loss |lap - s|^2 + |jac . n|^2 chained through model.latent gives an encoder parameter the
gradient of the fp64 oracle of the whole model; timing keys; refusals; the row route in a capture.

Bars: the project's fp32 bar for derivatives (FP32_BAR: max error <= 1e-3 of the reference's peak, cosine >= 0.99999), every peak
asserted > 0.  Distances measured on an MI355X are quoted in DESIGN.md 3.2g."""
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
import gno_jet2_adj_ref as LA  # noqa: E402
import gno_rows_jac_ref as JREF  # noqa: E402  (ragged_list)
import test_coord_grad_gpu as cg  # noqa: E402  (_batch64)
import test_field_adjoint_gpu as ag  # noqa: E402  (the regular and hand-built lists, the models, SHAPES, the refusal table)
import test_field_hessian_gpu as hb  # noqa: E402  (the model fixture, the watcher, check(), the bar, the queries)
import test_field_jacobian_adjoint_gpu as jg  # noqa: E402  (_route_edges)
import test_field_jacobian_rows_gpu as jr  # noqa: E402  (the lists a-e, the device operands)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NSRC = jr.NSRC
FP32_BAR = hb.FP32_BAR
from gaot_3d_amd.model.layers.magno import MAGNODecoder  # noqa: E402

AXES = MAGNODecoder.LAP_VJP_DIRS                # the directions the decoder's adjoint runs along: the references use the same
assert AXES == LA.AXES
# generic directions with an axis and a sum of two axes among them; the first nd are the directions of a call
DIRS6 = (hb.GENERIC[0], (0.0, 1.0, 0.0), hb.GENERIC[2], (1.0, 0.0, 1.0), hb.GENERIC[4], hb.GENERIC[5])
NDS = (1, 3, 6)


def _cots(nd, nq, gen, shared):
    return torch.randn(nd, nq, 32, generator=gen), torch.randn(1 if shared else nd, nq, 32, generator=gen)


def _slice(jets, nd):
    return jets[0], jets[1][:nd], jets[2][:nd]


# ---- op level: regular lists ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh", [1, 2, 3, 4])
def test_regular_lists_meet_fp64_the_older_adjoints_and_the_duality(nh):
    from gaot_3d_amd import graph, ops
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(nh, "linear")
    worst_identity = worst = 0.0
    for nq in ag.NQS:
        for k in ag.KS:
            src, dst, rowptr, x, g = ag._regular(nq, k, gen)
            xd, gd, nbr = x.to(DEV), g.to(DEV), src.to(DEV)
            gs = graph.by_source((nbr, k), NSRC)
            jets6 = LA.kernel_jets2(ws, bs, y, x, src, dst, DIRS6)
            for nd in NDS:
                dirs, jets = DIRS6[:nd], _slice(jets6, nd)
                for shared in (False, True):
                    p, s = _cots(nd, nq, gen, shared)
                    pd, sd = p.to(DEV), s.to(DEV)
                    n0 = ops.launch_count()
                    got = ops.gno_adjoint_jet2(wd, bd, yd, xd, dirs, gd, pd, sd, gs, k)
                    assert ops.launch_count() == n0 + 2, (nq, k, nd, shared)                # the kernel and its fix-up
                    assert got.shape == (NSRC, 32) and got.dtype == torch.float32
                    ref = LA.adjoint_jet2_closed(ws, bs, y, x, src, dst, rowptr, dirs, g, p, s, NSRC, jets)
                    rel, _ = hb.check(f"gno_adj_jet2/nh{nh}/nq{nq}/k{k}/nd{nd}/{'one' if shared else 'per_dir'}", got, ref, quiet=True)
                    worst = max(worst, rel)
                    # <G, out> + sum <P_i, d1_i> + sum <S_i, d2_i> against <grad_f, f>, both sides in fp64
                    out, d1, d2 = ops.gno_forward_knn_jet2("linear", wd, bd, yd, xd, fd, None, nbr, k, dirs)
                    lhs = (g.double() * out.double().cpu()).sum().item() + (p.double() * d1.double().cpu()).sum().item() \
                        + (s.double().expand(nd, -1, -1) * d2.double().cpu()).sum().item()
                    rhs = (got.double().cpu() * f.double()).sum().item()
                    terms = LA.adjoint_jet2_terms(ws, bs, y, x, src, dst, rowptr, dirs, g, p, s, jets)
                    scale = (terms * f.double()[src.long()]).abs().sum().item()
                    assert scale > 0
                    worst_identity = max(worst_identity, abs(lhs - rhs) / scale)
                    assert abs(lhs - rhs) <= 1e-3 * scale, (nq, k, nd, shared, lhs, rhs, scale)
            # grad_d1 = grad_d2 = 0: the value adjoint, no further from fp64 than gno_adjoint
            ref0 = REF.gno_adjoint_closed(ws, bs, y, x, src, dst, rowptr, g, NSRC)
            peak0 = ref0.abs().max().item()
            assert peak0 > 0
            z3, z1 = torch.zeros(3, nq, 32, device=DEV), torch.zeros(1, nq, 32, device=DEV)
            d_new = ag._dist(ops.gno_adjoint_jet2(wd, bd, yd, xd, DIRS6[:3], gd, z3, z1, gs, k), ref0)
            d_old = ag._dist(ops.gno_adjoint(wd, bd, yd, xd, gd, gs, k), ref0)
            assert d_new <= max(4.0 * d_old, 1e-6 * peak0), (nq, k, d_new, d_old, peak0)
            # the three axes with grad_d2 = 0: the Jacobian's adjoint, no further from fp64 than gno_adjoint_jac
            gj = torch.randn(3, nq, 32, generator=gen)
            gjd = gj.to(DEV)
            ref1 = LA.adjoint_jet2_closed(ws, bs, y, x, src, dst, rowptr, AXES, g, gj, torch.zeros(1, nq, 32), NSRC)
            peak1 = ref1.abs().max().item()
            assert peak1 > 0
            j_new = ag._dist(ops.gno_adjoint_jet2(wd, bd, yd, xd, AXES, gd, gjd, z1, gs, k), ref1)
            j_old = ag._dist(ops.gno_adjoint_jac(wd, bd, yd, xd, gd, gjd, gs, k), ref1)
            assert j_new <= max(4.0 * j_old, 1e-6 * peak1), (nq, k, j_new, j_old, peak1)
            print(f"[adjoint_jet2] nh{nh} nq{nq} k{k}: P = S = 0: |adj_jet2 - fp64| = {d_new:.3e}, |gno_adj - fp64| = {d_old:.3e}, peak "
                  f"{peak0:.3e}; axes, S = 0: |adj_jet2 - fp64| = {j_new:.3e}, |gno_adj_jac - fp64| = {j_old:.3e}, peak {peak1:.3e}")
    print(f"[adjoint_jet2] nh{nh}: worst kernel / fp64 = {worst:.3e} of the peak; worst |<G, out> + <P, d1> + <S, d2> - <A^T, f>| / "
          f"sum|terms| = {worst_identity:.3e}")


def _raw(wd, bd, yd, xd, dirs, gd, pd, sd, g, k, fill):
    """gaot_gno_adj_jet2 through the C ABI into a result pre-filled with ``fill``"""
    from gaot_3d_amd import _lib, ops
    lib = _lib.load()
    m, keep = ops._mlp_struct(wd, bd)
    hd, nd = ops._host_dirs("raw", dirs)
    out = torch.full((g.num_src, 32), fill, dtype=torch.float32, device=DEV)
    e = g.by_src.num_edges
    ws = ops._ws(lib.gaot_gno_adj_jet2_workspace_bytes(e), DEV)
    stride = 0 if sd.shape[0] == 1 and nd > 1 else g.num_dst * 32
    rc = lib.gaot_gno_adj_jet2(C.byref(m), ops._ptr(yd), ops._ptr(xd), hd, nd, ops._ptr(gd), ops._ptr(pd), ops._ptr(sd), stride,
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
        g = torch.randn(nq, 32, generator=gen)
        gr = ag._both_lists(src, dst, nq)
        rs = gr.by_src.rowptr.cpu()
        if name == "long_row":
            assert int(rs[8] - rs[7]) == 200 and (int(rs[8]) - 1) // 32 - int(rs[7]) // 32 >= 5
        else:
            assert rs[:5].tolist() == [0, 32, 42, 64, 69]
        xd, gd = x.to(DEV), g.to(DEV)
        unused = torch.ones(NSRC, dtype=torch.bool)
        unused[src.long()] = False
        for nd, shared in ((3, True), (6, False)):
            dirs = DIRS6[:nd]
            p, s = _cots(nd, nq, gen, shared)
            pd, sd = p.to(DEV), s.to(DEV)
            got = _raw(wd, bd, yd, xd, dirs, gd, pd, sd, gr, None, float("nan"))
            ref = LA.adjoint_jet2_closed(ws, bs, y, x, src, dst, gr.by_dst.rowptr.cpu(), dirs, g, p, s, NSRC)
            assert not torch.isnan(got).any(), name
            assert unused.any() and torch.equal(got[unused.to(DEV)], torch.zeros(int(unused.sum()), 32, device=DEV)), name
            hb.check(f"gno_adj_jet2/nh{nh}/{name}/nd{nd}", got, ref)
            assert torch.equal(got, ops.gno_adjoint_jet2(wd, bd, yd, xd, dirs, gd, pd, sd, gr)), name


def test_no_edges_and_no_queries():
    from gaot_3d_amd import graph, ops
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(2, "linear")
    empty = lambda: torch.empty(0, dtype=torch.int32, device=DEV)
    zeros = torch.zeros(NSRC, 32, device=DEV)
    for nq in (5, 0):
        rows = ops.BipartiteGraph(ops.SortedEdges(torch.zeros(nq + 1, dtype=torch.int32, device=DEV), None, empty(), empty(), nq),
                                  None, NSRC, nq)
        gr = graph.by_source(rows, NSRC)
        xd, gd = torch.zeros(nq, 3, device=DEV), torch.ones(nq, 32, device=DEV)
        pd, sd = torch.ones(3, nq, 32, device=DEV), torch.ones(1, nq, 32, device=DEV)
        n0 = ops.launch_count()
        got = ops.gno_adjoint_jet2(wd, bd, yd, xd, AXES, gd, pd, sd, gr)
        assert ops.launch_count() == n0 + 1                                                # the fix-up alone writes the zeros
        assert torch.equal(got, zeros)
        assert torch.equal(_raw(wd, bd, yd, xd, AXES, gd, pd, sd, gr, None, float("nan")), zeros)
    gr = graph.by_source((empty(), 8), NSRC)                                               # zero queries of a regular list
    assert torch.equal(ops.gno_adjoint_jet2(wd, bd, yd, torch.zeros(0, 3, device=DEV), AXES, torch.zeros(0, 32, device=DEV),
                                            torch.zeros(3, 0, 32, device=DEV), torch.zeros(3, 0, 32, device=DEV), gr, 8), zeros)


@pytest.mark.parametrize("nh", [1, 2, 3, 4])
def test_ragged_lists_take_the_degree_from_rowptr_dst(nh):
    from gaot_3d_amd import graph, ops
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(nh, "linear")
    for i, (name, deg) in enumerate(jr.DEGREES.items()):
        nq = len(deg)
        nd, shared = NDS[i % 3], bool(i % 2)
        dirs = DIRS6[:nd]
        x = torch.rand(nq, 3, generator=gen) * 2 - 1
        g = torch.randn(nq, 32, generator=gen)
        p, s = _cots(nd, nq, gen, shared)
        src, dst, rowptr = JREF.ragged_list(deg, NSRC, gen)
        rows = jr._graph(src, dst, rowptr, NSRC)                                           # the forward-only graph query_lists returns
        gr = graph.by_source(rows, NSRC)
        xd, gd, pd, sd = x.to(DEV), g.to(DEV), p.to(DEV), s.to(DEV)
        n0 = ops.launch_count()
        got = ops.gno_adjoint_jet2(wd, bd, yd, xd, dirs, gd, pd, sd, gr)
        assert ops.launch_count() == n0 + 2, name
        jets = LA.kernel_jets2(ws, bs, y, x, src, dst, dirs)
        ref = LA.adjoint_jet2_closed(ws, bs, y, x, src, dst, rowptr, dirs, g, p, s, NSRC, jets)
        hb.check(f"gno_adj_jet2/nh{nh}/list_{name}/nd{nd}/{'one' if shared else 'per_dir'}", got, ref)
        assert torch.equal(got, ops.gno_adjoint_jet2(wd, bd, yd, xd, dirs, gd, pd, sd, gr)), name    # reproducible
        with hb._precision("bf16"):
            assert torch.equal(got, ops.gno_adjoint_jet2(wd, bd, yd, xd, dirs, gd, pd, sd, gr)), name   # exact fp32 in both modes
        # the duality on ragged rows, the jets from the jet kernel on the same by-query list
        out, d1, d2 = ops.gno_forward_jet2("linear", wd, bd, yd, xd, fd, None, rows, dirs)
        lhs = (g.double() * out.double().cpu()).sum().item() + (p.double() * d1.double().cpu()).sum().item() \
            + (s.double().expand(nd, -1, -1) * d2.double().cpu()).sum().item()
        rhs = (got.double().cpu() * f.double()).sum().item()
        terms = LA.adjoint_jet2_terms(ws, bs, y, x, src, dst, rowptr, dirs, g, p, s, jets)
        scale = (terms * f.double()[src.long()]).abs().sum().item()
        assert scale > 0 and abs(lhs - rhs) <= 1e-3 * scale, (name, lhs, rhs, scale)
        print(f"[adjoint_jet2] nh{nh} list_{name}: |<G, out> + <P, d1> + <S, d2> - <A^T, f>| / sum|terms| = {abs(lhs - rhs) / scale:.3e}")


def test_on_a_regular_list_k_and_rowptr_dst_agree_and_one_plane_is_three_copies():
    from gaot_3d_amd import graph, ops
    for nh in (1, 2, 3, 4):
        gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(nh, "linear")
        for nq, k in ((7, 4), (33, 32), (1000, 8), (33, 1)):
            src, dst, rowptr, x, g = ag._regular(nq, k, gen)
            p, s = _cots(3, nq, gen, True)
            xd, gd, pd, sd = x.to(DEV), g.to(DEV), p.to(DEV), s.to(DEV)
            run = lambda gr, *kk: ops.gno_adjoint_jet2(wd, bd, yd, xd, AXES, gd, pd, sd, gr, *kk)
            by_k = run(graph.by_source((src.to(DEV), k), NSRC), k)
            assert torch.equal(by_k, run(graph.by_source(jr._graph(src, dst, rowptr, NSRC), NSRC))), (nh, nq, k)
            assert torch.equal(by_k, run(ag._both_lists(src, dst, nq))), (nh, nq, k)
            with hb._precision("bf16"):
                assert torch.equal(by_k, run(graph.by_source((src.to(DEV), k), NSRC), k)), (nh, nq, k)
            # stride 0 reads ONE plane where stride Nq * 32 reads three equal ones: the same operations, the same bits
            three = ops.gno_adjoint_jet2(wd, bd, yd, xd, AXES, gd, pd, sd.expand(3, -1, -1).contiguous(),
                                         graph.by_source((src.to(DEV), k), NSRC), k)
            assert torch.equal(by_k, three), (nh, nq, k)


def test_bad_operands_raise_before_any_launch():
    from gaot_3d_amd import _lib, graph, ops
    from gaot_3d_amd._lib import GaotError
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(2, "linear")
    src, dst, rowptr, x, g = ag._regular(33, 8, gen)
    p, s = _cots(3, 33, gen, False)
    xd, gd, pd, sd = x.to(DEV), g.to(DEV), p.to(DEV), s.to(DEV)
    gr = graph.by_source((src.to(DEV), 8), NSRC)
    rows = jr._graph(src, dst, rowptr, NSRC)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    run = ops.gno_adjoint_jet2
    bad = [
        lambda: run(wd, bd, yd, xd, AXES, gd, pd[:, :, :16].contiguous(), sd, gr, 8),       # grad_d1: channels
        lambda: run(wd, bd, yd, xd, AXES, gd, pd[:, :20].contiguous(), sd, gr, 8),          # rows
        lambda: run(wd, bd, yd, xd, AXES, gd, pd[:2].contiguous(), sd, gr, 8),              # two planes for three directions
        lambda: run(wd, bd, yd, xd, AXES, gd, pd[:1].contiguous(), sd, gr, 8),              # grad_d1 has no one-plane form
        lambda: run(wd, bd, yd, xd, AXES, gd, pd.permute(1, 0, 2).contiguous().permute(1, 0, 2), sd, gr, 8),   # not contiguous
        lambda: run(wd, bd, yd, xd, AXES, gd, pd.double(), sd, gr, 8),
        lambda: run(wd, bd, yd, xd, AXES, gd, pd.cpu(), sd, gr, 8),
        lambda: run(wd, bd, yd, xd, AXES, gd, None, sd, gr, 8),
        lambda: run(wd, bd, yd, xd, AXES, gd, pd, sd[:2].contiguous(), gr, 8),              # grad_d2: neither nd nor one plane
        lambda: run(wd, bd, yd, xd, AXES, gd, pd, sd[:, :20].contiguous(), gr, 8),
        lambda: run(wd, bd, yd, xd, AXES, gd, pd, sd[0], gr, 8),                            # [Nq, 32]
        lambda: run(wd, bd, yd, xd, AXES, gd, pd, sd.double(), gr, 8),
        lambda: run(wd, bd, yd, xd, AXES, gd, pd, sd.cpu(), gr, 8),
        lambda: run(wd, bd, yd, xd, AXES, gd, pd, None, gr, 8),
        lambda: run(wd, bd, yd, xd, (), gd, pd[:0].contiguous(), sd[:0].contiguous(), gr, 8),            # no direction
        lambda: run(wd, bd, yd, xd, DIRS6 + (AXES[0],), gd, torch.zeros(7, 33, 32, device=DEV), sd[:1].contiguous(), gr, 8),   # seven
        lambda: run(wd, bd, yd, xd, ((1.0, 0.0),) * 3, gd, pd, sd, gr, 8),                 # directions of two components
        lambda: run(wd, bd, yd, xd, torch.eye(3, device=DEV), gd, pd, sd, gr, 8),           # directions on the device
        lambda: run(wd, bd, yd, xd, AXES, gd[:, :16].contiguous(), pd, sd, gr, 8),          # gno_adjoint's rules
        lambda: run(wd, bd, yd, xd, AXES, gd.double(), pd, sd, gr, 8),
        lambda: run(wd, bd, yd, xd, AXES, gd.cpu(), pd, sd, gr, 8),
        lambda: run(wd, bd, yd[:100].contiguous(), xd, AXES, gd, pd, sd, gr, 8),
        lambda: run(wd, bd, yd, xd[:, :2].contiguous(), AXES, gd, pd, sd, gr, 8),
        lambda: run(wd, bd, yd, xd, AXES, gd, pd, sd, gr),                                  # neither rowptr_dst nor k
        lambda: run(wd, bd, yd, xd, AXES, gd, pd, sd, gr, 4),                               # k that does not match the list
        lambda: run(wd, bd, yd, xd, AXES, gd, pd, sd, gr, 0),
        lambda: run(wd, bd, yd, xd, AXES, gd, pd, sd, rows),                                # no by-source list
        lambda: run(wd[:1], bd[:1], yd, xd, AXES, gd, pd, sd, gr, 8),                       # one linear layer
        lambda: run([wd[0][:32].contiguous(), wd[1][:32, :32].contiguous(), wd[2][:, :32].contiguous()],
                    [bd[0][:32].contiguous(), bd[1][:32].contiguous(), bd[2]], yd, xd, AXES, gd, pd, sd, gr, 8),   # hidden width 32
    ]
    for i, call in enumerate(bad):
        with pytest.raises(GaotError):
            call()
        assert ops.launch_count() == n0, i
    # the C ABI's own checks, before any launch
    lib = _lib.load()
    m, keep = ops._mlp_struct(wd, bd)
    out = torch.zeros(NSRC, 32, device=DEV)
    wsp = ops._ws(lib.gaot_gno_adj_jet2_workspace_bytes(gr.by_src.num_edges), DEV)
    hd, _ = ops._host_dirs("raw", AXES)
    plane = 33 * 32

    def raw(dirs=hd, nd=3, g1=pd, g2=sd, stride=plane):
        return lib.gaot_gno_adj_jet2(C.byref(m), ops._ptr(yd), ops._ptr(xd), dirs, nd, ops._ptr(gd), ops._ptr(g1), ops._ptr(g2), stride,
                                     ops._ptr(None), 8, ops._ptr(gr.by_src.key), ops._ptr(gr.by_src.other), ops._ptr(gr.by_src.rowptr),
                                     gr.by_src.num_edges, NSRC, 33, ops._ptr(out), ops._ptr(wsp), wsp.numel(), ops._stream())
    for kw, word in ((dict(g1=None), "grad_d1"), (dict(g2=None), "grad_d2"), (dict(stride=32), "grad_d2_stride"),
                     (dict(stride=2 * plane), "grad_d2_stride"), (dict(nd=0), "nd must be"), (dict(nd=7), "nd must be"),
                     (dict(dirs=None), "null dirs"), (dict(dirs=ops._ptr(xd)), "host pointer")):
        assert raw(**kw) != 0 and word in lib.gaot_last_error().decode(), (kw, lib.gaot_last_error())
        assert ops.launch_count() == n0, kw
    assert raw(stride=0) == 0 and raw() == 0


# ---- op level: the element kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [64, 128, 256])
def test_the_element_kernel_meets_fp64_plane_by_plane(hidden):
    from gaot_3d_amd import ops
    from gaot_3d_amd._lib import GaotError
    gen = torch.Generator().manual_seed(hidden)
    worst = 0.0
    for rows in (1, 33, 1000):
        zus = torch.randn(5, rows, hidden, generator=gen)
        zus[0] *= 2.0                                          # pre-activations over the range where phi matters and beyond it
        a5 = torch.randn(5, rows, hidden, generator=gen)
        b1 = 0.3 * torch.randn(hidden, generator=gen)
        zd, ad, bd = zus.to(DEV), a5.to(DEV), b1.to(DEV)
        for with_a in (True, False):
            ref = LA.lap_cot_mid(zus[0].double() + b1.double(), zus[1:4], zus[4], a5[0] if with_a else None, a5[1:4], a5[4])
            n0 = ops.launch_count()
            got = ops.mlp2_lap_cot_mid(zd, ad[0] if with_a else None, ad[1:4], ad[4], bd)
            assert ops.launch_count() == n0 + 1
            assert got.shape == (5, rows, hidden) and got.dtype == torch.float32 and got.data_ptr() not in (zd.data_ptr(), ad.data_ptr())
            for pl, name in enumerate(("dz", "du0", "du1", "du2", "ds")):
                rel, _ = hb.check(f"mlp2_lap_cot_mid/h{hidden}/rows{rows}/{'A' if with_a else 'noA'}/{name}", got[pl], ref[pl], quiet=True)
                worst = max(worst, rel)
            # over the z stack, and (with A) over the cotangent stack: the same bits
            zc = zd.clone()
            assert torch.equal(ops.mlp2_lap_cot_mid(zc, ad[0] if with_a else None, ad[1:4], ad[4], bd, out=zc), got)
            if with_a:
                ac = ad.clone()
                assert torch.equal(ops.mlp2_lap_cot_mid(zd, ac[0], ac[1:4], ac[4], bd, out=ac), got)
        no_bias = ops.mlp2_lap_cot_mid(zd, ad[0], ad[1:4], ad[4])
        hb.check(f"mlp2_lap_cot_mid/h{hidden}/rows{rows}/no_bias", no_bias, LA.lap_cot_mid(zus[0], zus[1:4], zus[4], a5[0], a5[1:4], a5[4]),
                 quiet=True)
    print(f"[lap_cot_mid] hidden {hidden}: worst plane / fp64 = {worst:.3e} of the plane's peak")
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    for call in (lambda: ops.mlp2_lap_cot_mid(zd[:4], ad[0], ad[1:4], ad[4]), lambda: ops.mlp2_lap_cot_mid(zd, ad[0], ad[1:3], ad[4]),
                 lambda: ops.mlp2_lap_cot_mid(zd, ad[0], ad[1:4], ad[4, :5]), lambda: ops.mlp2_lap_cot_mid(zd.double(), ad[0], ad[1:4], ad[4]),
                 lambda: ops.mlp2_lap_cot_mid(zd, ad[0].cpu(), ad[1:4], ad[4]), lambda: ops.mlp2_lap_cot_mid(zd, ad[0], ad[1:4], ad[4], bd[:8]),
                 lambda: ops.mlp2_lap_cot_mid(zd.transpose(1, 2), ad[0], ad[1:4], ad[4]),
                 lambda: ops.mlp2_lap_cot_mid(zd[:, :, :6].contiguous(), ad[0, :, :6].contiguous(), ad[1:4, :, :6].contiguous(),
                                              ad[4, :, :6].contiguous())):
        with pytest.raises(GaotError):
            call()
    assert ops.launch_count() == n0


# ---- model level ------------------------------------------------------------------------------------------------------------------------
CHUNKS = ag.CHUNKS
MODELS = ag.MODELS
SHAPES = ag.SHAPES
assert SHAPES["two_scales_weighted_radius"] == ("radius", dict(out=2, scales=[1.0, 2.0], use_scale_weights=True))


def _cots3(nq, out, seed=43, device=DEV):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(nq, out, generator=gen).to(device), torch.randn(nq, out, 3, generator=gen).to(device),
            torch.randn(nq, out, generator=gen).to(device))


def _lap_of(p, xg):
    """(jac [Nq, out, 3], lap [Nq, out]) of p [Nq, out] whose row q depends on xg[q] alone, both still differentiable"""
    jac = torch.stack([torch.autograd.grad(p[:, o].sum(), xg, create_graph=True)[0] for o in range(p.shape[1])], dim=1)
    lap = torch.stack([sum(torch.autograd.grad(jac[:, o, d].sum(), xg, create_graph=True)[0][:, d] for d in range(3))
                       for o in range(p.shape[1])], dim=1)
    return jac, lap


_REFS = {}


def _oracle_lap_vjp(key, model, cfg, lat, q, gy, gj, gl):
    """-> (pred, jac, lap, and the gradients with respect to the latent of sum(gy * pred), sum(gj * jac), sum(gl * lap)): the fp64
    oracle's decoder on the CPU on the lists the streamed routes use, differentiated twice in the query (create_graph=True, per output
    channel) and then in the latent; once per key"""
    if key in _REFS:
        return _REFS[key]
    edges, tok = jg._route_edges(model, cfg, lat, q)
    sd = {n: v.detach().double().cpu() for n, v in model.state_dict().items()}
    lat64 = lat.detach().double().cpu().requires_grad_(True)
    xg = q.detach().double().cpu().requires_grad_(True)
    p = orc.magno_decoder(sd, cfg.magno, lat64, xg, tok.double().cpu(), types.SimpleNamespace(**edges))
    jac, lap = _lap_of(p, xg)
    (from_lap,) = torch.autograd.grad((lap * gl.double().cpu()).sum(), lat64, retain_graph=True)
    (from_jac,) = torch.autograd.grad((jac * gj.double().cpu()).sum(), lat64, retain_graph=True)
    (from_pred,) = torch.autograd.grad((p * gy.double().cpu()).sum(), lat64)
    _REFS[key] = (p.detach(), jac.detach(), lap.detach(), from_pred, from_jac, from_lap)
    return _REFS[key]


def _keys_ok(seen, rows):
    keys = seen["keys"]
    fwd = "gno_jet2_rows_nh" if rows else "gno_jet2_knn_nh"
    return (any(k.startswith("gno_adj_jet2_nh") for k in keys) and any(k.startswith(fwd) for k in keys)
            and any(k.startswith("mlp2_lap_cot_mid_h") for k in keys)
            and not any(k.startswith("gno_bwd") or k.startswith("gno_adj_nh") or k.startswith("gno_adj_jac_nh") for k in keys))


@pytest.mark.parametrize("strategy", list(MODELS))
def test_sample_laplacian_vjp_meets_the_oracle_at_every_chunking(strategy, monkeypatch):
    key, (model, batch, tokens, cfg) = ag._model(strategy)
    q = hb._queries(batch)
    lat = ag._latent(model, batch, tokens)
    gy, gj, gl = _cots3(q.shape[0], 1)
    ref_p, ref_j, ref_l, r_pred, r_jac, r_lap = _oracle_lap_vjp(key, model, cfg, lat, q, gy, gj, gl)
    ref = r_pred + r_jac + r_lap
    assert r_lap.abs().max() > 1e-3 * ref.abs().max()                                       # the Laplacian's part is there to be seen
    got = {}
    for chunk in CHUNKS:
        with hb._watch(monkeypatch) as seen:
            got[chunk] = model.sample_laplacian_vjp(lat, q, gy, gj, gl, chunk_points=chunk)
        assert _keys_ok(seen, strategy != "knn"), seen
        assert got[chunk].shape == lat.shape and got[chunk].dtype == torch.float32
        assert not got[chunk].requires_grad and got[chunk].grad_fn is None
        hb.check(f"sample_laplacian_vjp/{strategy}/chunk{chunk}", got[chunk], ref)
        assert torch.equal(got[chunk], model.sample_laplacian_vjp(lat, q, gy, gj, gl, chunk_points=chunk)), chunk     # reproducible
    peak = ref.abs().max().item()
    for chunk in CHUNKS[1:]:
        d = (got[chunk] - got[None]).abs().max().item()
        print(f"[chunking] sample_laplacian_vjp/{strategy}: chunk {chunk} against one piece: max |d| = {d:.3e} = {d / peak:.3e} of the peak {peak:.3e}")
        assert d <= 1e-5 * peak, (chunk, d, peak)
    with hb._precision("bf16"):
        assert torch.equal(model.sample_laplacian_vjp(lat, q, gy, gj, gl, chunk_points=250), got[250])           # the same bits in both modes
    # the cotangents that may be None
    hb.check(f"sample_laplacian_vjp/{strategy}/lap_only", model.sample_laplacian_vjp(lat, q, None, None, gl, chunk_points=250), r_lap)
    hb.check(f"sample_laplacian_vjp/{strategy}/cot_pred_none", model.sample_laplacian_vjp(lat, q, None, gj, gl, chunk_points=250),
             r_jac + r_lap)
    hb.check(f"sample_laplacian_vjp/{strategy}/cot_jac_none", model.sample_laplacian_vjp(lat, q, gy, None, gl, chunk_points=250),
             r_pred + r_lap)
    # cot_lap = 0 is sample_jacobian_vjp
    zero = model.sample_laplacian_vjp(lat, q, gy, gj, torch.zeros_like(gl), chunk_points=250)
    vjp = model.sample_jacobian_vjp(lat, q, gy, gj, chunk_points=250)
    peak0 = (r_pred + r_jac).abs().max().item()
    d = (zero - vjp).abs().max().item()
    print(f"[jacobian] sample_laplacian_vjp/{strategy}: cot_lap = 0 against sample_jacobian_vjp: max |d| = {d:.3e} = {d / peak0:.3e} of the "
          f"peak {peak0:.3e}")
    assert peak0 > 0 and d <= 1e-5 * peak0, (d, peak0)
    # a latent that requires grad: still outside autograd
    out = model.sample_laplacian_vjp(model.latent(batch, tokens), q[:100], gy[:100].contiguous(), gj[:100].contiguous(),
                                     gl[:100].contiguous())
    assert not out.requires_grad


@pytest.mark.parametrize("case", list(SHAPES))
def test_other_shapes_meet_the_oracle(case, monkeypatch):
    strategy, kw = SHAPES[case]
    kw = dict(kw)
    out = kw.pop("out", 1)
    key, (model, batch, tokens, cfg) = ag._model(strategy, out=out, **kw)
    q = hb._queries(batch, 150, 150)
    lat = ag._latent(model, batch, tokens)
    gy, gj, gl = _cots3(q.shape[0], out)
    _, _, ref_l, r_pred, r_jac, r_lap = _oracle_lap_vjp(key + "/150", model, cfg, lat, q, gy, gj, gl)
    with hb._watch(monkeypatch) as seen:
        got = model.sample_laplacian_vjp(lat, q, gy, gj, gl, chunk_points=128)
    assert _keys_ok(seen, strategy != "knn"), seen
    hb.check(f"sample_laplacian_vjp/{case}", got, r_pred + r_jac + r_lap)
    hb.check(f"sample_laplacian_vjp/{case}/lap_only", model.sample_laplacian_vjp(lat, q, None, None, gl, chunk_points=128), r_lap)


@pytest.mark.parametrize("strategy", list(MODELS))
def test_sample_laplacian_autograd_is_the_forward_calls_and_its_vjp_backward(strategy):
    key, (model, batch, tokens, cfg) = ag._model(strategy)
    q = hb._queries(batch)
    lat = ag._latent(model, batch, tokens)
    gy, gj, gl = _cots3(q.shape[0], 1, seed=47)
    dec, tok = model.decoder, model._tokens(1, q.device, None, None)[0]
    with torch.no_grad():                                                                     # fp32 mode
        p0, l0 = dec.sample_laplacian_rows(lat, q, tok, chunk_points=250)                     # on 'knn' the call IS sample_laplacian
        _, j0, _ = dec.sample_hessian_rows(lat, q, tok, chunk_points=250)
    for mode in ("fp32", "bf16"):
        with hb._precision(mode):
            leaf = lat.clone().requires_grad_(True)
            pred, jac, lap = model.sample_laplacian_autograd(leaf, q, chunk_points=250)
            assert pred.requires_grad and jac.requires_grad and lap.requires_grad
            assert torch.equal(pred.detach(), p0) and torch.equal(jac.detach(), j0) and torch.equal(lap.detach(), l0), mode
            (grad,) = torch.autograd.grad((pred * gy).sum() + (jac * gj).sum() + (lap * gl).sum(), leaf, retain_graph=True)
            assert torch.equal(grad, model.sample_laplacian_vjp(lat, q, gy, gj, gl, chunk_points=250)), mode
            (grad,) = torch.autograd.grad((lap * gl).sum(), leaf, retain_graph=True)          # pred and jac got no gradient: None
            assert torch.equal(grad, model.sample_laplacian_vjp(lat, q, None, None, gl, chunk_points=250)), mode
            (grad,) = torch.autograd.grad((pred * gy).sum() + (jac * gj).sum(), leaf)         # lap got none: a zero cotangent
            assert torch.equal(grad, model.sample_laplacian_vjp(lat, q, gy, gj, torch.zeros_like(gl), chunk_points=250)), mode
    with pytest.raises(ValueError, match="query_pos requires grad"):
        model.sample_laplacian_autograd(lat.clone().requires_grad_(True), q.clone().requires_grad_(True))


@pytest.mark.parametrize("strategy", ["knn", "bidirectional"])
def test_a_residual_loss_reaches_an_encoder_parameter(strategy):
    """the loss |lap - s|^2 + |jac . n|^2 through sample_laplacian_autograd + the autograd of model.latent, against the fp64 oracle of
    the whole model on the route's decoder lists, differentiated twice in the query and then in the parameter"""
    key, (model, batch, tokens, cfg) = ag._model(strategy)
    q = hb._queries(batch)
    gen = torch.Generator().manual_seed(53)
    n = torch.nn.functional.normalize(torch.randn(q.shape[0], 3, generator=gen), dim=1).to(DEV)
    s = torch.randn(q.shape[0], 1, generator=gen).to(DEV)
    name = "encoder.gno.channel_mlp.fcs.0.weight"
    param = dict(model.named_parameters())[name]
    pred, jac, lap = model.sample_laplacian_autograd(model.latent(batch, tokens), q, chunk_points=250)
    loss = ((lap - s) ** 2).sum() + ((jac * n[:, None, :]).sum(-1) ** 2).sum()
    (got,) = torch.autograd.grad(loss, param)
    edges, tok = jg._route_edges(model, cfg, ag._latent(model, batch, tokens), q)
    sd = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    sd[name].requires_grad_(True)
    b64 = cg._batch64(batch.to("cpu"))
    for k, v in edges.items():
        setattr(b64, k, v)
    xg = q.detach().double().cpu().requires_grad_(True)
    p = orc.gaot3d_forward(sd, cfg, b64, tok.double().cpu(), query_coord_pos=xg)
    jac64, lap64 = _lap_of(p, xg)
    loss64 = ((lap64 - s.double().cpu()) ** 2).sum() + ((jac64 * n.double().cpu()[:, None, :]).sum(-1) ** 2).sum()
    (ref,) = torch.autograd.grad(loss64, sd[name])
    hb.check(f"sample_laplacian_autograd/{strategy}/residual_loss/encoder_parameter", got, ref)


@pytest.mark.parametrize("case", list(ag.REFUSALS))
def test_other_configurations_are_refused_before_any_launch(case):
    from gaot_3d_amd import ops
    strategy, k, kw, msg = ag.REFUSALS[case]
    model, batch, tokens, cfg = hb._setup(f"adjoint/refuse/{case}", k=k, **MODELS[strategy], **kw)
    lat = ag._latent(model, batch, tokens)
    q = batch.pos[:200].contiguous()
    gy, gj, gl = _cots3(200, 1)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    with pytest.raises(NotImplementedError, match="adjoint of the field's Laplacian.*" + msg):
        model.sample_laplacian_vjp(lat, q, gy, gj, gl)
    with pytest.raises(NotImplementedError, match="adjoint of the field's Laplacian.*" + msg):
        model.sample_laplacian_autograd(lat.clone().requires_grad_(True), q)
    assert ops.launch_count() == n0


def test_argument_rules_raise_on_the_device():
    from gaot_3d_amd import ops
    key, (model, batch, tokens, cfg) = ag._model("knn")
    lat = ag._latent(model, batch, tokens)
    q = batch.pos[:100].contiguous()
    gy, gj, gl = _cots3(100, 1)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    for bad in (gy.double(), gy.cpu(), gy[:50], torch.zeros(100, 2, device=DEV), torch.zeros(100, device=DEV)):
        with pytest.raises(ValueError, match="cot_pred"):
            model.sample_laplacian_vjp(lat, q, bad, gj, gl)
    for bad in (gj.double(), gj.cpu(), gj[:50], torch.zeros(100, 1, 2, device=DEV), torch.zeros(100, 3, device=DEV)):
        with pytest.raises(ValueError, match="cot_jac"):
            model.sample_laplacian_vjp(lat, q, gy, bad, gl)
    for bad in (gl.double(), gl.cpu(), gl[:50], torch.zeros(100, 2, device=DEV), torch.zeros(100, device=DEV), None):
        with pytest.raises(ValueError, match="cot_lap"):
            model.sample_laplacian_vjp(lat, q, gy, gj, bad)
    with pytest.raises(ValueError, match="chunk_points"):
        model.sample_laplacian_vjp(lat, q, gy, gj, gl, chunk_points=0)
    model.decoder.decoder_strategy = "reverse"
    try:
        with pytest.raises(ValueError, match="reverse"):
            model.sample_laplacian_vjp(lat, q, gy, gj, gl)
        with pytest.raises(ValueError, match="reverse"):
            model.sample_laplacian_autograd(lat, q)
    finally:
        model.decoder.decoder_strategy = "knn"
    model.decoder._shard_group = object()
    try:
        with pytest.raises(NotImplementedError, match="point-sharded"):
            model.sample_laplacian_vjp(lat, q, gy, gj, gl)
    finally:
        del model.decoder._shard_group
    model.decoder.projection.non_linearity = "relu"                                        # sample_jacobian_vjp's, not the Laplacian's
    try:
        with pytest.raises(NotImplementedError, match="adjoint of the field's Laplacian.*erf-GELU"):
            model.sample_laplacian_vjp(lat, q, gy, gj, gl)
        with pytest.raises(NotImplementedError, match="adjoint of the field's Laplacian.*erf-GELU"):
            model.sample_laplacian_autograd(lat.clone().requires_grad_(True), q)
    finally:
        model.decoder.projection.non_linearity = "gelu"
    assert ops.launch_count() == n0
    tok = model._tokens(1, q.device, None, None)[0]
    with pytest.raises(NotImplementedError, match="do not stream"):                         # tokens off the regular grid
        model.sample_laplacian_vjp(lat, q, gy, gj, gl, tokens_pos=(tok + 0.01 * torch.rand_like(tok)))


def test_in_a_capture_the_row_route_raises_before_any_launch():
    from gaot_3d_amd import ops
    from gaot_3d_amd._lib import GaotError
    key, (model, batch, tokens, cfg) = ag._model("bidirectional")
    q = batch.pos[:300].contiguous()
    lat = ag._latent(model, batch, tokens)
    gy, gj, gl = _cots3(300, 1)
    eager = model.sample_laplacian_vjp(lat, q, gy, gj, gl)            # describes the grid, warms the allocator
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(GaotError, match="captured"):
        with torch.cuda.graph(graph):
            model.sample_laplacian_vjp(lat, q, gy, gj, gl)
    assert ops.launch_count() == n0
    torch.cuda.synchronize()
    assert torch.equal(model.sample_laplacian_vjp(lat, q, gy, gj, gl), eager)
