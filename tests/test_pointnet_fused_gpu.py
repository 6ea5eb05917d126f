"""GPU: the fused PointNet GeometricEmbedding kernels (csrc/pointnet.hip, ops.pointnet_fwd / pointnet_bwd,
functional.PointNetPoolFn, GeometricEmbedding method='pointnet') against the fp64 CPU oracle (oracle/gaot_oracle.py::geoembed
on fp64 copies of the parameters and inputs).  Bars: the project's fp32 bars -- outputs rtol 1e-4 / atol 1e-5,
parameter and coordinate gradients rtol 1e-3 / atol 1e-5.  Every comparison prints a [parity] line."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import gaot_oracle as orc  # noqa: E402  (checker only)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUT_BAR = (1e-4, 1e-5)
GRAD_BAR = (1e-3, 1e-5)
Q, S = 300, 900
HUB, TIE, DEAD = 140, 10, 20          # rows of the adversarial graph
FAR = (890, 891, 892, 893)            # sources far away on axis 0: the neighbours of row DEAD


def close(name, got, ref, bar):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs().max().item() if got.numel() else 0.0
    print(f"[parity] {name}: max_abs={err:.3e} ref_peak={ref.abs().max().item() if ref.numel() else 0:.3e}")
    assert torch.isfinite(got).all(), name
    assert torch.allclose(got, ref, rtol=bar[0], atol=bar[1]), f"{name}: max abs err {err:.3e}"


@functools.lru_cache(maxsize=None)
def adversarial_edges():
    """~4 700 edges over 300 queries and 900 sources, shuffled: rows without edges at 0, at 299 and at 150..154; degrees
    1, 2, 3, 5, 7, 33, 65 repeated; a hub row of 1 500 edges (more than any workgroup's 256-edge tile) mid-list; row TIE = the same
    source twice (an exact tie); row DEAD = four sources so far away on axis 0 that the first layer is all negative"""
    gen = torch.Generator().manual_seed(1234)
    cycle = (1, 2, 3, 5, 7, 33, 65, 1, 2, 3, 5, 7)
    src, dst = [], []
    for r in range(Q):
        if r in (0, Q - 1) or 150 <= r < 155:
            continue
        if r == HUB:
            s = torch.cat([torch.randperm(890, generator=gen), torch.randint(0, 890, (1500 - 890,), generator=gen)])
        elif r == TIE:
            s = torch.tensor([77, 77])
        elif r == DEAD:
            s = torch.tensor(FAR)
        else:
            s = torch.randperm(890, generator=gen)[:cycle[r % len(cycle)]]
        src.append(s)
        dst.append(torch.full((s.numel(),), r))
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    return ei[:, torch.randperm(ei.shape[1], generator=gen)].contiguous()


@functools.lru_cache(maxsize=None)
def coords(d):
    gen = torch.Generator().manual_seed(99 + d)
    sp = torch.rand(S, d, generator=gen) * 2 - 1
    qp = torch.rand(Q, d, generator=gen) * 2 - 1
    sp[list(FAR), 0] = -50.0 - torch.arange(4.0)
    return sp, qp


def weights(d, seed=5):
    """(w1, b1, w2, b2) fp32.  Column 0 of w1 >= 0.1 and b2 < 0: an offset of -50 on axis 0 makes every z1 < 0, so z2 = b2 < 0"""
    gen = torch.Generator().manual_seed(seed + d)
    w1 = (torch.rand(32, d, generator=gen) - 0.5)
    w1[:, 0] = 0.1 + w1[:, 0].abs()
    b1 = (torch.rand(32, generator=gen) - 0.5)
    w2 = (torch.rand(32, 32, generator=gen) - 0.5) * 0.7
    b2 = -(0.01 + 0.1 * torch.rand(32, generator=gen))
    return w1, b1, w2, b2


def oracle_pool(ei, sp, qp, ws, pooling, seed=3):
    """the oracle with the identity as fc, so that its output IS its pooled rows (rows without edges: 0 either way)
    -> (pooled fp64, R, grads of sum(pooled * R) with respect to [sp, qp, w1, b1, w2, b2])"""
    leaves = [t.detach().double().clone().requires_grad_() for t in (sp, qp, *ws)]
    sd = {"pointnet_mlp.0.weight": leaves[2], "pointnet_mlp.0.bias": leaves[3], "pointnet_mlp.2.weight": leaves[4],
          "pointnet_mlp.2.bias": leaves[5], "fc.0.weight": torch.eye(32, dtype=torch.float64),
          "fc.0.bias": torch.zeros(32, dtype=torch.float64)}
    out = orc.geoembed(sd, "", leaves[0], leaves[1], ei, method="pointnet", pooling=pooling)
    r = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    grads = list(torch.autograd.grad((out * r).sum(), leaves))
    return out.detach(), r, grads


@functools.lru_cache(maxsize=None)
def direct_case(d, pooling):
    ei = adversarial_edges()
    sp, qp = coords(d)
    ws = weights(d)
    return (ei, sp, qp, ws) + oracle_pool(ei, sp, qp, ws, pooling)


def run_direct(ei, sp, qp, ws, r, mode, nq, ns):
    from gaot_3d_amd import ops
    g = ops.build_graph(ei.to(DEV), ns, nq)
    dev = [t.to(DEV) for t in (sp, qp, *ws)]
    pooled, arg = ops.pointnet_fwd(dev[0], dev[1], g, *dev[2:], mode)
    res = ops.pointnet_bwd(dev[0], dev[1], g, *dev[2:], mode, r.float().to(DEV), arg, want_source=True, want_query=True)
    torch.cuda.synchronize()
    return g, pooled, arg, res


@pytest.mark.parametrize("pooling", ["max", "mean"])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_ops_on_the_adversarial_graph(d, pooling):
    """ops.pointnet_fwd / pointnet_bwd directly: pooled, argmax, the four parameter gradients, d_source and d_query"""
    from gaot_3d_amd import edgeops as EO
    ei, sp, qp, ws, ref, r, gref = direct_case(d, pooling)
    mode = EO.MAX if pooling == "max" else EO.MEAN
    g, pooled, arg, (dw1, db1, dw2, db2, dsrc, dqry) = run_direct(ei, sp, qp, ws, r, mode, Q, S)
    tag = f"pointnet_ops/D{d}/{pooling}"
    close(f"{tag}/pooled", pooled, ref, OUT_BAR)
    rp = g.by_dst.rowptr.cpu().long()
    deg = rp[1:] - rp[:-1]
    assert deg[0] == 0 and deg[Q - 1] == 0 and (deg[150:155] == 0).all() and deg[HUB] == 1500 and deg.sum() == ei.shape[1]
    assert not pooled[deg.to(DEV) == 0].any(), "rows without edges must be zero"
    assert not pooled[DEAD].any() and not ref[DEAD].any(), "row DEAD: every z2 <= 0"
    if pooling == "max":
        # the oracle's h2 per edge in the dst-sorted order, rounded to fp32, reduced by the general kernel
        so, sk = g.by_dst.other.cpu().long(), g.by_dst.key.cpu().long()
        w1, b1, w2, b2 = (t.double() for t in ws)
        h1 = torch.relu((sp.double()[so] - qp.double()[sk]) @ w1.T + b1)
        h2 = torch.relu(h1 @ w2.T + b2)
        _, arg_ref = EO.segment_reduce(h2.float().to(DEV), g.by_dst.rowptr, None, Q, EO.MAX, want_argmax=True)
        gap = torch.full((Q, 32), float("inf"), dtype=torch.float64)
        for row in range(Q):
            if deg[row] >= 2:
                top = h2[rp[row]:rp[row + 1]].topk(2, dim=0).values
                gap[row] = top[0] - top[1]
        sure = (gap > 1e-5).to(DEV)
        assert arg.dtype == torch.int32 and (arg[deg.to(DEV) == 0] == -1).all()
        assert torch.equal(arg[sure], arg_ref[sure]), f"{tag}: argmax differs where the maximum is clear"
        print(f"[parity] {tag}/argmax: compared {int(sure.sum())} of {Q * 32} (row, channel) pairs, all equal")
        assert (arg[TIE] == int(rp[TIE])).all(), "an exact tie: the first edge wins"
        assert (arg[DEAD] == int(rp[DEAD])).all(), "all values equal (0): the first edge wins"
    close(f"{tag}/d_w1", dw1, gref[2], GRAD_BAR)
    close(f"{tag}/d_b1", db1, gref[3], GRAD_BAR)
    close(f"{tag}/d_w2", dw2, gref[4], GRAD_BAR)
    close(f"{tag}/d_b2", db2, gref[5], GRAD_BAR)
    close(f"{tag}/d_source", dsrc, gref[0], GRAD_BAR)
    close(f"{tag}/d_query", dqry, gref[1], GRAD_BAR)
    assert not dqry[DEAD].any() and not dsrc[list(FAR)].any(), "row DEAD passes no gradient on"
    # bit-reproducible
    _, pooled2, arg2, res2 = run_direct(ei, sp, qp, ws, r, mode, Q, S)
    assert torch.equal(pooled, pooled2) and (arg is None or torch.equal(arg, arg2))
    for a, b in zip((dw1, db1, dw2, db2, dsrc, dqry), res2):
        assert torch.equal(a, b)


@pytest.mark.parametrize("pooling", ["max", "mean"])
def test_ops_one_row_and_no_edges(pooling):
    """E = 5 over one query; E = 0 over four queries (zeros, -1, zero gradients)"""
    from gaot_3d_amd import edgeops as EO
    mode = EO.MAX if pooling == "max" else EO.MEAN
    gen = torch.Generator().manual_seed(8)
    ws = weights(3, seed=11)
    sp, qp = torch.rand(7, 3, generator=gen) * 2 - 1, torch.rand(1, 3, generator=gen) * 2 - 1
    ei = torch.tensor([[4, 0, 6, 2, 3], [0, 0, 0, 0, 0]])
    ref, r, gref = oracle_pool(ei, sp, qp, ws, pooling)
    _, pooled, arg, res = run_direct(ei, sp, qp, ws, r, mode, 1, 7)
    close(f"pointnet_ops/one_row/{pooling}/pooled", pooled, ref, OUT_BAR)
    for name, got, want in zip(("d_w1", "d_b1", "d_w2", "d_b2", "d_source", "d_query"), res, gref[2:] + gref[:2]):
        close(f"pointnet_ops/one_row/{pooling}/{name}", got, want, GRAD_BAR)
    qp4 = torch.rand(4, 3, generator=gen)
    r4 = torch.randn(4, 32, generator=gen, dtype=torch.float64)
    _, pooled, arg, res = run_direct(torch.zeros(2, 0, dtype=torch.long), sp, qp4, ws, r4, mode, 4, 7)
    assert pooled.shape == (4, 32) and not pooled.any()
    assert arg is None or (arg == -1).all()
    for t, shape in zip(res, ((32, 3), (32,), (32, 32), (32,), (7, 3), (4, 3))):
        assert tuple(t.shape) == shape and not t.any()


def _module(d, c, pooling, hidden=32):
    from gaot_3d_amd.model.layers.geoembed import GeometricEmbedding
    torch.manual_seed(100 * d + c)
    ge = GeometricEmbedding(d, c, method="pointnet", pooling=pooling)
    if hidden != 32:
        ge.pointnet_mlp = torch.nn.Sequential(torch.nn.Linear(d, hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, 32), torch.nn.ReLU())
    else:
        with torch.no_grad():       # row DEAD stays dead with the module's parameters too
            for p, w in zip((ge.pointnet_mlp[0].weight, ge.pointnet_mlp[0].bias, ge.pointnet_mlp[2].weight, ge.pointnet_mlp[2].bias),
                            weights(d, seed=21)):
                p.copy_(w)
    return ge.to(DEV)


def _module_against_oracle(ge, d, pooling, tag, coord_sets):
    ei = adversarial_edges()
    sp, qp = coords(d)
    names = [k for k, _ in ge.named_parameters()]
    sd = {k: v.detach().double().cpu().requires_grad_() for k, v in ge.state_dict().items()}
    s64, q64 = sp.double().requires_grad_(), qp.double().requires_grad_()
    ref = orc.geoembed(sd, "", s64, q64, ei, method="pointnet", pooling=pooling)
    r = torch.randn(ref.shape, generator=torch.Generator().manual_seed(17), dtype=torch.float64)
    gref = torch.autograd.grad((ref * r).sum(), [sd[k] for k in names] + [s64, q64])
    eid, rd = ei.to(DEV), r.float().to(DEV)
    for want_s, want_q in coord_sets:
        s = sp.to(DEV).requires_grad_(want_s)
        q = qp.to(DEV).requires_grad_(want_q)
        out = ge(s, q, eid)
        got = torch.autograd.grad((out * rd).sum(), list(ge.parameters()) + ([s] if want_s else []) + ([q] if want_q else []))
        t = f"{tag}/{'s' if want_s else ''}{'q' if want_q else ''}{'' if want_s or want_q else 'nocoord'}"
        close(f"{t}/out", out, ref, OUT_BAR)
        for k, a, b in zip(names, got, gref):
            close(f"{t}/grad/{k}", a, b, GRAD_BAR)
        if want_s:
            close(f"{t}/grad/source_pos", got[len(names)], gref[-2], GRAD_BAR)
        if want_q:
            close(f"{t}/grad/query_pos", got[-1], gref[-1], GRAD_BAR)


@pytest.mark.parametrize("pooling", ["max", "mean"])
@pytest.mark.parametrize("c", [16, 32])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_module_against_oracle(d, c, pooling):
    """GeometricEmbedding(D, C, 'pointnet', pooling) on the adversarial graph: output and all gradients, with no coordinate
    gradient, the sources' only and the queries' only; the fused kernels ran (ops.timing_summary)"""
    from gaot_3d_amd import ops
    ge = _module(d, c, pooling)
    ops.timing_reset(True)
    try:
        _module_against_oracle(ge, d, pooling, f"pointnet_module/D{d}/C{c}/{pooling}", ((False, False), (True, False), (False, True)))
        torch.cuda.synchronize()
        used = ops.timing_summary()
    finally:
        ops.timing_reset(False)
    assert used.get("pointnet_fwd", (0,))[0] == 3 and used.get("pointnet_bwd", (0,))[0] == 3, used


@pytest.mark.parametrize("pooling", ["max", "mean"])
def test_module_with_another_mlp_shape_keeps_the_general_path(pooling):
    """a pointnet_mlp with hidden width 48 is outside the fused kernels: the general per-edge path, same oracle, same bars"""
    from gaot_3d_amd import ops
    ge = _module(3, 32, pooling, hidden=48)
    ops.timing_reset(True)
    try:
        _module_against_oracle(ge, 3, pooling, f"pointnet_module/hidden48/{pooling}", ((True, True),))
        torch.cuda.synchronize()
        used = ops.timing_summary()
    finally:
        ops.timing_reset(False)
    assert "pointnet_fwd" not in used and "pointnet_bwd" not in used, used


def test_no_per_edge_tensor():
    """20 000 queries of degree 32 (E = 640 000): one forward + backward of the module allocates less than ONE [E, 32] fp32 tensor
    (81.9 MB) -- the general path keeps two of them and builds two more in the backward"""
    from gaot_3d_amd import ops
    from gaot_3d_amd.model.layers.geoembed import GeometricEmbedding
    nq, k, ns = 20000, 32, 5000
    e = nq * k
    gen = torch.Generator().manual_seed(0)
    ei = torch.stack([torch.randint(0, ns, (e,), generator=gen), torch.arange(nq).repeat_interleave(k)]).to(DEV)
    sp, qp = torch.rand(ns, 3, generator=gen).to(DEV), torch.rand(nq, 3, generator=gen).to(DEV)
    torch.manual_seed(0)
    ge = GeometricEmbedding(3, 32, method="pointnet", pooling="max").to(DEV)
    g = ops.build_graph(ei, ns, nq)
    r = torch.randn(nq, 32, generator=gen).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ge(sp, qp, ei, graph=g)
    (out * r).sum().backward()
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    print(f"[parity] pointnet peak memory growth over forward+backward at E={e}: {growth / 1e6:.1f} MB (one [E,32] tensor: {e * 128 / 1e6:.1f} MB)")
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in ge.parameters())
    assert growth < e * 32 * 4, f"{growth} bytes"


def test_graph_replay_is_bitwise_the_eager_step():
    """one forward + backward of the module (D = 3, max) eagerly, then captured with torch.cuda.graph after the warm-up: the
    replay gives the eager step's output and gradients bit for bit"""
    from gaot_3d_amd import ops
    ge = _module(3, 32, "max")
    ei = adversarial_edges().to(DEV)
    sp, qp = (t.to(DEV) for t in coords(3))
    g = ops.build_graph(ei, S, Q)
    r = torch.randn(Q, 32, generator=torch.Generator().manual_seed(2)).to(DEV)
    params = list(ge.parameters())

    def step():
        for p in params:
            p.grad = None
        out = ge(sp, qp, ei, graph=g)
        (out * r).sum().backward()
        return out.detach()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out_e = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out_e = out_e.clone()
    eager = [p.grad.clone() for p in params]
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="global"):
        out_g = step()
    graph.instantiate()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_g, out_e)
    assert all(torch.equal(p.grad, e) for p, e in zip(params, eager))
    del graph
