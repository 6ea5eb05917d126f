"""Streamed field sampling for 'radius' and 'bidirectional' decoders: graph.query_lists (the by-query neighbour list written row by row:
gaot_radius_grid_* for 'radius', the per-query union kernels gaot_nbr_union_grid_* for 'bidirectional') and MAGNODecoder.sample on it.

  * lists: rowptr / key / other of graph.query_lists are torch.equal to ops.csr_build(graph._decoder_edges(...), 1, Nq) -- forward's
    route through cat, coalesce and the stable sort by query -- on the grids (8, 8, 8) and (6, 5, 4), for random queries partly outside
    the box, all grid nodes, all cell centres (eight-way distance ties), Nq = 1 and 33, k in {1, 3, 8, 16}, r in {0.1, 0.45, 1.0}; the
    truth lists are checked to hold what the cases are for (a radius row cut at the cap, queries with and without a token within r,
    duplicates between the two sets);
  * empty rows: ops.gno_forward on the streamed 'radius' lists at r = 0.1 gives exact zero rows for queries without a neighbour and is
    torch.equal to ops.gno_forward on build_graph of the same edges, fp32 and bf16;
  * model level (4096 points, latent 8 x 8 x 8, r = 0.45, k = 8): sample against forward with edges built on the device, 'linear' /
    'nonlinear' transforms, both precisions, chunk_points None / 700, at the bounds of tests/test_field_sample_gpu.py.  Measured: 0
    in one pass; with chunks of 700 at most 5.7e-6 on predictions of peak 26 -- the lists are forward's, but a row that straddles two
    of the forward kernel's 32-edge tiles is summed from two partial sums, and where a row lies against the tiles depends on its
    offset in the launch, hence on the chunk (forward's own route differs from itself in the same way when it is chunked);
    sample builds no CSR and runs gno_fwd_nh* / gno_fwd_nl*, not gno_fwd_knn*;
  * use_attn and k = 40 'bidirectional' decoders still fall back and agree;
  * k beyond the token count and a non-positive radius raise GaotError without a launch, from query_lists and from the C entry points;
  * sample of a 'bidirectional' decoder inside a stream capture raises GaotError and leaves the device usable."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_field_sample_gpu as base  # noqa: E402  (the model fixture, the watchers and the bounds of the knn sampling tests)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRIDS = ((8, 8, 8), (6, 5, 4))
KS = (1, 3, 8, 16)
RADII = (0.1, 0.45, 1.0)
CAP = 32


def _grid(dims):
    from gaot_3d_amd import graph
    ax = [torch.linspace(-1, 1, n) for n in dims]
    tok = torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1).reshape(-1, 3).to(DEV)
    return graph.as_latent_grid(tok, dims)


def _queries(dims):
    gen = torch.Generator().manual_seed(7)
    rnd = torch.rand(3000, 3, generator=gen) * 2.4 - 1.2                          # some of them outside the grid's box
    ax = [torch.linspace(-1, 1, n) for n in dims]
    nodes = torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1).reshape(-1, 3)
    mid = [(a[1:] + a[:-1]) / 2 for a in ax]
    centres = torch.stack(torch.meshgrid(*mid, indexing="ij"), dim=-1).reshape(-1, 3)   # eight equidistant tokens each
    return {"random": rnd, "nodes": nodes, "centres": centres, "one": rnd[5:6].clone(), "thirty-three": rnd[100:133].clone()}


def _truth(strategy, q, grid, r, k):
    from gaot_3d_amd import graph, ops
    ei = graph._decoder_edges(strategy, q, grid, r, k)
    return ei, ops.csr_build(ei, 1, q.shape[0])


@pytest.mark.parametrize("strategy", ["radius", "bidirectional"])
@pytest.mark.parametrize("dims", GRIDS, ids=["8x8x8", "6x5x4"])
def test_lists_equal_forwards_route(dims, strategy):
    from gaot_3d_amd import graph
    grid = _grid(dims)
    seen = {"cap": False, "none": False, "some": False, "dup": False}
    cases = 0
    for name, q in _queries(dims).items():
        q = q.to(DEV)
        nq = q.shape[0]
        for r in RADII:
            _, rad = _truth("radius", q, grid, r, 1)
            deg = rad.rowptr[1:] - rad.rowptr[:-1]
            seen["cap"] |= r == 1.0 and int(deg.max()) == CAP
            if name == "random" and r == 0.1:
                seen["none"] |= bool((deg == 0).any())
                seen["some"] |= bool((deg > 0).any())
            for k in (KS if strategy == "bidirectional" else (1,)):
                _, ref = _truth(strategy, q, grid, r, k)
                if strategy == "bidirectional" and r == 0.45 and k == 8:
                    seen["dup"] |= ref.num_edges < nq * k + rad.num_edges
                got = graph.query_lists(strategy, q, grid, r, k)
                assert got.by_src is None and got.by_dst.perm is None
                assert (got.num_src, got.num_dst, got.by_dst.num_rows) == (grid.num_tokens, nq, nq)
                for f in ("rowptr", "key", "other"):
                    a, b = getattr(got.by_dst, f), getattr(ref, f)
                    assert a.dtype == b.dtype and torch.equal(a, b), (dims, strategy, name, r, k, f, a.shape, b.shape)
                cases += 1
    # the cases hold what they are for (dims 8x8x8: a ball of 1.0 holds ~180 tokens, the grid step is 0.286)
    if dims == (8, 8, 8):
        assert seen["cap"] and seen["none"] and seen["some"], seen
        assert seen["dup"] or strategy == "radius", seen
    print(f"[parity] query_lists/{strategy}/{'x'.join(map(str, dims))}: {cases} lists equal to forward's route")


@pytest.mark.parametrize("precision", [0, 1], ids=["fp32", "bf16"])
def test_empty_rows_are_exact_zeros(precision):
    from gaot_3d_amd import graph, ops
    grid = _grid((8, 8, 8))
    q = _queries((8, 8, 8))["random"].to(DEV)
    gen = torch.Generator().manual_seed(3)
    dims = [6, 64, 64, 32]
    ws = [(torch.randn(dims[i + 1], dims[i], generator=gen) / math.sqrt(dims[i])).to(DEV) for i in range(3)]
    bs = [(0.1 * torch.randn(dims[i + 1], generator=gen)).to(DEV) for i in range(3)]
    f = torch.randn(grid.num_tokens, 32, generator=gen).to(DEV)
    ei, _ = _truth("radius", q, grid, 0.1, 1)
    rows = graph.query_lists("radius", q, grid, 0.1, 1)
    ref = ops.gno_forward(ws, bs, grid.pos, q, f, ops.build_graph(ei, grid.num_tokens, q.shape[0]), precision=precision)
    got = ops.gno_forward(ws, bs, grid.pos, q, f, rows, precision=precision)
    empty = (rows.by_dst.rowptr[1:] == rows.by_dst.rowptr[:-1])
    assert bool(empty.any()) and not bool(empty.all())
    assert torch.equal(got[empty], torch.zeros_like(got[empty]))
    assert bool((got[~empty] != 0).any())
    assert torch.equal(got, ref)


# ---- model level ------------------------------------------------------------------------------------------------------------------------
DECODERS = {
    "radius": dict(neighbor_strategy=["knn", "radius"], gno_radius=0.45),
    "bidirectional": dict(neighbor_strategy="bidirectional", gno_radius=0.45),
}


def _model(strategy, tt="linear", k=8, **more):
    key = f"rows/{strategy}/{tt}/k{k}/" + ",".join(f"{a}={b}" for a, b in sorted(more.items()))
    return base._setup(key, k=k, out_gno_transform_type=tt, **DECODERS[strategy], **more)


def _streamed_rows(seen):
    keys = seen["keys"]
    return (seen["csr"] == 0 and not any(k.startswith("csr_build") or k.startswith("gno_fwd_knn") for k in keys)
            and any(k.startswith("gno_fwd_nh") or k.startswith("gno_fwd_nl") for k in keys))


@pytest.mark.parametrize("chunk", [None, 700])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("tt", ["linear", "nonlinear"])
@pytest.mark.parametrize("strategy", list(DECODERS))
def test_sample_streams_and_equals_forward(strategy, tt, precision, chunk, monkeypatch):
    model, batch, tokens = _model(strategy, tt)
    q = batch.pos
    with base._precision(precision), torch.no_grad():
        ref = base._forward_at(model, batch, tokens, q)
        lat = model.latent(batch, tokens)
        with base._watch(monkeypatch) as seen:
            got = model.sample(lat, q, chunk_points=chunk)
    assert got.shape == ref.shape and not got.requires_grad
    base._agree(f"sample_rows/{strategy}/{tt}/{precision}/chunk{chunk}", got, ref, precision)
    assert _streamed_rows(seen), seen


@pytest.mark.parametrize("case", ["use_attn", "k40"])
def test_still_falling_back_and_agreeing(case, monkeypatch):
    model, batch, tokens = _model("bidirectional", k=40) if case == "k40" else _model("bidirectional", use_attn=True)
    q = base._other_queries()["random"][:1500].to(DEV)
    for precision in ("fp32", "bf16"):
        with base._precision(precision), torch.no_grad():
            ref = base._forward_at(model, batch, tokens, q)
            lat = model.latent(batch, tokens)
            with base._watch(monkeypatch) as seen:
                got = model.sample(lat, q, chunk_points=700)
        base._agree(f"sample_rows_fallback/{case}/{precision}", got, ref, precision)
        assert seen["csr"] > 0, seen                           # forward's route: the lists are sorted


# ---- arguments --------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_launch():
    from gaot_3d_amd import _lib, graph, ops
    from gaot_3d_amd._lib import GaotError
    lib = _lib.load()
    grid = _grid((2, 3, 2))                                    # 12 tokens
    q = _queries((2, 3, 2))["thirty-three"].to(DEV)
    n = q.shape[0]
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    with pytest.raises(GaotError, match="k must be"):
        graph.query_lists("bidirectional", q, grid, 0.5, 13)
    for r in (0.0, -1.0):
        for strategy in ("radius", "bidirectional"):
            with pytest.raises(GaotError, match="radius must be positive"):
                graph.query_lists(strategy, q, grid, r, 1)
    assert ops.launch_count() == n0
    # the entry points themselves
    gs = grid.c_struct()
    counts = torch.zeros(n, dtype=torch.int32, device=DEV)
    offs = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    oq, ot = torch.zeros(n * 40, dtype=torch.int32, device=DEV), torch.zeros(n * 40, dtype=torch.int32, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)

    def count(pos=ptr(q), g=C.byref(gs), tok=ptr(grid.pos), k=3, r=0.5, cap=CAP, out=ptr(counts), num=n):
        _lib.check(lib.gaot_nbr_union_grid_count(pos, num, g, tok, k, r, cap, out, null), "gaot_nbr_union_grid_count")

    def fill(pos=ptr(q), g=C.byref(gs), tok=ptr(grid.pos), k=3, r=0.5, cap=CAP, off=ptr(offs), a=ptr(oq), b=ptr(ot), num=n):
        _lib.check(lib.gaot_nbr_union_grid_fill(pos, num, g, tok, k, r, cap, off, a, b, null), "gaot_nbr_union_grid_fill")

    for fn in (count, fill):
        for kw, msg in ((dict(k=13), "k must be"), (dict(k=0), "k must be"), (dict(r=0.0), "radius must be positive"),
                        (dict(r=-0.5), "radius must be positive"), (dict(cap=0), "cap must be"), (dict(pos=null), "null pointer"),
                        (dict(tok=null), "null pointer"), (dict(g=None), "bad grid"), (dict(num=1 << 26), "beyond int32")):
            with pytest.raises(GaotError, match=msg):
                fn(**kw)
    with pytest.raises(GaotError, match="null pointer"):
        count(out=null)
    for kw in (dict(off=null), dict(a=null), dict(b=null)):
        with pytest.raises(GaotError, match="null pointer"):
            fill(**kw)
    with pytest.raises(GaotError, match="k beyond 32"):
        _lib.check(lib.gaot_nbr_union_grid_count(ptr(q), n, C.byref(_grid((4, 4, 4)).c_struct()), ptr(grid.pos), 33, 0.5, CAP,
                                                 ptr(counts), null), "gaot_nbr_union_grid_count")
    assert ops.launch_count() == n0
    rows = graph.query_lists("bidirectional", q, grid, 0.5, 3)             # and a good call: count, the scan's three, fill
    assert ops.launch_count() == n0 + 5
    assert int(rows.by_dst.rowptr[-1]) == rows.by_dst.num_edges >= 3 * n


def test_sample_in_a_capture_raises_and_the_device_stays_usable():
    from gaot_3d_amd._lib import GaotError
    model, batch, tokens = _model("bidirectional")
    q = batch.pos[:1000].contiguous()
    with torch.no_grad():
        lat = model.latent(batch, tokens)
        eager = model.sample(lat, q)                          # describes the grid, warms the allocator
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with pytest.raises(GaotError, match="captured"):
            with torch.cuda.graph(g):
                model.sample(lat, q)
        torch.cuda.synchronize()
        again = model.sample(lat, q)
        torch.cuda.synchronize()
    assert torch.equal(again, eager)
