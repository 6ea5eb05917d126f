"""The streamed field Jacobian on ROW lists: gaot_gno_fwd_jac (the tangent kernel of gaot_gno_fwd_knn_jac on the ragged by-query list of
any graph, finished by segment_walk and one four-plane fix-up), ops.gno_forward_jac, IntegralTransform.jacobian_rows and
MAGNODecoder / GAOT3D.sample_jacobian(row_lists=True) for 'radius' and 'bidirectional' decoders.

  * op level, 1..4 hidden layers x the three transform types, 211 sources, on the lists
      a  five edges in one row                       b  40 queries of 0..9 edges, the first, a middle and the last row empty
      c  a row of 70 edges between short rows (one 32-edge tile lies wholly inside it)
      d  64 edges with a row boundary on the tile boundary
      e  3000 queries of 0..24 edges: more than 1024 tiles, so the kernel's grid-stride loop runs
    the value plane is torch.equal to ops.gno_forward / gno_nl_forward(precision=0) on the same lists, the Jacobian meets the fp32 bar
    for coordinate gradients (tests/test_coord_grad_gpu.py FP32_BAR: max error <= 1e-3 of the reference's peak, cosine >= 0.99999)
    against the closed-form fp64 reference tests/gno_rows_jac_ref.py, empty rows are exact zeros in all four planes, two launches;
  * regular lists (k in {1, 4, 32}, Nq in {7, 33}): all four planes torch.equal to ops.gno_forward_knn_jac;
  * bad arguments raise GaotError before any launch; zero queries launch nothing; zero edges: the fix-up alone writes zeros;
  * model level (4096 points, latent 8 x 8 x 8, r = 0.45, k = 8; 3000 queries partly outside the box), row_lists=True: gno_fwd_jac*
    keys, no CSR build, no gno_bwd*; pred torch.equal to sample; the Jacobian meets the bar against the one assembled from
    forward(query_coord_pos=q.requires_grad_()); bf16 mode returns the fp32-mode result; two scales with softmax weights (the weight
    tangent), summed scales, 'nonlinear', 16 lifting channels; without the flag no gno_fwd_jac key; a 'knn' decoder ignores the flag;
    inside a stream capture the flagged call raises GaotError with no launch;
  * chunkings None / 1000 / 64 are bit-identical (every chunk's list is led by padding edges that put its rows against the 32-edge
    tiles where the list of all queries has them), and a list with leading padding edges gives the rows of the longer list it is a
    piece of, bit for bit, at the op level;
  * memory: nothing but the results grows with Nq, and the route needs less than the default route at 200 K queries in one piece."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gno_rows_jac_ref as REF  # noqa: E402
import test_field_jacobian_gpu as jb  # noqa: E402  (the model fixture, the watchers, check() and the bar of the knn Jacobian tests)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = jb.MODES
NSRC = jb.NSRC
FP32_BAR = jb.FP32_BAR


# ---- op level ---------------------------------------------------------------------------------------------------------------------------
def _degrees():
    gen = torch.Generator().manual_seed(31)
    b = torch.randint(0, 10, (40,), generator=gen)
    b[0] = b[20] = b[39] = 0
    b[1], b[21] = 9, 5
    e = torch.randint(0, 25, (3000,), generator=gen)
    return {"a": [5], "b": b.tolist(), "c": [3, 2, 70, 1, 4], "d": [10, 22, 7, 25], "e": e.tolist()}


DEGREES = _degrees()
assert sum(DEGREES["d"]) == 64 and sum(DEGREES["d"][:2]) == 32
assert (sum(DEGREES["e"]) + 31) // 32 > 1024 and min(DEGREES["e"]) == 0 and max(DEGREES["e"]) == 24
assert sum(DEGREES["c"][:2]) <= 32 and sum(DEGREES["c"][:3]) >= 64                       # tile 1 lies wholly inside the long row


def _graph(src, dst, rowptr, nsrc):
    from gaot_3d_amd import ops
    nq = rowptr.numel() - 1
    return ops.BipartiteGraph(ops.SortedEdges(rowptr.to(DEV), None, dst.to(DEV), src.to(DEV), nq), None, nsrc, nq)


def _device_operands(nh, mode):
    gen, y, f, ws, bs = jb._operands(nh, mode)
    yd, fd = y.to(DEV), f.to(DEV)
    wd, bd = [w.to(DEV) for w in ws], [b.to(DEV) for b in bs]
    t = None
    if mode != "linear":
        t = (f.double() @ ws[0][:, 6:].double().t()).float().to(DEV)       # the per-node term of layer 0, as the host layer forms it
        wd = [ws[0][:, :6].contiguous().to(DEV)] + wd[1:]
    fk = None if mode == "nonlinear_kernelonly" else fd
    return gen, y, f, ws, bs, yd, wd, bd, fk, t


def _forward(mode, wd, bd, yd, xd, fk, t, g):
    from gaot_3d_amd import ops
    if mode == "linear":
        return ops.gno_forward(wd, bd, yd, xd, fk, g, precision=0)
    return ops.gno_nl_forward(mode, wd, bd, yd, xd, fk, t, g, precision=0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nh", [1, 2, 3, 4])
def test_value_is_the_forward_and_jacobian_meets_the_bar(nh, mode):
    from gaot_3d_amd import ops
    gen, y, f, ws, bs, yd, wd, bd, fk, t = _device_operands(nh, mode)
    for name, deg in DEGREES.items():
        nq = len(deg)
        x = torch.rand(nq, 3, generator=gen) * 2 - 1
        src, dst, rowptr = REF.ragged_list(deg, NSRC, gen)
        g = _graph(src, dst, rowptr, NSRC)
        xd = x.to(DEV)
        n0 = ops.launch_count()
        out, jac = ops.gno_forward_jac(mode, wd, bd, yd, xd, fk, t, g)
        assert ops.launch_count() == n0 + 2, name                                            # the tangent kernel and the fix-up
        assert out.shape == (nq, 32) and jac.shape == (3, nq, 32) and jac.is_contiguous()
        val = _forward(mode, wd, bd, yd, xd, fk, t, g)
        assert torch.equal(out, val), (name, (out - val).abs().max().item())
        empty = (torch.tensor(deg) == 0).to(DEV)
        assert torch.equal(out[empty], torch.zeros_like(out[empty])), name
        assert torch.equal(jac[:, empty], torch.zeros_like(jac[:, empty])), name
        ro, rj = REF.gno_rows_jac(ws, bs, y, x, src, dst, rowptr, f, mode)
        assert torch.allclose(out.cpu().double(), ro, rtol=1e-4, atol=1e-5), name
        jb.check(f"gno_fwd_jac/{mode}/nh{nh}/list_{name}", jac, rj)


@pytest.mark.parametrize("mode", MODES)
def test_regular_lists_equal_the_knn_kernel(mode):
    from gaot_3d_amd import ops
    for nh in (1, 2, 3, 4):
        gen, y, f, ws, bs, yd, wd, bd, fk, t = _device_operands(nh, mode)
        for nq in (7, 33):
            xd = (torch.rand(nq, 3, generator=gen) * 2 - 1).to(DEV)
            for k in (1, 4, 32):
                src, dst, rowptr = REF.ragged_list([k] * nq, NSRC, gen)
                out, jac = ops.gno_forward_jac(mode, wd, bd, yd, xd, fk, t, _graph(src, dst, rowptr, NSRC))
                ko, kj = ops.gno_forward_knn_jac(mode, wd, bd, yd, xd, fk, t, src.to(DEV), k)
                assert torch.equal(out, ko), (nh, nq, k)
                assert torch.equal(jac, kj), (nh, nq, k, (jac - kj).abs().max().item())


@pytest.mark.parametrize("mode", MODES)
def test_a_piece_led_by_padding_edges_equals_its_rows_in_the_whole_list(mode):
    """rows [a, b) of list e, cut out and led by (edges before row a) mod 32 padding edges (query id -1, rowptr starting at the
    padding): all four planes of those rows are the whole list's, bit for bit -- what makes sample_jacobian independent of its chunks"""
    from gaot_3d_amd import ops
    gen, y, f, ws, bs, yd, wd, bd, fk, t = _device_operands(2, mode)
    deg = DEGREES["e"]
    nq = len(deg)
    xd = (torch.rand(nq, 3, generator=gen) * 2 - 1).to(DEV)
    src, dst, rowptr = REF.ragged_list(deg, NSRC, gen)
    out, jac = ops.gno_forward_jac(mode, wd, bd, yd, xd, fk, t, _graph(src, dst, rowptr, NSRC))
    for a, b in ((0, 1000), (1000, 1064), (1064, 3000), (2990, 3000)):
        e0, e1 = int(rowptr[a]), int(rowptr[b])
        lead = e0 % 32
        psrc = torch.cat([torch.zeros(lead, dtype=torch.int32), src[e0:e1]])
        pdst = torch.cat([torch.full((lead,), -1, dtype=torch.int32), dst[e0:e1] - a])
        prow = rowptr[a:b + 1] - e0 + lead
        po, pj = ops.gno_forward_jac(mode, wd, bd, yd, xd[a:b].contiguous(), fk, t, _graph(psrc, pdst, prow, NSRC))
        assert torch.equal(po, out[a:b]) and torch.equal(pj, jac[:, a:b]), (a, b)


def test_bad_arguments_raise_before_any_launch():
    from gaot_3d_amd import _lib, ops
    from gaot_3d_amd._lib import GaotError
    lib = _lib.load()
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = _device_operands(2, "linear")
    deg = DEGREES["b"]
    nq = len(deg)
    src, dst, rowptr = REF.ragged_list(deg, NSRC, gen)
    g = _graph(src, dst, rowptr, NSRC)
    e = g.by_dst.num_edges
    xd = (torch.rand(nq, 3, generator=gen) * 2 - 1).to(DEV)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    w128, b128 = jb._mlp(2, "linear", gen, hidden=128)
    with pytest.raises(GaotError, match="gaot_gno_fwd_jac: unsupported MLP shape"):
        ops.gno_forward_jac("linear", [w.to(DEV) for w in w128], [b.to(DEV) for b in b128], yd, xd, fd, None, g)
    with pytest.raises(GaotError, match="mode must be"):
        ops.gno_forward_jac("cubic", wd, bd, yd, xd, fd, None, g)
    with pytest.raises(GaotError, match="rows, the graph"):
        ops.gno_forward_jac("linear", wd, bd, yd, xd[:-1], fd, None, g)
    assert ops.launch_count() == n0
    m, keep = ops._mlp_struct(wd, bd)
    out = torch.empty(nq, 32, device=DEV)
    jac = torch.empty(3, nq, 32, device=DEV)
    need = lib.gaot_gno_fwd_jac_workspace_bytes(e)
    assert need == 1024 * ((e + 31) // 32)
    ws_ = torch.empty(need, dtype=torch.uint8, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)
    by = g.by_dst

    def call(mode=0, yp=ptr(yd), xp=ptr(xd), fp=ptr(fd), tab=null, s=ptr(by.other), d=ptr(by.key), rp=ptr(by.rowptr), ne=e, q=nq,
             o=ptr(out), j=ptr(jac), w=ptr(ws_), wb=need):
        _lib.check(lib.gaot_gno_fwd_jac(C.byref(m), mode, yp, xp, fp, tab, s, d, rp, ne, q, o, j, w, wb, null), "gaot_gno_fwd_jac")

    for kw, msg in ((dict(mode=3), "mode must be"), (dict(j=null), "null pointer"), (dict(o=null), "null pointer"),
                    (dict(fp=null), "null pointer"), (dict(s=null), "null pointer"), (dict(d=null), "null pointer"),
                    (dict(rp=null), "null pointer"), (dict(yp=null), "null pointer"), (dict(xp=null), "null pointer"),
                    (dict(mode=1), "null src_table"), (dict(w=null), "null workspace"), (dict(wb=need - 1), "workspace too small"),
                    (dict(ne=-1), "negative size"), (dict(q=-1), "negative size"), (dict(ne=1 << 31), "beyond int32")):
        with pytest.raises(GaotError, match="gaot_gno_fwd_jac: .*" + msg):
            call(**kw)
        assert ops.launch_count() == n0, kw
    call(q=0)                                                                                # zero queries: no launch
    assert ops.launch_count() == n0
    out.fill_(1.0)
    jac.fill_(1.0)
    zero_rows = torch.zeros(nq + 1, dtype=torch.int32, device=DEV)
    call(ne=0, rp=ptr(zero_rows), s=null, d=null, w=null, wb=0, fp=null, yp=null, xp=null)   # zero edges: the fix-up alone, zeros
    assert ops.launch_count() == n0 + 1
    assert not out.any() and not jac.any()
    call()                                                                                   # and a good call: TWO launches
    assert ops.launch_count() == n0 + 3
    good = ops.gno_forward_jac("linear", wd, bd, yd, xd, fd, None, g)
    assert torch.equal(out, good[0]) and torch.equal(jac, good[1])


def test_jacobian_rows_pads_coordinate_dimension_two_with_exact_zeros():
    from gaot_3d_amd import ops
    from gaot_3d_amd.model.layers.integral_transform import IntegralTransform
    torch.manual_seed(3)
    it = IntegralTransform(channel_mlp_layers=[4, 64, 64, 32], transform_type="linear", coord_dim=2).to(DEV).eval()
    gen = torch.Generator().manual_seed(4)
    deg = DEGREES["b"]
    nq = len(deg)
    y = (torch.rand(NSRC, 2, generator=gen) * 2 - 1).to(DEV)
    x = (torch.rand(nq, 2, generator=gen) * 2 - 1).to(DEV)
    f = torch.randn(NSRC, 32, generator=gen).to(DEV)
    src, dst, rowptr = REF.ragged_list(deg, NSRC, gen)
    out, jac = it.jacobian_rows(y, x, f, _graph(src, dst, rowptr, NSRC))
    assert out.shape == (nq, 32) and jac.shape == (3, nq, 32)
    assert torch.equal(jac[2], torch.zeros_like(jac[2]))
    ei = torch.stack([src, dst]).to(DEV)
    xg = x.clone().requires_grad_(True)
    o = it(y, xg, ei, f, graph=ops.build_graph(ei, NSRC, nq))
    assert torch.equal(out, o.detach())
    ref = torch.stack([torch.autograd.grad(o[:, c].sum(), xg, retain_graph=c < 31)[0] for c in range(32)], dim=-1)   # [Nq, 2, C]
    jb.check("jacobian_rows/coord_dim2", jac[:2], ref.permute(1, 0, 2))


# ---- model level ------------------------------------------------------------------------------------------------------------------------
DECODERS = {
    "radius": dict(neighbor_strategy=["knn", "radius"], gno_radius=0.45),
    "bidirectional": dict(neighbor_strategy="bidirectional", gno_radius=0.45),
}
CHUNKS = (None, 1000, 64)


def _model(strategy, out=1, **more):
    key = f"jac_rows/{strategy}/out{out}/" + ",".join(f"{a}={b}" for a, b in sorted(more.items()))
    return key, jb._setup(key, k=8, out=out, **DECODERS[strategy], **more)


def _streamed_rows(seen):
    keys = seen["keys"]
    return (any(k.startswith("gno_fwd_jac") for k in keys) and seen["csr"] == 0
            and not any(k.startswith("csr_build") or k.startswith("gno_bwd") or k.startswith("gno_fwd_knn") for k in keys))


_GOT = {}


def _streamed_results(strategy, monkeypatch):
    """sample_jacobian(row_lists=True) of the 3000 random queries at every chunking, with the keys it ran: computed once per strategy"""
    if strategy not in _GOT:
        key, (model, batch, tokens) = _model(strategy)
        q = jb._queries("random", batch)
        with torch.no_grad():
            lat = model.latent(batch, tokens)
        got = {}
        for chunk in CHUNKS:
            with jb._watch(monkeypatch) as seen:
                got[chunk] = model.sample_jacobian(lat, q, chunk_points=chunk, row_lists=True)
            assert _streamed_rows(seen), seen
        _GOT[strategy] = (key, model, batch, tokens, q, lat, got)
    return _GOT[strategy]


@pytest.mark.parametrize("strategy", list(DECODERS))
def test_row_lists_stream_and_equal_the_autograd_jacobian(strategy, monkeypatch):
    key, model, batch, tokens, q, lat, got = _streamed_results(strategy, monkeypatch)
    ref_p, ref_j = jb._autograd_jacobian((key, "random"), model, batch, tokens, q)
    for chunk in CHUNKS:
        pred, jac = got[chunk]
        assert pred.shape == (q.shape[0], 1) and jac.shape == (q.shape[0], 1, 3)
        assert not pred.requires_grad and not jac.requires_grad and pred.grad_fn is None and jac.grad_fn is None
        with torch.no_grad():
            smp = model.sample(lat, q)                      # the queries in one piece
        assert torch.equal(pred, smp), (chunk, (pred - smp).abs().max().item())
        assert torch.allclose(pred, ref_p, rtol=1e-4, atol=1e-5)
        jb.check(f"sample_jacobian_rows/{strategy}/chunk{chunk}", jac, ref_j)


@pytest.mark.parametrize("strategy", list(DECODERS))
def test_chunkings_are_bit_identical(strategy, monkeypatch):
    """A row that straddles two of the kernel's 32-edge tiles is the sum of two partial sums, and where a row lies against the tiles
    depends on its offset in the launch's list.  sample_jacobian leads every chunk's list with the padding edges that put its rows
    where the list of all queries has them, so the chunkings agree bit for bit (without that: 2-7e-7 of the peak apart)."""
    key, model, batch, tokens, q, lat, got = _streamed_results(strategy, monkeypatch)
    pred, jac = got[None]
    for chunk in CHUNKS[1:]:
        dp, dj = (got[chunk][0] - pred).abs().max().item(), (got[chunk][1] - jac).abs().max().item()
        print(f"[chunking] sample_jacobian_rows/{strategy}: chunk {chunk} against one piece: max |d pred| = {dp:.3e} (peak "
              f"{pred.abs().max().item():.3e}), max |d jac| = {dj:.3e} (peak {jac.abs().max().item():.3e})")
    for chunk in CHUNKS[1:]:
        assert torch.equal(got[chunk][0], pred) and torch.equal(got[chunk][1], jac), chunk


@pytest.mark.parametrize("strategy", list(DECODERS))
def test_bf16_mode_returns_the_fp32_result(strategy, monkeypatch):
    key, model, batch, tokens, q, lat, got = _streamed_results(strategy, monkeypatch)
    with jb._precision("bf16"):
        pb, jbf = model.sample_jacobian(lat, q, chunk_points=1000, row_lists=True)
    assert torch.equal(pb, got[1000][0]) and torch.equal(jbf, got[1000][1])


SHAPES = {
    "two_scales_weighted": ("radius", 2, dict(scales=[1.0, 2.0], use_scale_weights=True)),
    "two_scales_weighted_bidirectional": ("bidirectional", 2, dict(scales=[1.0, 2.0], use_scale_weights=True)),
    "two_scales_summed": ("radius", 1, dict(scales=[1.0, 2.0], use_scale_weights=False)),
    "nonlinear": ("bidirectional", 1, dict(out_gno_transform_type="nonlinear")),
    "c16": ("radius", 1, dict(lifting_channels=16)),
}


@pytest.mark.parametrize("case", list(SHAPES))
def test_other_shapes_stream(case, monkeypatch):
    strategy, out, kw = SHAPES[case]
    key, (model, batch, tokens) = _model(strategy, out=out, **kw)
    q = jb._queries("random", batch)[:1500]
    ref_p, ref_j = jb._autograd_jacobian((key, "random"), model, batch, tokens, q)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
        smp = model.sample(lat, q)                          # the queries in one piece
    with jb._watch(monkeypatch) as seen:
        pred, jac = model.sample_jacobian(lat, q, chunk_points=700, row_lists=True)
    assert _streamed_rows(seen), seen
    assert torch.equal(pred, smp)
    assert torch.allclose(pred, ref_p, rtol=1e-4, atol=1e-5)
    jb.check(f"sample_jacobian_rows/{case}", jac, ref_j)


@pytest.mark.parametrize("strategy", list(DECODERS))
def test_without_the_flag_the_route_is_todays(strategy, monkeypatch):
    key, (model, batch, tokens) = _model(strategy)
    q = jb._queries("random", batch)[:300]
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    with jb._watch(monkeypatch) as seen:
        pred, jac = model.sample_jacobian(lat, q, chunk_points=200)
    assert not any(k.startswith("gno_fwd_jac") for k in seen["keys"]) and seen["csr"] > 0, seen
    with jb._watch(monkeypatch) as seen:
        model.sample_jacobian(lat, q, chunk_points=200, row_lists=False)
    assert not any(k.startswith("gno_fwd_jac") for k in seen["keys"]) and seen["csr"] > 0, seen
    ps, js = model.sample_jacobian(lat, q, chunk_points=200, row_lists=True)
    assert torch.allclose(ps, pred, rtol=1e-4, atol=1e-5)
    jb.check(f"sample_jacobian_rows_against_default/{strategy}", js, jac)


def test_a_knn_decoder_ignores_the_flag(monkeypatch):
    model, batch, tokens = jb._setup()
    q = jb._queries("random", batch)[:1500]
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    plain = model.sample_jacobian(lat, q, chunk_points=700)
    with jb._watch(monkeypatch) as seen:
        flagged = model.sample_jacobian(lat, q, chunk_points=700, row_lists=True)
    assert jb._streamed(seen) and not any(k.startswith("gno_fwd_jac") for k in seen["keys"]), seen
    assert torch.equal(flagged[0], plain[0]) and torch.equal(flagged[1], plain[1])


def test_in_a_capture_the_flagged_call_raises_before_any_launch():
    from gaot_3d_amd import ops
    from gaot_3d_amd._lib import GaotError
    key, (model, batch, tokens) = _model("bidirectional")
    q = batch.pos[:1000].contiguous()
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    eager = model.sample_jacobian(lat, q, row_lists=True)           # describes the grid, warms the allocator
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(GaotError, match="captured"):
        with torch.cuda.graph(g):
            model.sample_jacobian(lat, q, row_lists=True)
    assert ops.launch_count() == n0
    torch.cuda.synchronize()
    again = model.sample_jacobian(lat, q, row_lists=True)
    torch.cuda.synchronize()
    assert torch.equal(again[0], eager[0]) and torch.equal(again[1], eager[1])


# ---- memory -----------------------------------------------------------------------------------------------------------------------------
def test_only_the_results_grow_with_the_number_of_queries():
    key, (model, batch, tokens) = _model("radius")
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    rest = {}
    for nq in (200000, 800000):
        q = (torch.rand(nq, 3, generator=gen) * 2 - 1).to(DEV)
        results = 4 * nq * 1 + 4 * nq * 1 * 3                   # pred and jac, fp32
        rest[nq] = jb._rise(lambda: model.sample_jacobian(lat, q, chunk_points=jb.MEM_CHUNK, row_lists=True)) - results
    q = (torch.rand(200000, 3, generator=gen) * 2 - 1).to(DEV)
    default = jb._rise(lambda: model.sample_jacobian(lat, q, chunk_points=200000)) - (4 * 200000 * 4)       # the default route, one piece
    print(f"[memory] sample_jacobian(row_lists=True) beyond its results: {rest[200000] / 2**20:.2f} MiB at 200 K, "
          f"{rest[800000] / 2**20:.2f} MiB at 800 K; default route at 200 K in one piece: {default / 2**20:.2f} MiB")
    assert abs(rest[800000] - rest[200000]) < 4 * 2**20, rest
    assert rest[200000] < default, (rest, default)
