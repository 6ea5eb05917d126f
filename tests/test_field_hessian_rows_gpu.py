"""Second spatial derivatives of the sampled field on ROW lists: gaot_gno_fwd_jet2 (the directional 2-jet kernel of
gaot_gno_fwd_knn_jet2 on the ragged by-query list of any graph, every plane finished by segment_walk and one fix-up over all
1 + 2 nd planes), ops.gno_forward_jet2, IntegralTransform.jet2_rows and MAGNODecoder / GAOT3D.sample_hessian_rows and
sample_laplacian_rows for 'radius' and 'bidirectional' decoders.

The bar is the project's fp32 bar for coordinate derivatives (FP32_BAR: max error <= 1e-3 of the reference's peak, cosine >= 0.99999),
applied separately to d1, to d2, to the diagonal and to the off-diagonal entries of the Hessian and to the Laplacian.

  * op level, 1..4 hidden layers x the three transform types, 211 sources, six generic directions, on lists a-e of
    tests/test_field_jacobian_rows_gpu.py (a single row; empty rows first, in the middle and last; a 70-edge row with a whole tile
    inside it; a row boundary on a tile boundary; 3000 queries and more than 1024 tiles): two launches, the value torch.equal to
    ops.gno_forward / gno_nl_forward(precision=0) and to ops.gno_forward_jac's, empty rows exact zeros in all 13 planes, d1 and d2 at
    the bar against tests/gno_rows_jet2_ref.py;
  * axis directions: d1[d] torch.equal to plane d of ops.gno_forward_jac; regular lists (k in {1, 4, 32}, Nq in {7, 33}): all planes
    torch.equal to ops.gno_forward_knn_jet2; a direction's planes do not depend on its company; a zero direction gives zeros; a
    piece of list e led by padding edges gives the rows of the whole list bit for bit;
  * bad arguments raise GaotError with the launch count unchanged; zero queries launch nothing; zero edges: the fix-up alone, zeros;
  * model level (4096 points, latent 8 x 8 x 8, r = 0.45, k = 8, 'radius' and 'bidirectional'; 300 sample points and 300 random queries
    partly outside the box, so some rows are empty) against the fp64 oracle's decoder on the edges of the lists graph.query_lists
    returned, per scale, differentiated twice on the CPU, no query excluded: gno_jet2_rows* and mlp2_jet2* keys, no CSR build, no
    gno_bwd* / gno_fwd_jac* / gno_jet2_knn* key; pred and jac torch.equal to sample_jacobian(row_lists=True); hess exactly symmetric
    and at the bar; lap the ordered trace and at the bar; chunkings None / 250 / 64 bit-identical; bf16 mode the fp32 bits; four
    output channels, 'nonlinear', two scales with softmax weights (the second-order weight term), two scales summed, four hidden
    layers; queries far from every token (empty rows) give sample's prediction and exactly zero derivatives; a 'knn' model gives
    sample_hessian / sample_laplacian; refusals and the capture error without a launch."""
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
import gno_rows_jac_ref as JREF  # noqa: E402
import gno_rows_jet2_ref as REF  # noqa: E402
import test_field_hessian_gpu as hb  # noqa: E402  (the model fixture with its config, the watcher, check(), the bar, the directions)
import test_field_jacobian_rows_gpu as jr  # noqa: E402  (the lists, the graph of a list, the device operands, the decoders)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = hb.MODES
NSRC = jr.NSRC
FP32_BAR = hb.FP32_BAR
GENERIC, AXES = hb.GENERIC, hb.AXES
DEGREES = jr.DEGREES
ZERO = (0.0, 0.0, 0.0)


# ---- op level ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nh", [1, 2, 3, 4])
def test_value_is_the_forward_and_the_jets_meet_the_bar(nh, mode):
    from gaot_3d_amd import ops
    gen, y, f, ws, bs, yd, wd, bd, fk, t = jr._device_operands(nh, mode)
    for name, deg in DEGREES.items():
        nq = len(deg)
        x = torch.rand(nq, 3, generator=gen) * 2 - 1
        src, dst, rowptr = JREF.ragged_list(deg, NSRC, gen)
        g = jr._graph(src, dst, rowptr, NSRC)
        xd = x.to(DEV)
        n0 = ops.launch_count()
        out, d1, d2 = ops.gno_forward_jet2(mode, wd, bd, yd, xd, fk, t, g, GENERIC)
        assert ops.launch_count() == n0 + 2, name                                            # the jet kernel and the fix-up
        assert out.shape == (nq, 32) and d1.shape == d2.shape == (6, nq, 32) and d1.is_contiguous() and d2.is_contiguous()
        val = jr._forward(mode, wd, bd, yd, xd, fk, t, g)
        assert torch.equal(out, val), (name, (out - val).abs().max().item())
        jo, jac = ops.gno_forward_jac(mode, wd, bd, yd, xd, fk, t, g)
        assert torch.equal(out, jo), name
        empty = (torch.tensor(deg) == 0).to(DEV)
        for plane in (out[empty], d1[:, empty], d2[:, empty]):
            assert torch.equal(plane, torch.zeros_like(plane)), name
        ro, r1, r2 = REF.gno_rows_jet2(ws, bs, y, x, src, dst, rowptr, f, mode, GENERIC)
        assert torch.allclose(out.cpu().double(), ro, rtol=1e-4, atol=1e-5), name
        hb.check(f"gno_jet2_rows/{mode}/nh{nh}/list_{name}/d1", d1, r1)
        hb.check(f"gno_jet2_rows/{mode}/nh{nh}/list_{name}/d2", d2, r2)
        # axis directions: the tangent planes of the Jacobian kernel on the same list, bit for bit
        oa, a1, a2 = ops.gno_forward_jet2(mode, wd, bd, yd, xd, fk, t, g, AXES)
        assert torch.equal(oa, val), name
        for d in range(3):
            assert torch.equal(a1[d], jac[d]), (name, d, (a1[d] - jac[d]).abs().max().item())


@pytest.mark.parametrize("mode", MODES)
def test_regular_lists_equal_the_knn_kernel(mode):
    from gaot_3d_amd import ops
    for nh in (1, 2, 3, 4):
        gen, y, f, ws, bs, yd, wd, bd, fk, t = jr._device_operands(nh, mode)
        for nq in (7, 33):
            xd = (torch.rand(nq, 3, generator=gen) * 2 - 1).to(DEV)
            for k in (1, 4, 32):
                src, dst, rowptr = JREF.ragged_list([k] * nq, NSRC, gen)
                got = ops.gno_forward_jet2(mode, wd, bd, yd, xd, fk, t, jr._graph(src, dst, rowptr, NSRC), GENERIC)
                knn = ops.gno_forward_knn_jet2(mode, wd, bd, yd, xd, fk, t, src.to(DEV), k, GENERIC)
                for a, b in zip(got, knn):
                    assert torch.equal(a, b), (nh, nq, k, (a - b).abs().max().item())


@pytest.mark.parametrize("mode", MODES)
def test_a_directions_planes_do_not_depend_on_its_company(mode):
    """alone, first of six, last of six; a zero direction gives exact zeros; on list c (a row through three tiles) and list b"""
    from gaot_3d_amd import ops
    gen, y, f, ws, bs, yd, wd, bd, fk, t = jr._device_operands(3, mode)
    for name in ("b", "c"):
        deg = DEGREES[name]
        xd = (torch.rand(len(deg), 3, generator=gen) * 2 - 1).to(DEV)
        src, dst, rowptr = JREF.ragged_list(deg, NSRC, gen)
        g = jr._graph(src, dst, rowptr, NSRC)
        v = GENERIC[4]
        _, s1, s2 = ops.gno_forward_jet2(mode, wd, bd, yd, xd, fk, t, g, (v,))
        _, f1, f2 = ops.gno_forward_jet2(mode, wd, bd, yd, xd, fk, t, g, (v, AXES[0], ZERO, *GENERIC[:3]))
        _, l1, l2 = ops.gno_forward_jet2(mode, wd, bd, yd, xd, fk, t, g, (*GENERIC[:3], ZERO, AXES[2], v))
        assert torch.equal(s1[0], f1[0]) and torch.equal(s2[0], f2[0]), name
        assert torch.equal(s1[0], l1[5]) and torch.equal(s2[0], l2[5]), name
        assert s2[0].abs().max() > 0
        for z in (f1[2], f2[2], l1[3], l2[3]):
            assert torch.equal(z, torch.zeros_like(z)), name


@pytest.mark.parametrize("mode", MODES)
def test_a_piece_led_by_padding_edges_equals_its_rows_in_the_whole_list(mode):
    """rows [a, b) of list e, cut out and led by (edges before row a) mod 32 padding edges: all 13 planes of those rows are the whole
    list's, bit for bit -- what makes sample_hessian_rows independent of its chunks"""
    from gaot_3d_amd import ops
    gen, y, f, ws, bs, yd, wd, bd, fk, t = jr._device_operands(2, mode)
    deg = DEGREES["e"]
    nq = len(deg)
    xd = (torch.rand(nq, 3, generator=gen) * 2 - 1).to(DEV)
    src, dst, rowptr = JREF.ragged_list(deg, NSRC, gen)
    out, d1, d2 = ops.gno_forward_jet2(mode, wd, bd, yd, xd, fk, t, jr._graph(src, dst, rowptr, NSRC), GENERIC)
    for a, b in ((0, 1000), (1000, 1064), (1064, 3000), (2990, 3000)):
        e0, e1 = int(rowptr[a]), int(rowptr[b])
        lead = e0 % 32
        psrc = torch.cat([torch.zeros(lead, dtype=torch.int32), src[e0:e1]])
        pdst = torch.cat([torch.full((lead,), -1, dtype=torch.int32), dst[e0:e1] - a])
        prow = rowptr[a:b + 1] - e0 + lead
        po, p1, p2 = ops.gno_forward_jet2(mode, wd, bd, yd, xd[a:b].contiguous(), fk, t, jr._graph(psrc, pdst, prow, NSRC), GENERIC)
        assert torch.equal(po, out[a:b]) and torch.equal(p1, d1[:, a:b]) and torch.equal(p2, d2[:, a:b]), (a, b)


def test_bad_arguments_raise_before_any_launch():
    from gaot_3d_amd import _lib, ops
    from gaot_3d_amd._lib import GaotError
    lib = _lib.load()
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(2, "linear")
    deg = DEGREES["b"]
    nq = len(deg)
    src, dst, rowptr = JREF.ragged_list(deg, NSRC, gen)
    g = jr._graph(src, dst, rowptr, NSRC)
    e = g.by_dst.num_edges
    xd = (torch.rand(nq, 3, generator=gen) * 2 - 1).to(DEV)
    dirs_dev = torch.tensor(AXES, device=DEV)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    w128, b128 = hb._mlp(2, "linear", gen, hidden=128)
    with pytest.raises(GaotError, match="gaot_gno_fwd_jet2: unsupported MLP shape"):
        ops.gno_forward_jet2("linear", [w.to(DEV) for w in w128], [b.to(DEV) for b in b128], yd, xd, fd, None, g, AXES)
    with pytest.raises(GaotError, match="mode must be"):
        ops.gno_forward_jet2("cubic", wd, bd, yd, xd, fd, None, g, AXES)
    with pytest.raises(GaotError, match="rows, the graph"):                                  # mismatched graph sizes
        ops.gno_forward_jet2("linear", wd, bd, yd, xd[:-1], fd, None, g, AXES)
    with pytest.raises(GaotError, match="rows, the graph"):
        ops.gno_forward_jet2("linear", wd, bd, yd[:-1], xd, fd[:-1], None, g, AXES)
    with pytest.raises(GaotError, match="gaot_gno_fwd_jet2: nd must be"):
        ops.gno_forward_jet2("linear", wd, bd, yd, xd, fd, None, g, ())
    with pytest.raises(GaotError, match="gaot_gno_fwd_jet2: nd must be"):
        ops.gno_forward_jet2("linear", wd, bd, yd, xd, fd, None, g, (*GENERIC, AXES[0]))
    with pytest.raises(GaotError, match="host"):
        ops.gno_forward_jet2("linear", wd, bd, yd, xd, fd, None, g, dirs_dev)
    assert ops.launch_count() == n0
    m, keep = ops._mlp_struct(wd, bd)
    nd = 3
    out = torch.empty(nq, 32, device=DEV)
    d1 = torch.empty(nd, nq, 32, device=DEV)
    d2 = torch.empty(nd, nq, 32, device=DEV)
    need = lib.gaot_gno_fwd_jet2_workspace_bytes(e, nd)
    assert need == 256 * (1 + 2 * nd) * ((e + 31) // 32)
    ws_ = torch.empty(need, dtype=torch.uint8, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)
    by = g.by_dst
    host_dirs = (C.c_float * 9)(*[c for v in AXES for c in v])

    def call(mode=0, yp=ptr(yd), xp=ptr(xd), fp=ptr(fd), tab=null, s=ptr(by.other), d=ptr(by.key), rp=ptr(by.rowptr), ne=e, q=nq,
             dv=host_dirs, n=nd, o=ptr(out), p1=ptr(d1), p2=ptr(d2), w=ptr(ws_), wb=need):
        _lib.check(lib.gaot_gno_fwd_jet2(C.byref(m), mode, yp, xp, fp, tab, s, d, rp, ne, q, dv, n, o, p1, p2, w, wb, null),
                   "gaot_gno_fwd_jet2")

    for kw, msg in ((dict(mode=3), "mode must be"), (dict(n=0), "nd must be"), (dict(n=7), "nd must be"), (dict(dv=null), "null dirs"),
                    (dict(dv=ptr(dirs_dev)), "host pointer"), (dict(p1=null), "null pointer"), (dict(p2=null), "null pointer"),
                    (dict(o=null), "null pointer"), (dict(fp=null), "null pointer"), (dict(s=null), "null pointer"),
                    (dict(d=null), "null pointer"), (dict(rp=null), "null pointer"), (dict(yp=null), "null pointer"),
                    (dict(xp=null), "null pointer"), (dict(mode=1), "null src_table"), (dict(w=null), "null workspace"),
                    (dict(wb=need - 1), "workspace too small"), (dict(wb=lib.gaot_gno_fwd_jet2_workspace_bytes(e, 2)), "workspace too small"),
                    (dict(ne=-1), "negative size"), (dict(q=-1), "negative size"), (dict(ne=1 << 31), "beyond int32")):
        with pytest.raises(GaotError, match="gaot_gno_fwd_jet2: .*" + msg):
            call(**kw)
        assert ops.launch_count() == n0, kw
    call(q=0)                                                                                # zero queries: no launch
    assert ops.launch_count() == n0
    for t_ in (out, d1, d2):
        t_.fill_(1.0)
    zero_rows = torch.zeros(nq + 1, dtype=torch.int32, device=DEV)
    call(ne=0, rp=ptr(zero_rows), s=null, d=null, w=null, wb=0, fp=null, yp=null, xp=null)   # zero edges: the fix-up alone, zeros
    assert ops.launch_count() == n0 + 1
    assert not out.any() and not d1.any() and not d2.any()
    call()                                                                                   # and a good call: TWO launches
    assert ops.launch_count() == n0 + 3
    good = ops.gno_forward_jet2("linear", wd, bd, yd, xd, fd, None, g, torch.tensor(AXES))   # directions as a CPU tensor
    assert torch.equal(out, good[0]) and torch.equal(d1, good[1]) and torch.equal(d2, good[2])


# ---- model level ------------------------------------------------------------------------------------------------------------------------
DECODERS = jr.DECODERS
CHUNKS = (None, 250, 64)


def _model(strategy, out=1, k=8, **more):
    key = f"hess_rows/{strategy}/out{out}/k{k}/" + ",".join(f"{a}={b}" for a, b in sorted(more.items()))
    return key, hb._setup(key, k=k, out=out, **DECODERS[strategy], **more)


def _streamed_rows(seen):
    keys = seen["keys"]
    return (any(k.startswith("gno_jet2_rows") for k in keys) and any(k.startswith("mlp2_jet2") for k in keys) and seen["csr"] == 0
            and not any(k.startswith("csr_build") or k.startswith("gno_bwd") or k.startswith("gno_fwd_jac") or k.startswith("gno_jet2_knn")
                        for k in keys))


_REFS = {}


def _oracle_hessian(key, model, cfg, lat, q):
    """(pred [Nq, out], jac [Nq, out, 3], hess [Nq, out, 3, 3], empty rows of scale 0) of the fp64 oracle's decoder on the CPU, the
    edges of every scale built from the list graph.query_lists returned for these queries, differentiated twice; once per key"""
    if key in _REFS:
        return _REFS[key]
    from gaot_3d_amd import graph as device_graph
    dec = model.decoder
    tok = model._tokens(1, q.device, None, None)[0]
    with torch.no_grad():
        grid = dec._stream_grid(lat, q, tok)
    assert grid is not None
    edges, empty = {}, None
    for si, scale in enumerate(cfg.magno.scales):
        rows = device_graph.query_lists(dec.decoder_strategy, q, grid, dec.gno_radius * scale, int(dec.k_neighbors))
        edges[f"decoder_edge_index_s{si}"] = torch.stack([rows.by_dst.other.long(), rows.by_dst.key.long()]).cpu()
        if si == 0:
            rp = rows.by_dst.rowptr.cpu()
            empty = rp[1:] == rp[:-1]
    sd = {n: v.detach().double().cpu() for n, v in model.state_dict().items()}
    xg = q.detach().double().cpu().requires_grad_(True)
    p = orc.magno_decoder(sd, cfg.magno, lat.detach().double().cpu(), xg, tok.double().cpu(), types.SimpleNamespace(**edges))
    oc = p.shape[1]
    jac, hess = torch.zeros(q.shape[0], oc, 3, dtype=torch.float64), torch.zeros(q.shape[0], oc, 3, 3, dtype=torch.float64)
    for o in range(oc):
        (g,) = torch.autograd.grad(p[:, o].sum(), xg, create_graph=True)
        jac[:, o] = g.detach()
        for i in range(3):
            (gg,) = torch.autograd.grad(g[:, i].sum(), xg, retain_graph=True)
            hess[:, o, i] = gg
    _REFS[key] = (p.detach(), jac, hess, empty)
    return _REFS[key]


_GOT = {}


def _streamed_results(strategy, monkeypatch):
    """sample_hessian_rows and sample_laplacian_rows of the 600 queries at every chunking, with the keys they ran: once per strategy"""
    if strategy not in _GOT:
        key, (model, batch, tokens, cfg) = _model(strategy)
        q = hb._queries(batch)
        with torch.no_grad():
            lat = model.latent(batch, tokens)
        got = {}
        for chunk in CHUNKS:
            with hb._watch(monkeypatch) as seen:
                h = model.sample_hessian_rows(lat, q, chunk_points=chunk)
                l = model.sample_laplacian_rows(lat, q, chunk_points=chunk)
            assert _streamed_rows(seen), seen
            got[chunk] = (h, l)
        _GOT[strategy] = (key, model, cfg, q, lat, got)
    return _GOT[strategy]


def _check_results(name, model, lat, q, h, l, ref, chunk=None):
    ref_p, ref_j, ref_h, _ = ref
    pred, jac, hess = h
    pl, lap = l
    nq, oc = q.shape[0], ref_p.shape[1]
    assert pred.shape == (nq, oc) and jac.shape == (nq, oc, 3) and hess.shape == (nq, oc, 3, 3) and lap.shape == (nq, oc)
    for t in (pred, jac, hess, pl, lap):
        assert not t.requires_grad and t.grad_fn is None
    pj, jj = model.sample_jacobian(lat, q, chunk_points=chunk, row_lists=True)
    assert torch.equal(pred, pj) and torch.equal(jac, jj) and torch.equal(pl, pj), name
    assert torch.allclose(pred.cpu().double(), ref_p, rtol=1e-4, atol=1e-5), name
    hb.check(f"{name}/jac", jac, ref_j)
    hb._check_hessian(name, hess, ref_h)
    for i in range(3):
        for j in range(i):
            assert torch.equal(hess[..., i, j], hess[..., j, i]), (name, i, j)
    assert torch.equal(lap, hess[..., 0, 0] + hess[..., 1, 1] + hess[..., 2, 2]), name
    hb.check(f"{name}/lap", lap, ref_h[..., 0, 0] + ref_h[..., 1, 1] + ref_h[..., 2, 2])


@pytest.mark.parametrize("strategy", list(DECODERS))
def test_row_lists_stream_and_meet_the_oracle(strategy, monkeypatch):
    key, model, cfg, q, lat, got = _streamed_results(strategy, monkeypatch)
    ref = _oracle_hessian(key, model, cfg, lat, q)
    print(f"[rows] sample_hessian_rows/{strategy}: {int(ref[3].sum())} of {q.shape[0]} queries have an empty row at scale 0 (none is excluded)")
    _check_results(f"sample_hessian_rows/{strategy}", model, lat, q, *got[None], ref)


@pytest.mark.parametrize("strategy", list(DECODERS))
def test_chunkings_are_bit_identical(strategy, monkeypatch):
    key, model, cfg, q, lat, got = _streamed_results(strategy, monkeypatch)
    (pred, jac, hess), (pl, lap) = got[None]
    for chunk in CHUNKS[1:]:
        (cp, cj, ch), (cpl, cl) = got[chunk]
        print(f"[chunking] sample_hessian_rows/{strategy}: chunk {chunk} against one piece: max |d hess| = "
              f"{(ch - hess).abs().max().item():.3e} (peak {hess.abs().max().item():.3e}), max |d lap| = {(cl - lap).abs().max().item():.3e}")
    for chunk in CHUNKS[1:]:
        (cp, cj, ch), (cpl, cl) = got[chunk]
        assert torch.equal(cp, pred) and torch.equal(cj, jac) and torch.equal(ch, hess), chunk
        assert torch.equal(cpl, pl) and torch.equal(cl, lap), chunk


@pytest.mark.parametrize("strategy", list(DECODERS))
def test_bf16_mode_returns_the_fp32_result(strategy, monkeypatch):
    key, model, cfg, q, lat, got = _streamed_results(strategy, monkeypatch)
    with hb._precision("bf16"):
        hbf = model.sample_hessian_rows(lat, q, chunk_points=250)
        lbf = model.sample_laplacian_rows(lat, q, chunk_points=250)
    assert all(torch.equal(a, b) for a, b in zip(hbf, got[250][0])) and all(torch.equal(a, b) for a, b in zip(lbf, got[250][1]))


SHAPES = {
    "four_channels": ("radius", 4, {}),
    "nonlinear": ("bidirectional", 1, dict(out_gno_transform_type="nonlinear")),
    "two_scales_weighted": ("radius", 2, dict(scales=[1.0, 2.0], use_scale_weights=True)),
    "two_scales_weighted_bidirectional": ("bidirectional", 1, dict(scales=[1.0, 2.0], use_scale_weights=True)),
    "two_scales_summed": ("radius", 1, dict(scales=[1.0, 2.0], use_scale_weights=False)),
    "four_layers": ("bidirectional", 1, dict(out_gno_channel_mlp_hidden_layers=[64, 64, 64, 64])),
}


@pytest.mark.parametrize("case", list(SHAPES))
def test_other_shapes_stream(case, monkeypatch):
    strategy, out, kw = SHAPES[case]
    key, (model, batch, tokens, cfg) = _model(strategy, out=out, **kw)
    q = hb._queries(batch, 150, 150)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    ref = _oracle_hessian(key, model, cfg, lat, q)
    with hb._watch(monkeypatch) as seen:
        h = model.sample_hessian_rows(lat, q, chunk_points=128)
        l = model.sample_laplacian_rows(lat, q, chunk_points=128)
    assert _streamed_rows(seen), seen
    _check_results(f"sample_hessian_rows/{case}", model, lat, q, h, l, ref, chunk=128)


def test_queries_far_from_every_token_have_empty_rows_and_zero_derivatives():
    """the 600 queries above all find tokens within r = 0.45 (the farthest corner of [-1.2, 1.2]^3 is 0.35 from its token); queries at a
    distance have EMPTY rows on a 'radius' decoder: the prediction is the projection of zero rows, sample's bit for bit, and every
    derivative is exactly zero -- among queries that do have rows, in one chunk and cut apart"""
    from gaot_3d_amd import graph as device_graph
    key, (model, batch, tokens, cfg) = _model("radius")
    far = torch.tensor([[3.0, 0.1, -0.2], [-2.5, 2.5, 0.0], [0.3, 0.2, 4.0]], device=DEV)
    q = torch.cat([far[:1], batch.pos[:40], far[1:2], batch.pos[40:70], far[2:]]).contiguous()
    idx = torch.tensor([0, 41, 72], device=DEV)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
        smp = model.sample(lat, q)
    tok = model._tokens(1, q.device, None, None)[0]
    rp = device_graph.query_lists("radius", q, model.decoder._stream_grid(lat, q, tok), model.decoder.gno_radius, 8).by_dst.rowptr
    deg = rp[1:] - rp[:-1]
    assert not deg[idx].any() and int((deg == 0).sum()) == 3
    for chunk in (None, 41):
        pred, jac, hess = model.sample_hessian_rows(lat, q, chunk_points=chunk)
        pl, lap = model.sample_laplacian_rows(lat, q, chunk_points=chunk)
        assert torch.equal(pred, smp) and torch.equal(pl, smp)
        for t in (jac[idx], hess[idx], lap[idx]):
            assert torch.equal(t, torch.zeros_like(t)), chunk
        assert hess.abs().amax(dim=(1, 2, 3)).gt(0).sum() == q.shape[0] - 3


def test_on_a_knn_decoder_the_calls_are_the_knn_calls(monkeypatch):
    model, batch, tokens, cfg = hb._setup()
    q = hb._queries(batch)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    plain_h, plain_l = model.sample_hessian(lat, q, chunk_points=250), model.sample_laplacian(lat, q, chunk_points=250)
    with hb._watch(monkeypatch) as seen:
        rows_h, rows_l = model.sample_hessian_rows(lat, q, chunk_points=250), model.sample_laplacian_rows(lat, q, chunk_points=250)
    assert hb._streamed(seen) and not any(k.startswith("gno_jet2_rows") for k in seen["keys"]), seen
    assert all(torch.equal(a, b) for a, b in zip(rows_h, plain_h)) and all(torch.equal(a, b) for a, b in zip(rows_l, plain_l))


REFUSALS = {
    "use_attn": ("radius", 8, dict(use_attn=True), "use_attn"),
    "geoembed": ("bidirectional", 8, dict(use_geoembed=[True, True], embedding_method="pointnet"), "GeoEmbed"),
    "projection96": ("radius", 8, dict(projection_channels=96), "projection"),
    "bidirectional_k64": ("bidirectional", 64, {}, "k_neighbors = 64"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_other_configurations_are_refused(case):
    from gaot_3d_amd import ops
    strategy, k, kw, msg = REFUSALS[case]
    key, (model, batch, tokens, cfg) = _model(strategy, k=k, **kw)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    torch.cuda.synchronize()
    for method in (model.sample_hessian_rows, model.sample_laplacian_rows):
        n0 = ops.launch_count()
        with pytest.raises(NotImplementedError, match="second derivatives on row lists.*" + msg):
            method(lat, batch.pos[:200])
        assert ops.launch_count() == n0


def test_reverse_and_chunk_points_raise_value_errors():
    key, (model, batch, tokens, cfg) = _model("radius")
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    for method in (model.sample_hessian_rows, model.sample_laplacian_rows):
        with pytest.raises(ValueError, match="chunk_points"):
            method(lat, batch.pos[:100], chunk_points=0)
        model.decoder.decoder_strategy = "reverse"
        try:
            with pytest.raises(ValueError, match="reverse"):
                method(lat, batch.pos[:100])
        finally:
            model.decoder.decoder_strategy = "radius"


def test_in_a_capture_the_calls_raise_before_any_launch():
    from gaot_3d_amd import ops
    from gaot_3d_amd._lib import GaotError
    key, (model, batch, tokens, cfg) = _model("bidirectional")
    q = batch.pos[:300].contiguous()
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    eager = model.sample_hessian_rows(lat, q)                       # describes the grid, warms the allocator
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(GaotError, match="captured"):
        with torch.cuda.graph(g):
            model.sample_hessian_rows(lat, q)
    assert ops.launch_count() == n0
    torch.cuda.synchronize()
    again = model.sample_hessian_rows(lat, q)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(again, eager))
