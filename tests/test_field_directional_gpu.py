"""Directional derivatives of the sampled field along PER-QUERY directions: gaot_gno_fwd_knn_jet2_qd / gaot_gno_fwd_jet2_qd (the jet
kernels with the direction of a pass loaded per lane from a device array [Nq][nd][3]), ops.gno_forward_knn_jet2_qd /
gno_forward_jet2_qd, IntegralTransform.jet2_knn_qd / jet2_rows_qd and MAGNODecoder / GAOT3D.sample_directional on 'knn', 'radius' and
'bidirectional' decoders.

The bar is the project's fp32 bar for coordinate derivatives (tests/test_coord_grad_gpu.py FP32_BAR, as tests/test_field_hessian_gpu.py
uses it: max error <= 1e-3 of the reference's peak, cosine >= 0.99999), applied separately to d1 and to d2, each peak asserted > 0.
Contracts (C1 .. C7 of the kernels' header comment and of sample_directional's docstring):

  * op level, regular lists: Nq in {1, 7, 33, 1000} x k in {1 .. 32} x 1..4 hidden layers x the three transform types, 211 sources
    with repeats, nd rotated over {1, 3, 6}, random per-query directions (neither axis-aligned nor unit): one launch; the value
    torch.equal to ops.gno_forward_knn(precision=0) (C1); d1 / d2 at the bar against tests/gno_qdir_jet2_ref.py; the same directions
    for every query: all planes torch.equal to ops.gno_forward_knn_jet2 (C2); five direction sets handed out by q mod 5: every
    residue class's rows torch.equal to the host-direction call with its set (C3); a slot's planes alone, first of six, last of six,
    and a zero direction gives exact zeros (C4);
  * op level, row lists a-e of tests/test_field_jacobian_rows_gpu.py: two launches, C1 against ops.gno_forward / gno_nl_forward, empty
    rows exact zeros in all planes, the bar, C2, C3; regular lists equal the regular-list kernel and a piece led by padding edges
    gives the whole list's rows (C5); zero edges: the fix-up alone and zeros; zero queries: no launch; bad arguments raise with the
    launch count unchanged;
  * model level (4096 points, latent 8 x 8 x 8, k = 8, 'knn' / 'radius' / 'bidirectional' with r = 0.45; 300 sample points and 300
    random queries partly outside the box) against the fp64 oracle's decoder on the edges of the lists actually used, differentiated
    twice on the CPU and contracted (J v, v^T H v), no query excluded; orthonormal frames: d2.sum(-1) against sample_laplacian(_rows);
    chunkings None / 250 / 64 and bf16 mode bit-identical (C6); the axes: pred / d1 torch.equal to sample_jacobian's and d2 to the
    diagonal of sample_hessian(_rows)'s, softmax scale weights INCLUDED (C7); four channels, 'nonlinear', two scales weighted and
    summed, four hidden layers; far queries on a row route; only ..._qd GNO keys and mlp2_jet2*; graph replay on 'knn' with the
    coordinates and the directions overwritten in place, the capture error on a row route; every refusal."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gno_qdir_jet2_ref as REF  # noqa: E402
import gno_rows_jac_ref as JREF  # noqa: E402
import test_field_hessian_gpu as hb  # noqa: E402  (the model fixture, the watcher, check(), the bar, the knn oracle)
import test_field_hessian_rows_gpu as hr  # noqa: E402  (the row-list models and their oracle)
import test_field_jacobian_rows_gpu as jr  # noqa: E402  (the lists, the graph of a list, the device operands)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES, KS, NQS, NSRC = hb.MODES, hb.KS, hb.NQS, hb.NSRC
FP32_BAR = hb.FP32_BAR
GENERIC, AXES = hb.GENERIC, hb.AXES
DEGREES = jr.DEGREES


def _rand_dirs(nq, nd, gen):
    return torch.randn(nq, nd, 3, generator=gen) * 1.4          # neither axis-aligned nor of unit length


def _uniform(dirs, nq):
    return torch.tensor(dirs)[None].expand(nq, len(dirs), 3).contiguous().to(DEV)


def _sets_by_residue(nq, nd, gen):
    """five direction sets handed out by q mod 5 -> (the sets [5, nd, 3], the per-query tensor on the device)"""
    sets = _rand_dirs(5, nd, gen)
    return sets, sets[torch.arange(nq) % 5].contiguous().to(DEV)


def _check_residues(name, got, sets, host_call, nq):
    """C3: the rows of every residue class are the host-direction call's with that class's directions"""
    for r in range(min(5, nq)):
        want = host_call(sets[r].tolist())
        for a, b in zip(got, want):
            assert torch.equal(a[..., r::5, :], b[..., r::5, :]), (name, r, (a - b)[..., r::5, :].abs().max().item())


def _check_slots(name, call, qd):
    """C4: slot 0's planes alone, first of six and last of six; a zero direction gives exact zeros"""
    nq = qd.shape[0]
    v = qd[:, :1]
    zero = torch.zeros(nq, 1, 3, device=DEV)
    other = torch.tensor(GENERIC[:4], device=DEV)[None].expand(nq, 4, 3)
    _, s1, s2 = call(v.contiguous())
    _, f1, f2 = call(torch.cat([v, zero, other], dim=1))
    _, l1, l2 = call(torch.cat([other.flip(1), zero, v], dim=1))
    assert torch.equal(s1[0], f1[0]) and torch.equal(s2[0], f2[0]), name
    assert torch.equal(s1[0], l1[5]) and torch.equal(s2[0], l2[5]), name
    assert torch.equal(f1[2], l1[3]) and torch.equal(f2[2], l2[3]), name      # the same direction in another slot, in other company
    for z in (f1[1], f2[1], l1[4], l2[4]):
        assert torch.equal(z, torch.zeros_like(z)), name


# ---- op level, regular lists ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nh", [1, 2, 3, 4])
def test_regular_lists(nh, mode):
    from gaot_3d_amd import ops
    gen, y, f, ws, bs, yd, wd, bd, fk, t = jr._device_operands(nh, mode)
    worst = {"d1": [0.0, 1.0], "d2": [0.0, 1.0]}
    for qi, nq in enumerate(NQS):
        x = torch.rand(nq, 3, generator=gen) * 2 - 1
        xd = x.to(DEV)
        for ki, k in enumerate(KS):
            nd = (1, 3, 6)[(ki + qi) % 3]                # rotated with Nq: every k meets every nd
            name = f"gno_jet2_knn_qd/{mode}/nh{nh}/nq{nq}/k{k}/nd{nd}"
            nbr = torch.randint(0, NSRC, (nq * k,), generator=gen, dtype=torch.int32)        # repeats allowed
            nb = nbr.to(DEV)
            call = lambda qd: ops.gno_forward_knn_jet2_qd(mode, wd, bd, yd, xd, fk, t, nb, k, qd)
            host = lambda dirs: ops.gno_forward_knn_jet2(mode, wd, bd, yd, xd, fk, t, nb, k, dirs)
            qdirs = _rand_dirs(nq, nd, gen)
            qd = qdirs.to(DEV)
            n0 = ops.launch_count()
            out, d1, d2 = call(qd)
            assert ops.launch_count() == n0 + 1, name                                        # ONE launch
            assert out.shape == (nq, 32) and d1.shape == d2.shape == (nd, nq, 32) and d1.is_contiguous() and d2.is_contiguous()
            val = ops.gno_forward_knn(mode, wd, bd, yd, xd, fk, t, nb, k, precision=0)
            assert torch.equal(out, val), (name, (out - val).abs().max().item())             # C1
            ro, r1, r2 = REF.gno_knn_jet2_qd(ws, bs, y, x, nbr, k, f, mode, qdirs)
            assert torch.allclose(out.cpu().double(), ro, rtol=1e-4, atol=1e-5), name
            for pl, got, ref in (("d1", d1, r1), ("d2", d2, r2)):
                rel, cos = hb.check(f"{name}/{pl}", got, ref, quiet=True)
                worst[pl] = [max(worst[pl][0], rel), min(worst[pl][1], cos)]
            for a, b in zip(call(_uniform(GENERIC[:nd], nq)), host(GENERIC[:nd])):           # C2
                assert torch.equal(a, b), (name, (a - b).abs().max().item())
            sets, by_res = _sets_by_residue(nq, nd, gen)
            _check_residues(name, call(by_res), sets, host, nq)                              # C3
            _check_slots(name, call, qd)                                                     # C4
    for pl in ("d1", "d2"):
        print(f"[parity] gno_jet2_knn_qd/{mode}/nh{nh}/{pl}: worst rel_to_peak={worst[pl][0]:.3e} worst cosine={worst[pl][1]:.7f} over "
              f"{len(NQS) * len(KS)} shapes (bar {FP32_BAR[0]:.0e} / {FP32_BAR[1]})")


def test_regular_lists_bad_arguments_raise_before_any_launch():
    from gaot_3d_amd import ops
    from gaot_3d_amd._lib import GaotError
    gen, y, f, ws, bs, yd, wd, bd, fd, _ = jr._device_operands(2, "linear")
    nq = 40
    xd = (torch.rand(nq, 3, generator=gen) * 2 - 1).to(DEV)
    nbr = torch.zeros(nq * 8, dtype=torch.int32, device=DEV)
    qd = _rand_dirs(nq, 3, gen).to(DEV)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    call = lambda dirs, nb=nbr, k=8, x=xd: ops.gno_forward_knn_jet2_qd("linear", wd, bd, yd, x, fd, None, nb, k, dirs)
    for dirs, msg in ((qd[:, :0], "gaot_gno_fwd_knn_jet2_qd: nd must be"), (torch.cat([qd, qd, qd[:, :1]], 1), "gaot_gno_fwd_knn_jet2_qd: nd must be"),
                      (qd[:-1], "qdirs must be"), (qd[:, :, :2], "qdirs must be"), (qd[:, 0], "qdirs must be"), (qd.cpu(), "float32 tensor on"),
                      (qd.double(), "float32 tensor on"), (AXES, "float32 tensor on")):
        with pytest.raises(GaotError, match=msg):
            call(dirs)
        assert ops.launch_count() == n0, msg
    with pytest.raises(GaotError, match="gaot_gno_fwd_knn_jet2_qd: k must be"):
        call(qd, torch.zeros(nq * 3, dtype=torch.int32, device=DEV), 3)
    with pytest.raises(GaotError, match="nbr must hold"):
        call(qd, nbr[:-1])
    with pytest.raises(GaotError, match="mode must be"):
        ops.gno_forward_knn_jet2_qd("cubic", wd, bd, yd, xd, fd, None, nbr, 8, qd)
    assert ops.launch_count() == n0
    none = ops.gno_forward_knn_jet2_qd("linear", wd, bd, yd, xd[:0], fd, None, nbr[:0], 8, qd[:0])      # zero queries: no launch
    assert ops.launch_count() == n0 and none[0].shape == (0, 32) and none[1].shape == none[2].shape == (3, 0, 32)
    strided = torch.cat([qd, qd], dim=2)[:, :, :3]                                           # made contiguous when needed
    assert not strided.is_contiguous()
    a, b = call(strided), call(qd)
    assert ops.launch_count() == n0 + 2 and all(torch.equal(p, r) for p, r in zip(a, b))


# ---- op level, row lists ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nh", [1, 2, 3, 4])
def test_row_lists(nh, mode):
    from gaot_3d_amd import ops
    gen, y, f, ws, bs, yd, wd, bd, fk, t = jr._device_operands(nh, mode)
    for li, (lname, deg) in enumerate(DEGREES.items()):
        nq, nd = len(deg), (1, 3, 6)[(li + nh) % 3]
        name = f"gno_jet2_rows_qd/{mode}/nh{nh}/list_{lname}/nd{nd}"
        x = torch.rand(nq, 3, generator=gen) * 2 - 1
        src, dst, rowptr = JREF.ragged_list(deg, NSRC, gen)
        g = jr._graph(src, dst, rowptr, NSRC)
        xd = x.to(DEV)
        call = lambda qd: ops.gno_forward_jet2_qd(mode, wd, bd, yd, xd, fk, t, g, qd)
        host = lambda dirs: ops.gno_forward_jet2(mode, wd, bd, yd, xd, fk, t, g, dirs)
        qdirs = _rand_dirs(nq, nd, gen)
        n0 = ops.launch_count()
        out, d1, d2 = call(qdirs.to(DEV))
        assert ops.launch_count() == n0 + 2, name                                            # the jet kernel and the fix-up
        assert out.shape == (nq, 32) and d1.shape == d2.shape == (nd, nq, 32) and d1.is_contiguous() and d2.is_contiguous()
        val = jr._forward(mode, wd, bd, yd, xd, fk, t, g)
        assert torch.equal(out, val), (name, (out - val).abs().max().item())                 # C1
        empty = (torch.tensor(deg) == 0).to(DEV)
        for plane in (out[empty], d1[:, empty], d2[:, empty]):
            assert torch.equal(plane, torch.zeros_like(plane)), name
        ro, r1, r2 = REF.gno_rows_jet2_qd(ws, bs, y, x, src, dst, rowptr, f, mode, qdirs)
        assert torch.allclose(out.cpu().double(), ro, rtol=1e-4, atol=1e-5), name
        hb.check(f"{name}/d1", d1, r1)
        hb.check(f"{name}/d2", d2, r2)
        for a, b in zip(call(_uniform(GENERIC[:nd], nq)), host(GENERIC[:nd])):               # C2
            assert torch.equal(a, b), (name, (a - b).abs().max().item())
        sets, by_res = _sets_by_residue(nq, nd, gen)
        _check_residues(name, call(by_res), sets, host, nq)                                  # C3
    # C4 on list c (a row through three tiles)
    deg = DEGREES["c"]
    xd = (torch.rand(len(deg), 3, generator=gen) * 2 - 1).to(DEV)
    src, dst, rowptr = JREF.ragged_list(deg, NSRC, gen)
    g = jr._graph(src, dst, rowptr, NSRC)
    _check_slots(f"gno_jet2_rows_qd/{mode}/nh{nh}/list_c", lambda qd: ops.gno_forward_jet2_qd(mode, wd, bd, yd, xd, fk, t, g, qd),
                 _rand_dirs(len(deg), 1, gen).to(DEV))


@pytest.mark.parametrize("mode", MODES)
def test_regular_rows_equal_the_regular_list_kernel(mode):
    """C5, first half: on a list whose rows all have k | 32 edges the two kernels agree bit for bit"""
    from gaot_3d_amd import ops
    for nh in (1, 2, 3, 4):
        gen, y, f, ws, bs, yd, wd, bd, fk, t = jr._device_operands(nh, mode)
        for nq in (7, 33):
            xd = (torch.rand(nq, 3, generator=gen) * 2 - 1).to(DEV)
            qd = _rand_dirs(nq, 3, gen).to(DEV)
            for k in (1, 4, 32):
                src, dst, rowptr = JREF.ragged_list([k] * nq, NSRC, gen)
                got = ops.gno_forward_jet2_qd(mode, wd, bd, yd, xd, fk, t, jr._graph(src, dst, rowptr, NSRC), qd)
                knn = ops.gno_forward_knn_jet2_qd(mode, wd, bd, yd, xd, fk, t, src.to(DEV), k, qd)
                for a, b in zip(got, knn):
                    assert torch.equal(a, b), (nh, nq, k, (a - b).abs().max().item())


@pytest.mark.parametrize("mode", MODES)
def test_a_piece_led_by_padding_edges_equals_its_rows_in_the_whole_list(mode):
    """C5, second half: rows [a, b) of list e with their directions, cut out and led by (edges before row a) mod 32 padding edges
    (which read query 0's directions and are dropped): all planes of those rows are the whole list's -- what makes sample_directional
    independent of its chunks"""
    from gaot_3d_amd import ops
    gen, y, f, ws, bs, yd, wd, bd, fk, t = jr._device_operands(3, mode)
    deg = DEGREES["e"]
    nq = len(deg)
    xd = (torch.rand(nq, 3, generator=gen) * 2 - 1).to(DEV)
    qd = _rand_dirs(nq, 3, gen).to(DEV)
    src, dst, rowptr = JREF.ragged_list(deg, NSRC, gen)
    out, d1, d2 = ops.gno_forward_jet2_qd(mode, wd, bd, yd, xd, fk, t, jr._graph(src, dst, rowptr, NSRC), qd)
    for a, b in ((0, 1000), (1000, 1064), (1064, 3000), (2990, 3000)):
        e0, e1 = int(rowptr[a]), int(rowptr[b])
        lead = e0 % 32
        psrc = torch.cat([torch.zeros(lead, dtype=torch.int32), src[e0:e1]])
        pdst = torch.cat([torch.full((lead,), -1, dtype=torch.int32), dst[e0:e1] - a])
        prow = rowptr[a:b + 1] - e0 + lead
        po, p1, p2 = ops.gno_forward_jet2_qd(mode, wd, bd, yd, xd[a:b].contiguous(), fk, t, jr._graph(psrc, pdst, prow, NSRC), qd[a:b])
        assert torch.equal(po, out[a:b]) and torch.equal(p1, d1[:, a:b]) and torch.equal(p2, d2[:, a:b]), (a, b)


def test_row_lists_bad_arguments_zero_edges_and_zero_queries():
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
    nd = 3
    qd = _rand_dirs(nq, nd, gen).to(DEV)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    w128, b128 = hb._mlp(2, "linear", gen, hidden=128)
    with pytest.raises(GaotError, match="gaot_gno_fwd_jet2_qd: unsupported MLP shape"):
        ops.gno_forward_jet2_qd("linear", [w.to(DEV) for w in w128], [b.to(DEV) for b in b128], yd, xd, fd, None, g, qd)
    with pytest.raises(GaotError, match="mode must be"):
        ops.gno_forward_jet2_qd("cubic", wd, bd, yd, xd, fd, None, g, qd)
    with pytest.raises(GaotError, match="rows, the graph"):
        ops.gno_forward_jet2_qd("linear", wd, bd, yd, xd[:-1], fd, None, g, qd[:-1])
    for dirs, msg in ((qd[:, :0], "gaot_gno_fwd_jet2_qd: nd must be"), (torch.cat([qd, qd, qd[:, :1]], 1), "gaot_gno_fwd_jet2_qd: nd must be"),
                      (qd[:-1], "qdirs must be"), (qd[:, :, :2], "qdirs must be"), (qd.cpu(), "float32 tensor on"),
                      (qd.double(), "float32 tensor on"), (GENERIC[:3], "float32 tensor on")):
        with pytest.raises(GaotError, match=msg):
            ops.gno_forward_jet2_qd("linear", wd, bd, yd, xd, fd, None, g, dirs)
    assert ops.launch_count() == n0
    m, keep = ops._mlp_struct(wd, bd)
    out = torch.empty(nq, 32, device=DEV)
    d1 = torch.empty(nd, nq, 32, device=DEV)
    d2 = torch.empty(nd, nq, 32, device=DEV)
    need = lib.gaot_gno_fwd_jet2_workspace_bytes(e, nd)
    ws_ = torch.empty(need, dtype=torch.uint8, device=DEV)
    ptr = lambda t_: C.c_void_p(t_.data_ptr())
    null = C.c_void_p(0)
    by = g.by_dst

    def call(mode=0, yp=ptr(yd), xp=ptr(xd), fp=ptr(fd), tab=null, s=ptr(by.other), d=ptr(by.key), rp=ptr(by.rowptr), ne=e, q=nq,
             dv=ptr(qd), n=nd, o=ptr(out), p1=ptr(d1), p2=ptr(d2), w=ptr(ws_), wb=need):
        _lib.check(lib.gaot_gno_fwd_jet2_qd(C.byref(m), mode, yp, xp, fp, tab, s, d, rp, ne, q, dv, n, o, p1, p2, w, wb, null),
                   "gaot_gno_fwd_jet2_qd")

    for kw, msg in ((dict(mode=3), "mode must be"), (dict(n=0), "nd must be"), (dict(n=7), "nd must be"), (dict(dv=null), "null qdirs"),
                    (dict(p1=null), "null pointer"), (dict(p2=null), "null pointer"), (dict(o=null), "null pointer"),
                    (dict(fp=null), "null pointer"), (dict(s=null), "null pointer"), (dict(d=null), "null pointer"),
                    (dict(rp=null), "null pointer"), (dict(yp=null), "null pointer"), (dict(xp=null), "null pointer"),
                    (dict(mode=1), "null src_table"), (dict(w=null), "null workspace"), (dict(wb=need - 1), "workspace too small"),
                    (dict(ne=-1), "negative size"), (dict(q=-1), "negative size"), (dict(ne=1 << 31), "beyond int32")):
        with pytest.raises(GaotError, match="gaot_gno_fwd_jet2_qd: .*" + msg):
            call(**kw)
        assert ops.launch_count() == n0, kw
    call(q=0)                                                                                # zero queries: no launch
    assert ops.launch_count() == n0
    for t_ in (out, d1, d2):
        t_.fill_(1.0)
    zero_rows = torch.zeros(nq + 1, dtype=torch.int32, device=DEV)
    call(ne=0, rp=ptr(zero_rows), s=null, d=null, w=null, wb=0, fp=null, yp=null, xp=null, dv=null)   # zero edges: the fix-up alone, zeros
    assert ops.launch_count() == n0 + 1
    assert not out.any() and not d1.any() and not d2.any()
    call()                                                                                   # and a good call: TWO launches
    assert ops.launch_count() == n0 + 3
    good = ops.gno_forward_jet2_qd("linear", wd, bd, yd, xd, fd, None, g, qd)
    assert torch.equal(out, good[0]) and torch.equal(d1, good[1]) and torch.equal(d2, good[2])


# ---- model level ------------------------------------------------------------------------------------------------------------------------
STRATEGIES = ("knn", "radius", "bidirectional")
CHUNKS = (None, 250, 64)


def _model(strategy, out=1, **more):
    """-> (key, (model, batch, tokens, cfg)): the fixtures of the Hessian tests, shared with them (and their oracle results by key)"""
    if strategy == "knn":
        key = "shape/" + more.pop("case") if "case" in more else "cfg0"
        return key, hb._setup(key, out=out, **more)
    return hr._model(strategy, out=out, **more)


def _oracle(strategy, key, model, cfg, lat, q):
    """(pred, jac [Nq, out, 3], hess [Nq, out, 3, 3]) of the fp64 oracle's decoder on the edges of the lists actually used"""
    return (hb._oracle_hessian if strategy == "knn" else hr._oracle_hessian)(key, model, cfg, lat, q)[:3]


def _contract(jac, hess, dirs):
    """J v and v^T H v per query: [Nq, out, nd] each"""
    v = dirs.detach().double().cpu()
    return torch.einsum("qod,qid->qoi", jac, v), torch.einsum("qid,qode,qie->qoi", v, hess, v)


def _frames(nq, gen):
    """an orthonormal frame (n, t1, t2) per query, built from random vectors by Gram-Schmidt in fp64"""
    a = torch.randn(nq, 3, 3, generator=gen, dtype=torch.float64)
    n = a[:, 0] / a[:, 0].norm(dim=1, keepdim=True)
    t1 = a[:, 1] - (a[:, 1] * n).sum(1, keepdim=True) * n
    t1 = t1 / t1.norm(dim=1, keepdim=True)
    t2 = torch.linalg.cross(n, t1)
    return torch.stack([n, t1, t2], dim=1).float().contiguous()


def _streamed_qd(seen, strategy):
    """only the per-query GNO keys and the projection's jets: no CSR build, no backward, no host-direction jet key"""
    keys = seen["keys"]
    mine = "gno_jet2_knn_qd" if strategy == "knn" else "gno_jet2_rows_qd"
    gno = [k for k in keys if k.startswith("gno_")]
    return (bool(gno) and all(k.startswith(mine) for k in gno) and any(k.startswith("mlp2_jet2") for k in keys) and seen["csr"] == 0
            and not any(k.startswith("csr_build") for k in keys))


def _rows_kind(strategy):
    return "" if strategy == "knn" else "_rows"


def _axes_identities(name, model, lat, q, strategy, chunk=None):
    """C7: with the three axes for every query pred / d1 are sample_jacobian's and d2 is the diagonal of sample_hessian(_rows)'s"""
    pred, d1, d2 = model.sample_directional(lat, q, _uniform(AXES, q.shape[0]), chunk_points=chunk)
    pj, jj = model.sample_jacobian(lat, q, chunk_points=chunk, row_lists=True)
    ph, jh, hh = getattr(model, "sample_hessian" + _rows_kind(strategy))(lat, q, chunk_points=chunk)
    i3 = torch.arange(3)
    assert torch.equal(pred, pj) and torch.equal(d1, jj), (name, (d1 - jj).abs().max().item())
    assert torch.equal(d2, hh[:, :, i3, i3]), (name, (d2 - hh[:, :, i3, i3]).abs().max().item())


_GOT = {}


def _results(strategy, monkeypatch):
    """sample_directional of the 600 queries along random directions (nd = 3) at every chunking, once per strategy"""
    if strategy not in _GOT:
        key, (model, batch, tokens, cfg) = _model(strategy)
        q = hb._queries(batch)
        dirs = _rand_dirs(q.shape[0], 3, torch.Generator().manual_seed(17)).to(DEV)
        with torch.no_grad():
            lat = model.latent(batch, tokens)
        got = {}
        for chunk in CHUNKS:
            with hb._watch(monkeypatch) as seen:
                got[chunk] = model.sample_directional(lat, q, dirs, chunk_points=chunk)
            assert _streamed_qd(seen, strategy), seen
        _GOT[strategy] = (key, model, cfg, q, dirs, lat, got)
    return _GOT[strategy]


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_sample_directional_meets_the_oracle(strategy, monkeypatch):
    key, model, cfg, q, dirs, lat, got = _results(strategy, monkeypatch)
    ref_p, ref_j, ref_h = _oracle(strategy, key, model, cfg, lat, q)
    pred, d1, d2 = got[None]
    assert pred.shape == (600, 1) and d1.shape == d2.shape == (600, 1, 3)
    for t in (pred, d1, d2):
        assert not t.requires_grad and t.grad_fn is None
    assert torch.allclose(pred.cpu().double(), ref_p, rtol=1e-4, atol=1e-5)
    r1, r2 = _contract(ref_j, ref_h, dirs)
    hb.check(f"sample_directional/{strategy}/d1", d1, r1)                                     # no query excluded
    hb.check(f"sample_directional/{strategy}/d2", d2, r2)
    # [Nq, 3] is one direction per query; a latent that requires grad still gives results outside autograd
    one = model.sample_directional(lat, q, dirs[:, 0].contiguous())
    assert one[1].shape == (600, 1, 1) and torch.equal(one[0], pred) and torch.equal(one[1][..., 0], d1[..., 0]) and torch.equal(one[2][..., 0], d2[..., 0])
    lat_g = model.latent(*_model(strategy)[1][1:3])
    assert lat_g.requires_grad and not any(t.requires_grad for t in model.sample_directional(lat_g, q[:100], dirs[:100]))
    # directions are used as given: d1 is linear and d2 quadratic in their length (a power of two scales exactly)
    _, h1, h2 = model.sample_directional(lat, q, 2.0 * dirs)
    assert torch.equal(h1, 2.0 * d1) and torch.equal(h2, 4.0 * d2)


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_orthonormal_frames_sum_to_the_laplacian(strategy):
    """the trace is invariant under rotation: D^2_n + D^2_t1 + D^2_t2 in any orthonormal frame is the Laplacian"""
    key, (model, batch, tokens, cfg) = _model(strategy)
    q = hb._queries(batch)
    frames = _frames(q.shape[0], torch.Generator().manual_seed(23)).to(DEV)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    pred, d1, d2 = model.sample_directional(lat, q, frames)
    pl, lap = getattr(model, "sample_laplacian" + _rows_kind(strategy))(lat, q)
    assert torch.equal(pred, pl)
    hb.check(f"sample_directional/{strategy}/frame_trace_against_laplacian", d2.sum(-1), lap)
    ref_p, ref_j, ref_h = _oracle(strategy, key, model, cfg, lat, q)
    hb.check(f"sample_directional/{strategy}/frame_trace_against_oracle", d2.sum(-1), ref_h[..., 0, 0] + ref_h[..., 1, 1] + ref_h[..., 2, 2])


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_chunkings_and_bf16_mode_are_bit_identical(strategy, monkeypatch):
    key, model, cfg, q, dirs, lat, got = _results(strategy, monkeypatch)
    for chunk in CHUNKS[1:]:
        assert all(torch.equal(a, b) for a, b in zip(got[chunk], got[None])), chunk           # C6
    with hb._precision("bf16"):
        bf = model.sample_directional(lat, q, dirs, chunk_points=250)
    assert all(torch.equal(a, b) for a, b in zip(bf, got[None]))


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_axes_give_the_jacobian_and_the_hessian_diagonal(strategy):
    key, (model, batch, tokens, cfg) = _model(strategy)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    _axes_identities(f"sample_directional/{strategy}/axes", model, lat, hb._queries(batch), strategy, chunk=250)


SHAPES = {**{f"knn/{case}": ("knn", kw.get("out", 1), {"case": case, **{a: b for a, b in kw.items() if a != "out"}})
             for case, kw in hb.SHAPES.items()},
          **{f"rows/{case}": spec for case, spec in hr.SHAPES.items()}}


@pytest.mark.parametrize("case", list(SHAPES))
def test_other_shapes_stream(case, monkeypatch):
    """four channels, 'nonlinear', two scales (softmax-weighted: on rows the mix carries w' and w'' along every row's own direction;
    summed), four hidden layers -- the bar against the oracle and C7, bit for bit, softmax weights included"""
    strategy, out, kw = SHAPES[case]
    key, (model, batch, tokens, cfg) = _model(strategy, out=out, **kw)
    q = hb._queries(batch, 0, 300) if strategy == "knn" else hb._queries(batch, 150, 150)
    dirs = _rand_dirs(q.shape[0], 2, torch.Generator().manual_seed(29)).to(DEV)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    ref_p, ref_j, ref_h = _oracle(strategy, key, model, cfg, lat, q)
    with hb._watch(monkeypatch) as seen:
        pred, d1, d2 = model.sample_directional(lat, q, dirs, chunk_points=128)
    assert _streamed_qd(seen, strategy), seen
    assert torch.allclose(pred.cpu().double(), ref_p, rtol=1e-4, atol=1e-5), case
    r1, r2 = _contract(ref_j, ref_h, dirs)
    hb.check(f"sample_directional/{case}/d1", d1, r1)
    hb.check(f"sample_directional/{case}/d2", d2, r2)
    _axes_identities(f"sample_directional/{case}/axes", model, lat, q, strategy, chunk=128)


def test_queries_far_from_every_token_have_zero_derivatives():
    """queries at a distance have EMPTY rows on a 'radius' decoder: the prediction is sample's bit for bit and every derivative is
    exactly zero, whatever their directions -- among queries that do have rows, in one chunk and cut apart"""
    key, (model, batch, tokens, cfg) = _model("radius")
    far = torch.tensor([[3.0, 0.1, -0.2], [-2.5, 2.5, 0.0], [0.3, 0.2, 4.0]], device=DEV)
    q = torch.cat([far[:1], batch.pos[:40], far[1:2], batch.pos[40:70], far[2:]]).contiguous()
    idx = torch.tensor([0, 41, 72], device=DEV)
    dirs = _rand_dirs(q.shape[0], 3, torch.Generator().manual_seed(31)).to(DEV)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
        smp = model.sample(lat, q)
    for chunk in (None, 41):
        pred, d1, d2 = model.sample_directional(lat, q, dirs, chunk_points=chunk)
        assert torch.equal(pred, smp)
        for t in (d1[idx], d2[idx]):
            assert torch.equal(t, torch.zeros_like(t)), chunk
        assert d2.abs().amax(dim=(1, 2)).gt(0).sum() == q.shape[0] - 3


def test_graph_replay_on_knn_equals_eager_with_new_coordinates_and_directions():
    key, (model, batch, tokens, cfg) = _model("knn")
    qs = hb._queries(batch, 1500, 1500)
    q1, q2 = qs[:1500].contiguous(), qs[1500:].contiguous()
    gen = torch.Generator().manual_seed(37)
    v1, v2 = _rand_dirs(1500, 3, gen).to(DEV), _rand_dirs(1500, 3, gen).to(DEV)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    qbuf, vbuf = q1.clone(), v1.clone()
    e1 = model.sample_directional(lat, qbuf, vbuf, chunk_points=600)       # the eager call: describes the grid, warms the allocator
    e2 = model.sample_directional(lat, q2, v2, chunk_points=600)
    e3 = model.sample_directional(lat, q2, v1, chunk_points=600)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model.sample_directional(lat, qbuf, vbuf, chunk_points=600)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, e1))
    qbuf.copy_(q2)                                                         # new coordinates, the old directions
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, e3))
    vbuf.copy_(v2)                                                         # and new directions: read on the device at replay
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, e2))
    assert not torch.equal(e1[2], e2[2]) and not torch.equal(e3[2], e2[2])


def test_in_a_capture_a_row_route_raises_before_any_launch():
    from gaot_3d_amd import ops
    from gaot_3d_amd._lib import GaotError
    key, (model, batch, tokens, cfg) = _model("bidirectional")
    q = batch.pos[:300].contiguous()
    dirs = _rand_dirs(300, 2, torch.Generator().manual_seed(41)).to(DEV)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    eager = model.sample_directional(lat, q, dirs)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(GaotError, match="captured"):
        with torch.cuda.graph(g):
            model.sample_directional(lat, q, dirs)
    assert ops.launch_count() == n0
    torch.cuda.synchronize()
    again = model.sample_directional(lat, q, dirs)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(again, eager))


REFUSALS = {**{f"knn/{case}": ("knn", case, "second derivatives")
               for case in ("use_attn", "geoembed", "k3", "projection96")},
            **{f"rows/{case}": ("rows", case, "second derivatives on row lists.*" + spec[3]) for case, spec in hr.REFUSALS.items()}}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_other_configurations_are_refused(case):
    from gaot_3d_amd import ops
    route, name, msg = REFUSALS[case]
    if route == "knn":
        model, batch, tokens, cfg = hb._setup("refuse/" + name, **hb.REFUSALS[name])
    else:
        strategy, k, kw, _ = hr.REFUSALS[name]
        _, (model, batch, tokens, cfg) = hr._model(strategy, k=k, **kw)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    dirs = _uniform(GENERIC[:2], 200)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    with pytest.raises(NotImplementedError, match=msg):
        model.sample_directional(lat, batch.pos[:200], dirs)
    assert ops.launch_count() == n0


@pytest.mark.parametrize("strategy", ["knn", "radius"])
def test_sampling_off_grid_tokens_and_argument_errors(strategy):
    from gaot_3d_amd import ops
    key, (model, batch, tokens, cfg) = _model(strategy)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    q = batch.pos[:100].contiguous()
    dirs = _uniform(GENERIC[:2], 100)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    model.decoder.sampling_strategy = "max_neighbors"
    try:
        with pytest.raises(NotImplementedError, match="neighbour sampling"):
            model.sample_directional(lat, q, dirs)
    finally:
        model.decoder.sampling_strategy = None
    for bad, msg in ((dirs[:-1], "100 queries"), (dirs[:, :0], "nd = 0"), (torch.cat([dirs] * 4, 1), "nd = 8"), (dirs[:, :, :2], "3 components"),
                     (dirs.double(), "float32"), (dirs.cpu(), "device")):
        with pytest.raises(ValueError, match=msg):
            model.sample_directional(lat, q, bad)
    with pytest.raises(ValueError, match="chunk_points"):
        model.sample_directional(lat, q, dirs, chunk_points=0)
    kept = model.decoder.decoder_strategy
    model.decoder.decoder_strategy = "reverse"
    try:
        with pytest.raises(ValueError, match="reverse"):
            model.sample_directional(lat, q, dirs)
    finally:
        model.decoder.decoder_strategy = kept
    assert ops.launch_count() == n0
    off = (tokens + 0.01 * torch.rand_like(tokens)).contiguous()           # tokens off the regular grid
    with pytest.raises(NotImplementedError, match="do not stream"):
        model.sample_directional(lat, q, dirs, tokens_pos=off)
    good = model.sample_directional(lat, q, dirs)                          # and the model still streams
    assert good[1].abs().max() > 0
