"""Spatial derivatives of the sampled field: gaot_gno_fwd_knn_jac (the fused GNO forward on a regular k-neighbour list with three
forward-mode tangents), IntegralTransform.jacobian_knn, jvp_rows of the per-point MLPs, MAGNODecoder / GAOT3D.sample_jacobian.

  * op level: Nq in {1, 7, 33, 1000} x k in {1 .. 32} x 1..4 hidden layers x the three transform types; the value plane is
    torch.equal to ops.gno_forward_knn(precision=0), the Jacobian meets the fp32 bar for coordinate gradients
    (tests/test_coord_grad_gpu.py FP32_BAR: max error <= 1e-3 of the reference's peak, cosine >= 0.99999) against the closed-form
    fp64 reference tests/gno_jac_ref.py;
  * bad arguments raise GaotError before any launch;
  * jvp_rows (1000 rows, 32 -> 256 -> 4, GELU, both MLP classes) against fp64 autograd of the same MLP;
  * model level (4096 points, latent 8 x 8 x 8, k = 8, two layers, eval): sample_jacobian against the Jacobian assembled from
    forward(query_coord_pos=q.requires_grad_()) with one autograd.grad per output channel, at the sample's points and at random
    points partly outside the box, chunkings bit-identical, pred torch.equal to sample, no CSR build and no gno_bwd*;
  * bf16 mode returns the fp32-mode result bit for bit; other shapes stream through padding; radius / bidirectional / k = 3 /
    pointnet GeoEmbed decoders take the autograd route; use_attn / statistical GeoEmbed / reverse raise;
  * memory: nothing but the results grows with Nq; the autograd route needs at least four times the streaming route's remainder;
  * sample_jacobian captured in a hipGraph replays, with new coordinates in the captured buffer, to the eager result bit for bit."""
import contextlib
import ctypes as C
import math
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gno_jac_ref as REF  # noqa: E402
import parity as PAR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("linear", "nonlinear", "nonlinear_kernelonly")
KS = (1, 2, 4, 8, 16, 32)
NQS = (1, 7, 33, 1000)      # Nq * k below one 32-edge tile, ragged against it, and many workgroups
NSRC = 211
FP32_BAR = (1e-3, 0.99999)  # tests/test_coord_grad_gpu.py: max error relative to the reference's peak, cosine


def measure(got, ref):
    got = got.detach().double().cpu().reshape(-1)
    ref = ref.detach().double().cpu().reshape(-1)
    err = (got - ref).abs().max().item()
    peak = ref.abs().max().item()
    cos = (got @ ref).item() / (got.norm().item() * ref.norm().item() + 1e-300)
    return err, peak, cos


def check(name, got, ref, bar=FP32_BAR, quiet=False):
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    rel, cos_min = bar
    err, peak, cos = measure(got, ref)
    if not quiet:
        print(f"[parity] {name}: max_abs={err:.3e} rel_to_peak={err / (peak + 1e-300):.3e} cosine={cos:.7f} peak={peak:.3e}")
    assert peak > 0, f"{name}: reference Jacobian is zero"
    assert err <= rel * peak and cos >= cos_min, f"{name}: max err {err:.3e} (peak {peak:.3e}), cosine {cos:.7f}"
    return err / peak, cos


@contextlib.contextmanager
def _precision(p):
    import gaot_3d_amd
    gaot_3d_amd.set_precision(p)
    try:
        yield
    finally:
        gaot_3d_amd.set_precision("fp32")


# ---- op level ---------------------------------------------------------------------------------------------------------------------------
def _mlp(nh, mode, gen, hidden=64):
    cin = 0 if mode == "linear" else 32
    dims = [6 + cin] + [hidden] * nh + [32]
    ws = [torch.randn(dims[i + 1], dims[i], generator=gen) / math.sqrt(dims[i]) for i in range(len(dims) - 1)]
    bs = [0.1 * torch.randn(dims[i + 1], generator=gen) for i in range(len(dims) - 1)]
    return ws, bs


def _operands(nh, mode):
    gen = torch.Generator().manual_seed(100 * nh + MODES.index(mode))
    y = torch.rand(NSRC, 3, generator=gen) * 2 - 1
    f = torch.randn(NSRC, 32, generator=gen)
    ws, bs = _mlp(nh, mode, gen)
    return gen, y, f, ws, bs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nh", [1, 2, 3, 4])
def test_value_is_the_knn_forward_and_jacobian_meets_the_bar(nh, mode):
    from gaot_3d_amd import ops
    gen, y, f, ws, bs = _operands(nh, mode)
    yd, fd = y.to(DEV), f.to(DEV)
    wd, bd = [w.to(DEV) for w in ws], [b.to(DEV) for b in bs]
    t = None
    if mode != "linear":
        t = (f.double() @ ws[0][:, 6:].double().t()).float().to(DEV)       # the per-node term of layer 0, as the host layer forms it
        wd = [ws[0][:, :6].contiguous().to(DEV)] + wd[1:]
    fk = None if mode == "nonlinear_kernelonly" else fd
    worst_rel, worst_cos = 0.0, 1.0
    for nq in NQS:
        x = torch.rand(nq, 3, generator=gen) * 2 - 1
        xd = x.to(DEV)
        for k in KS:
            nbr = torch.randint(0, NSRC, (nq * k,), generator=gen, dtype=torch.int32)        # repeats allowed
            nd = nbr.to(DEV)
            n0 = ops.launch_count()
            out, jac = ops.gno_forward_knn_jac(mode, wd, bd, yd, xd, fk, t, nd, k)
            assert ops.launch_count() == n0 + 1                                              # ONE launch
            assert out.shape == (nq, 32) and jac.shape == (3, nq, 32) and jac.is_contiguous()
            val = ops.gno_forward_knn(mode, wd, bd, yd, xd, fk, t, nd, k, precision=0)
            assert torch.equal(out, val), (nq, k, (out - val).abs().max().item())
            # the reference evaluates the same fp32 operands (t is part of layer 0 there: W_0 with its feature columns)
            ro, rj = REF.gno_knn_jac(ws, bs, y, x, nbr, k, f, mode)
            assert torch.allclose(out.cpu().double(), ro, rtol=1e-4, atol=1e-5), (nq, k)
            rel, cos = check(f"gno_fwd_knn_jac/{mode}/nh{nh}/nq{nq}/k{k}", jac, rj, quiet=True)
            worst_rel, worst_cos = max(worst_rel, rel), min(worst_cos, cos)
    print(f"[parity] gno_fwd_knn_jac/{mode}/nh{nh}: worst rel_to_peak={worst_rel:.3e} worst cosine={worst_cos:.7f} over "
          f"{len(NQS) * len(KS)} shapes (bar {FP32_BAR[0]:.0e} / {FP32_BAR[1]})")


def test_bad_arguments_raise_before_any_launch():
    from gaot_3d_amd import _lib, ops
    from gaot_3d_amd._lib import GaotError
    lib = _lib.load()
    gen, y, f, ws, bs = _operands(2, "linear")
    yd, fd = y.to(DEV), f.to(DEV)
    wd, bd = [w.to(DEV) for w in ws], [b.to(DEV) for b in bs]
    nq = 40
    xd = (torch.rand(nq, 3, generator=gen) * 2 - 1).to(DEV)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    with pytest.raises(GaotError, match="gaot_gno_fwd_knn_jac: k must be"):
        ops.gno_forward_knn_jac("linear", wd, bd, yd, xd, fd, None, torch.zeros(nq * 3, dtype=torch.int32, device=DEV), 3)
    assert ops.launch_count() == n0
    w128, b128 = _mlp(2, "linear", gen, hidden=128)
    with pytest.raises(GaotError, match="gaot_gno_fwd_knn_jac: unsupported MLP shape"):
        ops.gno_forward_knn_jac("linear", [w.to(DEV) for w in w128], [b.to(DEV) for b in b128], yd, xd, fd, None,
                                torch.zeros(nq * 8, dtype=torch.int32, device=DEV), 8)
    assert ops.launch_count() == n0
    m, keep = ops._mlp_struct(wd, bd)
    nbr = torch.zeros(nq * 8, dtype=torch.int32, device=DEV)
    out = torch.empty(nq, 32, device=DEV)
    jac = torch.empty(3, nq, 32, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)
    with pytest.raises(GaotError, match="gaot_gno_fwd_knn_jac: null pointer"):       # a null jac
        _lib.check(lib.gaot_gno_fwd_knn_jac(C.byref(m), 0, ptr(yd), ptr(xd), ptr(fd), null, ptr(nbr), 8, nq, ptr(out), null, null),
                   "gaot_gno_fwd_knn_jac")
    assert ops.launch_count() == n0
    with pytest.raises(GaotError, match="gaot_gno_fwd_knn_jac: null src_table"):
        _lib.check(lib.gaot_gno_fwd_knn_jac(C.byref(m), 1, ptr(yd), ptr(xd), ptr(fd), null, ptr(nbr), 8, nq, ptr(out), ptr(jac), null),
                   "gaot_gno_fwd_knn_jac")
    assert ops.launch_count() == n0
    with pytest.raises(GaotError, match="gaot_gno_fwd_knn_jac: .*beyond int32"):
        _lib.check(lib.gaot_gno_fwd_knn_jac(C.byref(m), 0, ptr(yd), ptr(xd), ptr(fd), null, ptr(nbr), 8, 1 << 28, ptr(out), ptr(jac),
                                            null), "gaot_gno_fwd_knn_jac")
    assert ops.launch_count() == n0
    # zero queries: no launch; and a good call is ONE launch
    _lib.check(lib.gaot_gno_fwd_knn_jac(C.byref(m), 0, ptr(yd), ptr(xd), ptr(fd), null, ptr(nbr), 8, 0, ptr(out), ptr(jac), null),
               "gaot_gno_fwd_knn_jac")
    assert ops.launch_count() == n0
    ops.gno_forward_knn_jac("linear", wd, bd, yd, xd, fd, None, nbr, 8)
    assert ops.launch_count() == n0 + 1


# ---- the per-point MLP's tangent ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["linear", "channel"])
def test_jvp_rows_against_fp64_autograd(kind):
    from gaot_3d_amd.model.layers.mlp import ChannelMLP, LinearChannelMLP
    torch.manual_seed(5)
    mlp = LinearChannelMLP([32, 256, 4]) if kind == "linear" else ChannelMLP(32, 4, 256, n_layers=2)
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(1000, 32, generator=gen)
    dxs = [torch.randn(1000, 32, generator=gen) for _ in range(3)]
    # fp64 reference on the CPU: the same MLP, one backward per output channel
    w = [(fc.weight[:, :, 0] if fc.weight.dim() == 3 else fc.weight).detach().double() for fc in mlp.fcs]
    b = [fc.bias.detach().double() for fc in mlp.fcs]
    xg = x.double().requires_grad_(True)
    yr = torch.nn.functional.gelu(xg @ w[0].t() + b[0]) @ w[1].t() + b[1]
    grads = [torch.autograd.grad(yr[:, o].sum(), xg, retain_graph=True)[0] for o in range(4)]          # [N, 32] each
    refs = [torch.stack([(g * d.double()).sum(1) for g in grads], dim=1) for d in dxs]                  # [N, 4] each
    mlp = mlp.to(DEV).eval()
    y, dys = mlp.jvp_rows(x.to(DEV), [d.to(DEV) for d in dxs])
    assert y.shape == (1000, 4) and len(dys) == 3 and not y.requires_grad and not dys[0].requires_grad
    with torch.no_grad():
        assert torch.equal(y, mlp.forward_rows(x.to(DEV)))
    assert torch.allclose(y.cpu().double(), yr.detach(), rtol=1e-4, atol=1e-5)
    for d in range(3):
        check(f"jvp_rows/{kind}/direction{d}", dys[d], refs[d])


# ---- model level ------------------------------------------------------------------------------------------------------------------------
NPTS, LATENT = 4096, (8, 8, 8)
_MODELS = {}


def _setup(key="cfg0", k=8, out=1, **magno):
    """a configs[0]-shaped model in eval mode with its sample, built once per variant and shared by the tests"""
    if key in _MODELS:
        return _MODELS[key]
    from gaot_3d_amd.data import make_synthetic_sample
    from gaot_3d_amd.model import init_model
    from gaot_3d_amd.model.layers.attn import AttentionConfig, FFNConfig, TransformerConfig
    from gaot_3d_amd.model.layers.magno import MAGNOConfig
    kw = dict(gno_coord_dim=3, lifting_channels=32, encoder_feature_attr="pos", mlp_type="linear", use_geoembed=[True, False],
              neighbor_strategy="knn", k_neighbors=k, precompute_edges=True)
    kw.update(magno)
    cfg = types.SimpleNamespace(
        magno=MAGNOConfig(**kw),
        transformer=TransformerConfig(patch_size=2, hidden_size=256, num_layers=2, positional_embedding="rope",
                                      attn_config=AttentionConfig(hidden_size=256, num_heads=8, num_kv_heads=8, atten_dropout=0.0),
                                      ffn_config=FFNConfig(hidden_size=1024)),
        latent_tokens=LATENT)
    torch.manual_seed(0)
    model = init_model(3, out, "gaot_3d", cfg)
    batch, tokens = make_synthetic_sample(NPTS, LATENT, k=k, in_normals=False, surface=False, seed=0)
    for si in range(1, len(kw.get("scales", [1.0]))):       # knn lists do not depend on the scale: every scale sees the same edges
        setattr(batch, f"encoder_edge_index_s{si}", batch.encoder_edge_index_s0)
        setattr(batch, f"decoder_edge_index_s{si}", batch.decoder_edge_index_s0)
    # an untrained model predicts O(1e-2): rescale its last affine map so that predictions are O(1)
    model = model.to(DEV).eval()
    bd, td = batch.to(DEV), tokens.to(DEV)
    with torch.no_grad():
        p0 = model(bd, td)
        last = model.decoder.projection.fcs[-1]
        PAR.unit_scale_last_layer(last.weight, last.bias, float(p0.std()))
    _MODELS[key] = (model, bd, td)
    return _MODELS[key]


@contextlib.contextmanager
def _watch(monkeypatch):
    """timing keys and CSR builds of the calls made inside"""
    from gaot_3d_amd import ops
    seen = {"csr": 0, "keys": set()}
    real = ops.csr_build

    def counted(*a, **k):
        seen["csr"] += 1
        return real(*a, **k)
    monkeypatch.setattr(ops, "csr_build", counted)
    ops.timing_reset(True)
    try:
        yield seen
        torch.cuda.synchronize()
        seen["keys"] = set(ops.timing_summary())
    finally:
        ops.timing_reset(False)
        monkeypatch.setattr(ops, "csr_build", real)


def _streamed(seen):
    keys = seen["keys"]
    return (any(k.startswith("gno_fwd_knn_jac") for k in keys) and seen["csr"] == 0
            and not any(k.startswith("csr_build") or k.startswith("gno_bwd") for k in keys))


_REFS = {}


def _autograd_jacobian(key, model, batch, tokens, q):
    """(pred [Nq, out], jac [Nq, out, 3]) through forward's own route: edges built on the device for the queries, one autograd.grad
    per output channel; computed once per (model, query set) and shared"""
    if key in _REFS:
        return _REFS[key]
    qg = q.detach().clone().requires_grad_(True)
    model.decoder.precompute_edges = False
    try:
        p = model(batch, tokens, query_coord_pos=qg, query_coord_batch_idx=torch.zeros(q.shape[0], dtype=torch.long, device=q.device))
    finally:
        model.decoder.precompute_edges = True
    cols = [torch.autograd.grad(p[:, o].sum(), qg, retain_graph=o + 1 < p.shape[1])[0] for o in range(p.shape[1])]
    _REFS[key] = (p.detach(), torch.stack(cols, dim=1))
    return _REFS[key]


def _queries(which, batch):
    if which == "points":
        return batch.pos
    gen = torch.Generator().manual_seed(7)
    return (torch.rand(3000, 3, generator=gen) * 2.4 - 1.2).to(DEV)                   # some of them outside the grid's box


@pytest.mark.parametrize("which", ["points", "random"])
def test_sample_jacobian_equals_the_autograd_jacobian(which, monkeypatch):
    model, batch, tokens = _setup()
    q = _queries(which, batch)
    ref_p, ref_j = _autograd_jacobian(("cfg0", which), model, batch, tokens, q)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
        smp = model.sample(lat, q)
    got = {}
    for chunk in (None, 1000, 64):
        with _watch(monkeypatch) as seen:
            got[chunk] = model.sample_jacobian(lat, q, chunk_points=chunk)
        assert _streamed(seen), seen
    pred, jac = got[None]
    assert pred.shape == (q.shape[0], 1) and jac.shape == (q.shape[0], 1, 3)
    assert not pred.requires_grad and not jac.requires_grad and pred.grad_fn is None and jac.grad_fn is None
    for chunk in (1000, 64):
        assert torch.equal(got[chunk][0], pred) and torch.equal(got[chunk][1], jac), chunk
    assert torch.equal(pred, smp)
    assert torch.allclose(pred, ref_p, rtol=1e-4, atol=1e-5)
    check(f"sample_jacobian/{which}", jac, ref_j)
    # a latent that requires grad still gives results outside autograd
    lat_g = model.latent(batch, tokens)
    assert lat_g.requires_grad
    pg, jg = model.sample_jacobian(lat_g, q[:100])
    assert not pg.requires_grad and not jg.requires_grad


def test_bf16_mode_returns_the_fp32_result():
    model, batch, tokens = _setup()
    q = _queries("random", batch)
    with torch.no_grad():
        lat = model.latent(batch, tokens)               # ONE fp32 latent tensor for both modes
    pred, jac = model.sample_jacobian(lat, q, chunk_points=1000)
    with _precision("bf16"):
        pb, jb = model.sample_jacobian(lat, q, chunk_points=1000)
    assert torch.equal(pb, pred) and torch.equal(jb, jac)


SHAPES = {
    "c16": dict(lifting_channels=16),
    "c64": dict(lifting_channels=64),
    "hidden32": dict(out_gno_channel_mlp_hidden_layers=[32, 32]),
    "nonlinear": dict(out_gno_transform_type="nonlinear"),
    "nonlinear_kernelonly": dict(out_gno_transform_type="nonlinear_kernelonly", lifting_channels=48),
    "two_scales": dict(scales=[1.0, 2.0], use_scale_weights=True),
    # four hidden layers: the forward kernels take them in fp32 mode, the fp32 backward does not (the reference runs the general path)
    "four_layers": dict(out_gno_channel_mlp_hidden_layers=[64, 64, 64, 64]),
}


@pytest.mark.parametrize("case", list(SHAPES))
def test_other_shapes_stream_through_padding(case, monkeypatch):
    model, batch, tokens = _setup("shape/" + case, out=2 if case == "two_scales" else 1, **SHAPES[case])
    q = _queries("random", batch)[:1500]
    ref_p, ref_j = _autograd_jacobian(("shape/" + case, "random"), model, batch, tokens, q)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
        smp = model.sample(lat, q)
    with _watch(monkeypatch) as seen:
        pred, jac = model.sample_jacobian(lat, q, chunk_points=700)
    assert _streamed(seen), seen
    assert torch.equal(pred, smp)
    check(f"sample_jacobian/{case}", jac, ref_j)


def test_coordinate_dimension_two_pads_with_exact_zeros():
    """IntegralTransform.jacobian_knn on 2-D coordinates: the plane of the padded direction is exactly zero, the other two meet the
    bar against autograd through forward() on the graph of the same lists"""
    from gaot_3d_amd import ops
    from gaot_3d_amd.model.layers.integral_transform import IntegralTransform
    torch.manual_seed(3)
    it = IntegralTransform(channel_mlp_layers=[4, 64, 64, 32], transform_type="linear", coord_dim=2).to(DEV).eval()
    gen = torch.Generator().manual_seed(4)
    nq, k = 333, 4
    y = (torch.rand(NSRC, 2, generator=gen) * 2 - 1).to(DEV)
    x = (torch.rand(nq, 2, generator=gen) * 2 - 1).to(DEV)
    f = torch.randn(NSRC, 32, generator=gen).to(DEV)
    nbr = torch.randint(0, NSRC, (nq * k,), generator=gen, dtype=torch.int32).to(DEV)
    out, jac = it.jacobian_knn(y, x, nbr, k, f)
    assert out.shape == (nq, 32) and jac.shape == (3, nq, 32)
    assert torch.equal(jac[2], torch.zeros_like(jac[2]))
    ei = torch.stack([nbr, torch.arange(nq, dtype=torch.int32, device=DEV).repeat_interleave(k)])
    xg = x.clone().requires_grad_(True)
    o = it(y, xg, ei, f, graph=ops.build_graph(ei, NSRC, nq))
    assert torch.equal(out, o.detach())
    ref = torch.stack([torch.autograd.grad(o[:, c].sum(), xg, retain_graph=c < 31)[0] for c in range(32)], dim=-1)   # [Nq, 2, C]
    check("jacobian_knn/coord_dim2", jac[:2], ref.permute(1, 0, 2))


FALLBACKS = {
    "radius": dict(neighbor_strategy=["knn", "radius"], gno_radius=0.45),
    "bidirectional": dict(neighbor_strategy="bidirectional", gno_radius=0.45),
    "k3": dict(),
    "pointnet": dict(use_geoembed=[True, True], embedding_method="pointnet"),
}


@pytest.mark.parametrize("case", list(FALLBACKS))
def test_fallbacks_take_the_autograd_route(case, monkeypatch):
    model, batch, tokens = _setup("fallback/" + case, k=3 if case == "k3" else 8, **FALLBACKS[case])
    q = _queries("random", batch)[:1500]
    ref_p, ref_j = _autograd_jacobian(("fallback/" + case, "random"), model, batch, tokens, q)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    with _watch(monkeypatch) as seen:
        pred, jac = model.sample_jacobian(lat, q, chunk_points=700)
    assert not any(k.startswith("gno_fwd_knn_jac") for k in seen["keys"]), seen
    assert not pred.requires_grad and not jac.requires_grad and jac.shape == (1500, 1, 3)
    assert torch.allclose(pred, ref_p, rtol=1e-5, atol=1e-6), (pred - ref_p).abs().max().item()
    print(f"[parity] sample_jacobian_fallback/{case}: max_abs={(jac - ref_j).abs().max().item():.3e} peak={ref_j.abs().max().item():.3e}")
    assert ref_j.abs().max() > 0
    assert torch.allclose(jac, ref_j, rtol=1e-5, atol=1e-6), (jac - ref_j).abs().max().item()


@pytest.mark.parametrize("case", ["use_attn", "statistical"])
def test_unsupported_decoders_raise(case):
    kw = dict(use_attn=True) if case == "use_attn" else dict(use_geoembed=[True, True], embedding_method="statistical")
    model, batch, tokens = _setup("raise/" + case, **kw)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    with pytest.raises(NotImplementedError):
        model.sample_jacobian(lat, batch.pos[:200])


def test_reverse_raises():
    model, batch, tokens = _setup()
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    model.decoder.decoder_strategy = "reverse"
    try:
        with pytest.raises(ValueError, match="reverse"):
            model.sample_jacobian(lat, batch.pos[:100])
    finally:
        model.decoder.decoder_strategy = "knn"


# ---- memory -----------------------------------------------------------------------------------------------------------------------------
MEM_CHUNK = 20000


def _rise(fn):
    fn()                                        # warm-up: lazily built tables, the grid descriptor
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del out
    return rise


def test_only_the_results_grow_with_the_number_of_queries(monkeypatch):
    model, batch, tokens = _setup()
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    rest = {}
    for nq in (200000, 800000):
        q = (torch.rand(nq, 3, generator=gen) * 2 - 1).to(DEV)
        results = 4 * nq * 1 + 4 * nq * 1 * 3                   # pred and jac, fp32
        rest[nq] = _rise(lambda: model.sample_jacobian(lat, q, chunk_points=MEM_CHUNK)) - results
    q = (torch.rand(200000, 3, generator=gen) * 2 - 1).to(DEV)
    monkeypatch.setattr(model.decoder, "_stream_grid", lambda *a: None)          # the autograd route, in one piece
    auto = _rise(lambda: model.sample_jacobian(lat, q, chunk_points=200000))
    print(f"[memory] sample_jacobian beyond its results: {rest[200000] / 2**20:.2f} MiB at 200 K, {rest[800000] / 2**20:.2f} MiB at 800 K; "
          f"autograd route at 200 K in one piece: {auto / 2**20:.2f} MiB")
    assert abs(rest[800000] - rest[200000]) < 4 * 2**20, rest
    assert auto >= 4 * rest[200000], (auto, rest)


# ---- graph replay -----------------------------------------------------------------------------------------------------------------------
def test_sample_jacobian_graph_replay_equals_eager():
    model, batch, tokens = _setup()
    qs = _queries("random", batch)
    q1, q2 = qs[:1500].contiguous(), qs[1500:].contiguous()
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    buf = q1.clone()
    e1 = model.sample_jacobian(lat, buf, chunk_points=600)          # the eager call: describes the grid, warms the allocator
    e2 = model.sample_jacobian(lat, q2, chunk_points=600)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model.sample_jacobian(lat, buf, chunk_points=600)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], e1[0]) and torch.equal(out[1], e1[1])
    buf.copy_(q2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], e2[0]) and torch.equal(out[1], e2[1])
    assert not torch.equal(e1[1], e2[1])
