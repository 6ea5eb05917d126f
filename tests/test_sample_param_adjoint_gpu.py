"""Training the decoder through the sampled field: MAGNODecoder / GAOT3D.sample_vjp_params (the latent's gradient AND every decoder
parameter's from one streamed call) and GAOT3D.sample_autograd_params (functional.SampleTrainFn).

The model fixture is tests/test_field_hessian_gpu.py's, as tests/test_field_adjoint_gpu.py uses it: 4096 points, latent 8 x 8 x 8, k = 8,
300 sample points and 300 random queries partly outside the box; 'knn' / 'radius' / 'bidirectional'; chunkings None / 250 / 64.
References: torch.autograd.grad of the fp64 oracle's decoder (oracle/gaot_oracle.py) on the CPU, on the lists actually used, with
respect to the latent and every decoder entry of the state dict.  Bar: the project's fp32 bar for derivatives (FP32_BAR: max error
<= 1e-3 of the reference's peak, cosine >= 0.99999), every peak asserted > 0.

  * grad_latent and every parameter's gradient meet the oracle at every chunking; chunkings agree within 1e-5 of the peak and are each
    reproducible bit for bit; bf16 mode is torch.equal;
  * further shapes: four output channels, two scales summed, two scales weighted on 'radius' (the weighting MLP's gradients through
    dlogits), three hidden layers, a projection the fused kernel does not take (hidden 96: the GEMM chain);
  * two scales weighted on 'knn': the mix is of equal operands -- the weighting MLP's gradients are exact zeros, the oracle's below
    1e-12 of the projection gradient's peak (checked on the CPU values first);
  * sample_autograd_params: pred torch.equal to the default, every decoder .grad torch.equal to sample_vjp_params's entry,
    a parameter with requires_grad=False keeps .grad None, the default call leaves every decoder .grad None; chained through
    model.latent an encoder weight's and a decoder kernel-MLP weight's gradient meet forward(query_coord_pos=...)'s at the bar;
  * timing keys (gno_bwd_nh*, the forward's, mlp2_bwd_f32_h256, no gno_adj*); nothing sized by Nq survives the call; refusals (four
    hidden layers, 'nonlinear', use_attn, a capture on a row route, a bad cotangent) leave the launch count unchanged.

Measured on an MI355X: against the oracle at most 2.5e-6 of the peak over the latent and every parameter, all strategies, chunkings
and shapes; chunkings at most 4.3e-7 of the peak apart; chained gradients 7.1e-7 (encoder weight), 4.8e-7 (decoder kernel-MLP weight)
and 1.6e-6 (projection weight) of the peak from forward's."""
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gaot_oracle as orc  # noqa: E402  (checker only)
import test_field_adjoint_gpu as fa  # noqa: E402  (the models, the cotangent, the latent)
import test_field_hessian_gpu as hb  # noqa: E402  (the model fixture, the watcher, check(), the bar, the queries)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32_BAR = hb.FP32_BAR
CHUNKS = (None, 250, 64)
WEIGHTING = "scale_weighting."
SHAPES = {
    "four_channels": ("knn", dict(out=4)),
    "two_scales_summed_bidirectional": ("bidirectional", dict(scales=[1.0, 2.0], use_scale_weights=False)),
    "two_scales_weighted_radius": ("radius", dict(out=2, scales=[1.0, 2.0], use_scale_weights=True)),
    "three_layers": ("knn", dict(out_gno_channel_mlp_hidden_layers=[64, 64, 64])),
    "three_layers_radius": ("radius", dict(out_gno_channel_mlp_hidden_layers=[64, 64, 64])),
    "projection_96_on_the_chain": ("knn", dict(out=2, projection_channels=96)),
}
_REFS = {}


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """Later tests that bound the rise of allocated memory (tests/test_gno_weighted_gpu.py) are sensitive to which blocks of torch's
    caching allocator they are served from.  The models this module adds to the shared fixture cache, its references and the
    workspaces and chunk tensors its calls left in the allocator's cache are handed back when the module is done."""
    import gc
    had = set(hb._MODELS)
    yield
    for key in set(hb._MODELS) - had:
        del hb._MODELS[key]
    _REFS.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _oracle(key, model, cfg, lat, q, g):
    """(grad of sum(g * decoder(latent)) with respect to the latent, {decoder parameter: its gradient}) by fp64 autograd of the oracle's
    decoder on the CPU, on the edges of the lists the streamed routes use; once per key.  A parameter the loss does not reach: zeros"""
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
    names = [n for n, _ in dec.named_parameters()]
    sd = {n: v.detach().double().cpu() for n, v in model.state_dict().items()}
    for n in names:
        sd["decoder." + n].requires_grad_(True)
    lat64 = lat.detach().double().cpu().requires_grad_(True)
    p = orc.magno_decoder(sd, cfg.magno, lat64, q.detach().double().cpu(), tok.double().cpu(), types.SimpleNamespace(**edges))
    leaves = [lat64] + [sd["decoder." + n] for n in names]
    grads = torch.autograd.grad((p * g.double().cpu()).sum(), leaves, allow_unused=True)
    grads = [torch.zeros_like(leaf) if gr is None else gr for leaf, gr in zip(leaves, grads)]
    _REFS[key] = (grads[0], dict(zip(names, grads[1:])))
    return _REFS[key]


def _check_all(tag, model, got_lat, got, ref_lat, ref, skip=()):
    names = [n for n, _ in model.decoder.named_parameters()]
    assert list(got) == names and set(ref) == set(names)
    assert got_lat.dtype == torch.float32 and not got_lat.requires_grad
    hb.check(f"{tag}/latent", got_lat, ref_lat)
    for n, p in model.decoder.named_parameters():
        assert got[n].shape == p.shape and got[n].dtype == torch.float32 and not got[n].requires_grad, n
        if not n.startswith(skip or "\0"):
            hb.check(f"{tag}/{n}", got[n], ref[n])


def _keys_ok(seen, rows):
    keys = seen["keys"]
    fwd = "gno_fwd_nh" if rows else "gno_fwd_knn_nh"
    return (any(k.startswith("gno_bwd_nh") for k in keys) and any(k.startswith(fwd) for k in keys) and "mlp2_bwd_f32_h256" in keys
            and not any(k.startswith("gno_adj") for k in keys))


@pytest.mark.parametrize("strategy", list(fa.MODELS))
def test_every_gradient_meets_the_oracle_at_every_chunking(strategy, monkeypatch):
    key, (model, batch, tokens, cfg) = fa._model(strategy)
    q = hb._queries(batch)
    lat = fa._latent(model, batch, tokens)
    g = fa._cotangent(q.shape[0], 1)
    ref_lat, ref = _oracle(key, model, cfg, lat, q, g)
    got = {}
    for chunk in CHUNKS:
        with hb._watch(monkeypatch) as seen:
            got[chunk] = model.sample_vjp_params(lat, q, g, chunk_points=chunk)
        assert _keys_ok(seen, strategy != "knn"), seen
        _check_all(f"sample_vjp_params/{strategy}/chunk{chunk}", model, *got[chunk], ref_lat, ref)
        again = model.sample_vjp_params(lat, q, g, chunk_points=chunk)                     # reproducible
        assert torch.equal(again[0], got[chunk][0]) and all(torch.equal(again[1][n], got[chunk][1][n]) for n in ref), chunk
    for chunk in CHUNKS[1:]:
        for n, a, b, r in [("latent", got[chunk][0], got[None][0], ref_lat)] + [(n, got[chunk][1][n], got[None][1][n], ref[n]) for n in ref]:
            d, peak = (a - b).abs().max().item(), r.abs().max().item()
            print(f"[chunking] sample_vjp_params/{strategy}/{n}: chunk {chunk} against one piece: {d / peak:.3e} of the peak {peak:.3e}")
            assert d <= 1e-5 * peak, (chunk, n, d, peak)
    with hb._precision("bf16"):
        b16 = model.sample_vjp_params(lat, q, g, chunk_points=250)                        # the same bits in both modes
    assert torch.equal(b16[0], got[250][0]) and all(torch.equal(b16[1][n], got[250][1][n]) for n in ref)
    # not sample_vjp's bits (another kernel, another order), but its values
    hb.check(f"sample_vjp_params/{strategy}/latent against sample_vjp", got[250][0], model.sample_vjp(lat, q, g, chunk_points=250).double().cpu())
    # a latent that requires grad: still outside autograd
    out, grads = model.sample_vjp_params(model.latent(batch, tokens), q[:100], g[:100].contiguous())
    assert not out.requires_grad and not any(t.requires_grad for t in grads.values())


@pytest.mark.parametrize("case", list(SHAPES))
def test_other_shapes_meet_the_oracle(case, monkeypatch):
    strategy, kw = SHAPES[case]
    kw = dict(kw)
    out = kw.pop("out", 1)
    key, (model, batch, tokens, cfg) = fa._model(strategy, out=out, **kw)
    q = hb._queries(batch, 150, 150)
    lat = fa._latent(model, batch, tokens)
    g = fa._cotangent(q.shape[0], out)
    ref_lat, ref = _oracle(key, model, cfg, lat, q, g)
    with hb._watch(monkeypatch) as seen:
        got_lat, got = model.sample_vjp_params(lat, q, g, chunk_points=128)
    chain = kw.get("projection_channels") == 96
    assert any(k.startswith("gno_bwd_nh") for k in seen["keys"]) and not any(k.startswith("gno_adj") for k in seen["keys"])
    assert ("mlp2_bwd_f32_h256" in seen["keys"]) == (not chain) and not (chain and any(k.startswith("mlp2_bwd_f32") for k in seen["keys"]))
    if "weighted" in case:
        assert any(n.startswith(WEIGHTING) for n in got)
    _check_all(f"sample_vjp_params/{case}", model, got_lat, got, ref_lat, ref)


def test_on_knn_the_scale_weighting_gradients_are_exact_zeros(monkeypatch):
    key, (model, batch, tokens, cfg) = fa._model("knn", out=2, scales=[1.0, 2.0], use_scale_weights=True)
    q = hb._queries(batch, 150, 150)
    lat = fa._latent(model, batch, tokens)
    g = fa._cotangent(q.shape[0], 2)
    ref_lat, ref = _oracle(key, model, cfg, lat, q, g)
    weighting = [n for n in ref if n.startswith(WEIGHTING)]
    assert len(weighting) == 4
    peak = ref["projection.fcs.0.weight"].abs().max().item()
    assert peak > 0
    for n in weighting:                                  # the fixture on the CPU first: sum_s w_s = 1 leaves rounding only
        assert ref[n].abs().max().item() <= 1e-12 * peak, (n, ref[n].abs().max().item(), peak)
    got_lat, got = model.sample_vjp_params(lat, q, g, chunk_points=128)
    for n in weighting:
        assert torch.equal(got[n], torch.zeros_like(got[n])), n
    _check_all("sample_vjp_params/two_scales_weighted_knn", model, got_lat, got, ref_lat, ref, skip=WEIGHTING)


@pytest.mark.parametrize("strategy", ["knn", "radius"])
def test_sample_autograd_params(strategy):
    key, (model, batch, tokens, cfg) = fa._model(strategy)
    q = hb._queries(batch)
    lat = fa._latent(model, batch, tokens)
    w = fa._cotangent(q.shape[0], 1, seed=17)
    params = dict(model.decoder.named_parameters())
    frozen = "gno.channel_mlp.fcs.1.bias"
    try:
        model.zero_grad(set_to_none=True)
        leaf = lat.clone().requires_grad_(True)
        base = model.sample_autograd(leaf, q, chunk_points=250)
        (base * w).sum().backward()
        assert leaf.grad is not None and all(p.grad is None for p in params.values())      # the default: the latent alone
        base_grad = leaf.grad.clone()
        assert torch.equal(base_grad, model.sample_vjp(lat, q, w, chunk_points=250))
        params[frozen].requires_grad_(False)
        want_lat, want = model.sample_vjp_params(lat, q, w, chunk_points=250)
        for mode in ("fp32", "bf16"):
            with hb._precision(mode):
                model.zero_grad(set_to_none=True)
                leaf = lat.clone().requires_grad_(True)
                pred = model.sample_autograd_params(leaf, q, chunk_points=250)
                assert pred.requires_grad and torch.equal(pred.detach(), base.detach()), mode
                (pred * w).sum().backward()
            assert torch.equal(leaf.grad, want_lat), mode
            for n, p in params.items():
                if n == frozen:
                    assert p.grad is None
                else:
                    assert p.grad is not None and torch.equal(p.grad, want[n]), (mode, n)
        # a latent that needs no gradient: the parameters alone
        model.zero_grad(set_to_none=True)
        pred = model.sample_autograd_params(lat, q, chunk_points=250)
        assert pred.requires_grad
        (pred * w).sum().backward()
        assert torch.equal(params["projection.fcs.0.weight"].grad, want["projection.fcs.0.weight"])
        # no decoder parameter requires grad: the existing node
        for p in params.values():
            p.requires_grad_(False)
        leaf = lat.clone().requires_grad_(True)
        pred = model.sample_autograd_params(leaf, q, chunk_points=250)
        assert type(pred.grad_fn).__name__.startswith("SampleLatentFn")
        (grad,) = torch.autograd.grad((pred * w).sum(), leaf)
        assert torch.equal(grad, base_grad)
        with pytest.raises(ValueError, match="query_pos requires grad"):
            model.sample_autograd_params(leaf, q.clone().requires_grad_(True))
    finally:
        for p in params.values():
            p.requires_grad_(True)
        model.zero_grad(set_to_none=True)


@pytest.mark.parametrize("strategy", ["knn", "bidirectional"])
def test_chained_through_the_latent_it_meets_the_route_it_replaces(strategy):
    """the loss sum(w * pred) reaches an encoder weight and a decoder kernel-MLP weight through sample_autograd_params +
    the autograd of model.latent, and through forward(query_coord_pos=q) -- edge list, decoder graph -- with the same values at the bar"""
    key, (model, batch, tokens, cfg) = fa._model(strategy)
    q = hb._queries(batch)
    w = fa._cotangent(q.shape[0], 1, seed=19)
    leaves = [model.encoder.gno.channel_mlp.fcs[0].weight, model.decoder.gno.channel_mlp.fcs[0].weight, model.decoder.projection.fcs[0].weight]
    model.decoder.precompute_edges = False
    try:
        p_ref = model(batch, tokens, query_coord_pos=q, query_coord_batch_idx=torch.zeros(q.shape[0], dtype=torch.long, device=DEV))
    finally:
        model.decoder.precompute_edges = True
    refs = torch.autograd.grad((p_ref * w).sum(), leaves)
    pred = model.sample_autograd_params(model.latent(batch, tokens), q, chunk_points=250)
    gots = torch.autograd.grad((pred * w).sum(), leaves)
    assert torch.allclose(pred.detach(), p_ref.detach(), rtol=1e-4, atol=1e-5)
    for name, got, ref in zip(("encoder_weight", "decoder_kernel_mlp_weight", "projection_weight"), gots, refs):
        hb.check(f"sample_autograd_params/{strategy}/{name}", got, ref.double().cpu())


@pytest.mark.parametrize("strategy", ["knn", "radius"])
def test_nothing_sized_by_the_queries_survives_the_call(strategy):
    key, (model, batch, tokens, cfg) = fa._model(strategy)
    gen = torch.Generator().manual_seed(23)
    q = (torch.rand(20000, 3, generator=gen) * 2.4 - 1.2).to(DEV)
    lat = fa._latent(model, batch, tokens)
    g = fa._cotangent(q.shape[0], 1)
    model.sample_vjp_params(lat, q[:2000].contiguous(), g[:2000].contiguous(), chunk_points=1000)      # the grid's description, the allocator
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    out, grads = model.sample_vjp_params(lat, q, g, chunk_points=4096)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - m0
    kept = sum((t.numel() * 4 + 511) // 512 * 512 for t in [out, *grads.values()])
    assert grown <= kept, (grown, kept)                                                # back to the start plus the results,
    sized = [lat.numel()] + [p.numel() for p in model.decoder.parameters()]             # none of which is sized by Nq
    assert kept == sum((n * 4 + 511) // 512 * 512 for n in sized)


REFUSALS = {
    "four_hidden_layers": ("knn", dict(out_gno_channel_mlp_hidden_layers=[64, 64, 64, 64]), "4 hidden layers"),
    "four_hidden_layers_radius": ("radius", dict(out_gno_channel_mlp_hidden_layers=[64, 64, 64, 64]), "4 hidden layers"),
    "nonlinear": ("knn", dict(out_gno_transform_type="nonlinear"), "'nonlinear'"),
    "use_attn": ("knn", dict(use_attn=True), "use_attn"),
    "use_attn_radius": ("radius", dict(use_attn=True), "on row lists.*use_attn"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_other_configurations_are_refused_before_any_launch(case):
    from gaot_3d_amd import ops
    strategy, kw, msg = REFUSALS[case]
    model, batch, tokens, cfg = hb._setup(f"param_adjoint/refuse/{case}", k=8, **fa.MODELS[strategy], **kw)
    lat = fa._latent(model, batch, tokens)
    q = batch.pos[:200].contiguous()
    g = fa._cotangent(200, 1)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    with pytest.raises(NotImplementedError, match=msg):
        model.sample_vjp_params(lat, q, g)
    with pytest.raises(NotImplementedError, match=msg):
        model.sample_autograd_params(lat.clone().requires_grad_(True), q)
    assert ops.launch_count() == n0


def test_a_bad_cotangent_and_a_capture_on_a_row_route_raise_before_any_launch():
    from gaot_3d_amd import ops
    from gaot_3d_amd._lib import GaotError
    key, (model, batch, tokens, cfg) = fa._model("bidirectional")
    q = batch.pos[:300].contiguous()
    lat = fa._latent(model, batch, tokens)
    g = fa._cotangent(300, 1)
    eager = model.sample_vjp_params(lat, q, g)                   # describes the grid, warms the allocator
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    for bad in (g.double(), g.cpu(), g[:50], torch.zeros(300, 2, device=DEV), torch.zeros(300, device=DEV)):
        with pytest.raises(ValueError, match="cotangent"):
            model.sample_vjp_params(lat, q, bad)
    with pytest.raises(ValueError, match="chunk_points"):
        model.sample_vjp_params(lat, q, g, chunk_points=0)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(GaotError, match="captured"):
        with torch.cuda.graph(graph):
            model.sample_vjp_params(lat, q, g)
    assert ops.launch_count() == n0
    torch.cuda.synchronize()
    again = model.sample_vjp_params(lat, q, g)
    assert torch.equal(again[0], eager[0]) and all(torch.equal(again[1][n], eager[1][n]) for n in eager[1])
