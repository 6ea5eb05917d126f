"""Sampling the decoded field at arbitrary points without an edge list: gaot_gno_fwd_knn (the fused GNO forward on the regular
k-neighbour list that gaot_knn_grid writes), IntegralTransform.forward_knn, MAGNODecoder.sample, GAOT3D.latent / GAOT3D.sample.

  * op level: on random coordinates, weights and neighbour ids (repeats allowed), Nq in {1, 7, 33, 1000} x k in {1 .. 32} x 1..4
    hidden layers x the three transform types x fp32 / bf16, ops.gno_forward_knn is torch.equal to ops.gno_forward /
    ops.gno_nl_forward on ops.build_graph of the same lists, and in fp32 mode within rtol 1e-4 / atol 1e-5 of the oracle;
  * bad arguments (k = 3, a null pointer, hidden width 128) raise GaotError before any launch;
  * model level (4096 points, latent 8 x 8 x 8, k = 8, two layers, eval): sample(latent(batch), batch.pos) against forward under
    no_grad, for chunk_points None / 1000 / 64, both precisions, at the bounds of tests/test_model_gpu.py (fp32 rtol 1e-4 / atol
    1e-5; bf16 2e-2 of the peak, relative L2 1e-2); the decoder call runs gno_fwd_knn* and neither a CSR build nor gno_fwd_nh*;
  * queries that are not the sample's points (random points partly outside the grid's box, all grid nodes and all cell centres,
    where distances tie) against forward(query_coord_pos=...) with edges built on the device;
  * the other transform types and shapes stream too; radius / use_attn / GeoEmbed / k = 3 decoders fall back and agree with forward;
    reverse raises; the result never requires grad;
  * memory: the peak rise of sample stays under the result + two chunks' ids, GNO rows and predictions + 4 MiB, and the existing
    no_grad route measured beside it needs at least four times that;
  * sample captured in a hipGraph replays, with new coordinates in the captured buffer, to the eager result bit for bit."""
import contextlib
import ctypes as C
import math
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import gaot_oracle as orc  # noqa: E402  (checker only)
import parity as PAR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("linear", "nonlinear", "nonlinear_kernelonly")
KS = (1, 2, 4, 8, 16, 32)
NQS = (1, 7, 33, 1000)      # Nq * k below the 64-edge macro tile, ragged against it, and many workgroups
NSRC = 211


def close(name, a, b, rtol, atol):
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    err = (a - b).abs().max().item() if a.numel() else 0.0
    print(f"[parity] {name}: max_abs={err:.3e} ref_peak={b.abs().max().item() if b.numel() else 0:.3e}")
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"{name}: max abs err {err:.3e}"


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
    """one source set and kernel MLP per (n_hidden, mode), on the CPU; the device copies are made by the caller"""
    gen = torch.Generator().manual_seed(100 * nh + MODES.index(mode))
    y = torch.rand(NSRC, 3, generator=gen) * 2 - 1
    f = torch.randn(NSRC, 32, generator=gen)
    ws, bs = _mlp(nh, mode, gen)
    return gen, y, f, ws, bs


def _oracle(ws, bs, y, x, ei, f, mode):
    sd = {}
    for l, (w, b) in enumerate(zip(ws, bs)):
        sd[f"channel_mlp.fcs.{l}.weight"] = w.double()
        sd[f"channel_mlp.fcs.{l}.bias"] = b.double()
    return orc.integral_transform(sd, "", y.double(), x.double(), ei.long(), f.double(), mode, False, 3)


@pytest.mark.parametrize("precision", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nh", [1, 2, 3, 4])
def test_knn_forward_is_the_graph_forward_bit_for_bit(nh, mode, precision):
    from gaot_3d_amd import ops
    gen, y, f, ws, bs = _operands(nh, mode)
    yd, fd = y.to(DEV), f.to(DEV)
    wd, bd = [w.to(DEV) for w in ws], [b.to(DEV) for b in bs]
    t = None
    if mode != "linear":
        t = (f.double() @ ws[0][:, 6:].double().t()).float().to(DEV)       # the per-node term of layer 0, as the host layer forms it
        wd = [ws[0][:, :6].contiguous().to(DEV)] + wd[1:]
    fk = None if mode == "nonlinear_kernelonly" else fd
    worst = 0.0
    for nq in NQS:
        x = torch.rand(nq, 3, generator=gen) * 2 - 1
        xd = x.to(DEV)
        for k in KS:
            nbr = torch.randint(0, NSRC, (nq * k,), generator=gen, dtype=torch.int32)        # repeats allowed
            ei = torch.stack([nbr, torch.arange(nq, dtype=torch.int32).repeat_interleave(k)])
            g = ops.build_graph(ei.to(DEV), NSRC, nq)
            if mode == "linear":
                ref = ops.gno_forward(wd, bd, yd, xd, fd, g, precision=precision)
            else:
                ref = ops.gno_nl_forward(mode, wd, bd, yd, xd, fk, t, g, precision=precision)
            got = ops.gno_forward_knn(mode, wd, bd, yd, xd, fk, t, nbr.to(DEV), k, precision=precision)
            assert got.shape == (nq, 32)
            assert torch.equal(got, ref), (nq, k, (got - ref).abs().max().item())
            if precision == 0:
                o = _oracle(ws, bs, y, x, ei, f, mode).float()
                worst = max(worst, (got.cpu() - o).abs().max().item())
                assert torch.allclose(got.cpu(), o, rtol=1e-4, atol=1e-5), (nq, k, (got.cpu() - o).abs().max().item())
    if precision == 0:
        print(f"[parity] gno_fwd_knn/{mode}/nh{nh}: max_abs={worst:.3e} against the oracle over {len(NQS) * len(KS)} shapes")


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
    with pytest.raises(GaotError, match="k must be"):
        ops.gno_forward_knn("linear", wd, bd, yd, xd, fd, None, torch.zeros(nq * 3, dtype=torch.int32, device=DEV), 3)
    assert ops.launch_count() == n0
    w128, b128 = _mlp(2, "linear", gen, hidden=128)
    with pytest.raises(GaotError, match="unsupported MLP shape"):
        ops.gno_forward_knn("linear", [w.to(DEV) for w in w128], [b.to(DEV) for b in b128], yd, xd, fd, None,
                            torch.zeros(nq * 8, dtype=torch.int32, device=DEV), 8)
    assert ops.launch_count() == n0
    m, keep = ops._mlp_struct(wd, bd)
    nbr = torch.zeros(nq * 8, dtype=torch.int32, device=DEV)
    out = torch.empty(nq, 32, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)
    for args in ((null, ptr(xd), ptr(fd), null, ptr(nbr)), (ptr(yd), ptr(xd), null, null, ptr(nbr)),
                 (ptr(yd), ptr(xd), ptr(fd), null, null)):
        with pytest.raises(GaotError, match="null pointer"):
            _lib.check(lib.gaot_gno_fwd_knn(C.byref(m), 0, *args, 8, nq, ptr(out), 0, null), "gaot_gno_fwd_knn")
        assert ops.launch_count() == n0
    with pytest.raises(GaotError, match="null src_table"):
        _lib.check(lib.gaot_gno_fwd_knn(C.byref(m), 1, ptr(yd), ptr(xd), ptr(fd), null, ptr(nbr), 8, nq, ptr(out), 0, null),
                   "gaot_gno_fwd_knn")
    with pytest.raises(GaotError, match="beyond int32"):
        _lib.check(lib.gaot_gno_fwd_knn(C.byref(m), 0, ptr(yd), ptr(xd), ptr(fd), null, ptr(nbr), 8, 1 << 28, ptr(out), 0, null),
                   "gaot_gno_fwd_knn")
    assert ops.launch_count() == n0
    ops.gno_forward_knn("linear", wd, bd, yd, xd, fd, None, nbr, 8)            # and a good call is ONE launch
    assert ops.launch_count() == n0 + 1


# ---- model level ------------------------------------------------------------------------------------------------------------------------
NPTS, LATENT = 4096, (8, 8, 8)
_MODELS = {}


def _setup(key="cfg0", k=8, **magno):
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
    model = init_model(3, 1, "gaot_3d", cfg)
    batch, tokens = make_synthetic_sample(NPTS, LATENT, k=k, in_normals=False, surface=False, seed=0)
    # an untrained model predicts O(1e-2): rescale its last affine map so that predictions are O(1) and the absolute bound bites
    model = model.to(DEV).eval()
    bd, td = batch.to(DEV), tokens.to(DEV)
    with torch.no_grad():
        p0 = model(bd, td)
        last = model.decoder.projection.fcs[-1]
        PAR.unit_scale_last_layer(last.weight, last.bias, float(p0.std()))
    _MODELS[key] = (model, bd, td)
    return _MODELS[key]


def _agree(name, got, ref, precision):
    d = (got - ref).abs().max().item() if got.numel() else 0.0
    print(f"[parity] {name}: max|sample - forward| = {d:.3e}")
    if precision == "fp32":
        close(name, got, ref, 1e-4, 1e-5)
    else:
        PAR.close_peak(name, got, ref, 2e-2, rel_l2=1e-2)


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
    return (any(k.startswith("gno_fwd_knn") for k in keys) and seen["csr"] == 0
            and not any(k.startswith("csr_build") or k.startswith("gno_fwd_nh") or k.startswith("gno_fwd_nl") for k in keys))


def _forward_at(model, batch, tokens, q):
    """forward's own route to predictions at other points: edges built on the device for the queries"""
    model.decoder.precompute_edges = False
    try:
        return model(batch, tokens, query_coord_pos=q, query_coord_batch_idx=torch.zeros(q.shape[0], dtype=torch.long, device=q.device))
    finally:
        model.decoder.precompute_edges = True


@pytest.mark.parametrize("chunk", [None, 1000, 64])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_sample_at_the_samples_points_equals_forward(precision, chunk, monkeypatch):
    """Zero is the expected difference wherever the batch's precomputed lists (knn_edges_grid on the host) order a point's tokens as
    gaot_knn_grid does; the row kernels behind the GNO (scale mix, projection) compute every row on its own, so neither the chunk
    size nor a row's place in a launch enters."""
    model, batch, tokens = _setup()
    with _precision(precision), torch.no_grad():
        ref = model(batch, tokens)
        lat = model.latent(batch, tokens)
        with _watch(monkeypatch) as seen:
            got = model.sample(lat, batch.pos, chunk_points=chunk)
        whole = model.sample(lat, batch.pos)
    assert got.shape == ref.shape and not got.requires_grad
    print(f"[parity] sample/{precision}/chunk{chunk}: max|chunked - one pass| = {(got - whole).abs().max().item():.3e}")
    _agree(f"sample/{precision}/chunk{chunk}", got, ref, precision)
    assert _streamed(seen), seen


def _other_queries():
    gen = torch.Generator().manual_seed(7)
    rnd = torch.rand(3000, 3, generator=gen) * 2.4 - 1.2                          # some of them outside the grid's box
    ax = [torch.linspace(-1, 1, n) for n in LATENT]
    nodes = torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1).reshape(-1, 3)
    mid = [(a[1:] + a[:-1]) / 2 for a in ax]
    centres = torch.stack(torch.meshgrid(*mid, indexing="ij"), dim=-1).reshape(-1, 3)   # eight equidistant tokens each
    return {"random": rnd, "nodes": nodes, "centres": centres}


@pytest.mark.parametrize("which", ["random", "nodes", "centres"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_sample_at_other_points_equals_forward_with_device_edges(precision, which, monkeypatch):
    model, batch, tokens = _setup()
    q = _other_queries()[which].to(DEV)
    with _precision(precision), torch.no_grad():
        ref = _forward_at(model, batch, tokens, q)
        lat = model.latent(batch, tokens)
        with _watch(monkeypatch) as seen:
            got = model.sample(lat, q, chunk_points=1000)
    assert got.shape == (q.shape[0], 1)
    _agree(f"sample_at/{which}/{precision}", got, ref, precision)
    assert _streamed(seen), seen


@pytest.mark.parametrize("channels", [16, 48])
@pytest.mark.parametrize("tt", ["nonlinear", "nonlinear_kernelonly"])
def test_other_transform_types_and_shapes_stream(tt, channels, monkeypatch):
    model, batch, tokens = _setup(f"{tt}/{channels}", out_gno_transform_type=tt, lifting_channels=channels,
                                  out_gno_channel_mlp_hidden_layers=[32, 32])
    for precision in ("fp32", "bf16"):
        with _precision(precision), torch.no_grad():
            ref = model(batch, tokens)
            lat = model.latent(batch, tokens)
            with _watch(monkeypatch) as seen:
                got = model.sample(lat, batch.pos, chunk_points=1500)
        _agree(f"sample/{tt}/c{channels}/{precision}", got, ref, precision)
        assert _streamed(seen), seen


FALLBACKS = {
    "radius": dict(neighbor_strategy=["knn", "radius"], gno_radius=0.45),
    "use_attn": dict(use_attn=True),
    "geoembed": dict(use_geoembed=[True, True]),
    "k3": dict(),
}


@pytest.mark.parametrize("case", list(FALLBACKS))
def test_fallbacks_equal_forward(case, monkeypatch):
    model, batch, tokens = _setup("fallback/" + case, k=3 if case == "k3" else 8, **FALLBACKS[case])
    q = _other_queries()["random"][:1500].to(DEV)
    for precision in ("fp32", "bf16"):
        with _precision(precision):
            with torch.no_grad():
                ref = _forward_at(model, batch, tokens, q)
                lat = model.latent(batch, tokens)
            with _watch(monkeypatch) as seen:
                got = model.sample(lat, q, chunk_points=700)
            # a latent that requires grad (its Transformer blocks run the fused row-block kernels, whose 1/rms differs from the no_grad
            # chain in the last bit: not compared) still gives a result outside autograd
            lat_g = model.latent(batch, tokens)
            assert lat_g.requires_grad
            out_g = model.sample(lat_g, q[:300], chunk_points=700)
            assert not out_g.requires_grad and out_g.grad_fn is None
        assert not got.requires_grad and got.grad_fn is None
        _agree(f"sample_fallback/{case}/{precision}", got, ref, precision)
        assert not any(k.startswith("gno_fwd_knn") for k in seen["keys"]), seen


def test_reverse_raises_and_result_never_requires_grad():
    model, batch, tokens = _setup()
    lat = model.latent(batch, tokens)
    assert lat.requires_grad
    out = model.sample(lat, batch.pos[:100])
    assert not out.requires_grad and out.grad_fn is None
    model.decoder.decoder_strategy = "reverse"
    try:
        with pytest.raises(ValueError, match="reverse"):
            model.sample(lat, batch.pos[:100])
    finally:
        model.decoder.decoder_strategy = "knn"


# ---- memory -----------------------------------------------------------------------------------------------------------------------------
MEM_NQ, MEM_CHUNK, MEM_K, MEM_OUT = 200003, 16384, 8, 1


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


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_sample_memory_is_the_result_and_two_chunks(precision):
    """the terms of the bound: the result, the chunk's ids, its GNO rows and its predictions; the factor 2 and the 4 MiB cover the
    allocator's rounding.  Route (a) -- neighbour strategy, build_graph, decoder under no_grad -- is measured beside it: it must need
    at least four times the bound, or the test measures nothing."""
    model, batch, tokens = _setup()
    gen = torch.Generator().manual_seed(11)
    q = (torch.rand(MEM_NQ, 3, generator=gen) * 2 - 1).to(DEV)
    bound = 4 * MEM_NQ * MEM_OUT + 2 * MEM_CHUNK * (4 * MEM_K + 4 * 32 + 4 * MEM_OUT) + 4 * 2**20
    with _precision(precision), torch.no_grad():
        lat = model.latent(batch, tokens)
        dec = model.decoder
        zeros_q = torch.zeros(MEM_NQ, dtype=torch.long, device=DEV)
        zeros_t = torch.zeros(tokens.shape[0], dtype=torch.long, device=DEV)
        b = _rise(lambda: model.sample(lat, q, chunk_points=MEM_CHUNK))
        a = _rise(lambda: dec._decode(lat, q, zeros_q, tokens, zeros_t, None, False))
    print(f"[memory] {precision}: sample {b / 2**20:.2f} MiB, no_grad forward route {a / 2**20:.2f} MiB, bound {bound / 2**20:.2f} MiB")
    assert b <= bound, (b, bound)
    assert a >= 4 * bound, (a, bound)


# ---- graph replay -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_sample_graph_replay_equals_eager(precision):
    model, batch, tokens = _setup()
    qs = _other_queries()["random"].to(DEV)
    q1, q2 = qs[:1500].contiguous(), qs[1500:].contiguous()
    with _precision(precision), torch.no_grad():
        lat = model.latent(batch, tokens)
        buf = q1.clone()
        eager1 = model.sample(lat, buf, chunk_points=600)          # the eager call: describes the grid, warms the allocator
        eager2 = model.sample(lat, q2, chunk_points=600)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = model.sample(lat, buf, chunk_points=600)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager1)
        buf.copy_(q2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager2)
        assert not torch.equal(eager1, eager2)
