"""Second spatial derivatives of the sampled field: gaot_gno_fwd_knn_jet2 (the fused GNO forward on a regular k-neighbour list with a
directional 2-jet per direction), gaot_mlp2_jet2 (the projection's jets), IntegralTransform.jet2_knn, jet2_rows of the per-point
MLPs, MAGNODecoder / GAOT3D.sample_hessian and sample_laplacian.

The bar is the project's fp32 bar for coordinate derivatives (tests/test_coord_grad_gpu.py FP32_BAR: max error <= 1e-3 of the
reference's peak, cosine >= 0.99999), applied separately to d1, to d2, to the diagonal and to the off-diagonal entries of the
Hessian, each against its own peak (asserted > 0).  An fp32 emulation of the algorithm on the CPU sits 4e-7 .. 8e-7 of the peak from
fp64, three orders of magnitude inside the bar.

  * op level, GNO: Nq in {1, 7, 33, 1000} x k in {1 .. 32} x 1..4 hidden layers x the three transform types, 211 sources with
    repeats, nd in {1, 3, 6} generic directions (neither axis-aligned nor unit): one launch; value torch.equal to
    ops.gno_forward_knn(precision=0); with axis directions d1[d] torch.equal to ops.gno_forward_knn_jac's plane d; d1 and d2 against
    tests/gno_jet2_ref.py; a direction's planes torch.equal given alone, first of six or last of six; a zero direction gives zeros;
  * bad arguments raise GaotError with the launch count unchanged;
  * op level, projection: rows in {1, 31, 33, 129, 1000} x hidden in {64, 128, 256} x 1..4 outputs x 1..3 directions, with and
    without b2, saturated rows included: y and d1 torch.equal to ops.mlp2_jvp, d2 at the bar, zero planes give zeros, rows [a:b]
    of a larger call equal the call on that slice;
  * model level (4096 points, latent 8 x 8 x 8, k = 8, two layers, eval), 300 queries at the sample's points and 300 random ones
    partly outside the box, against the fp64 oracle's decoder on the edges of the ids knn_to_grid returned, differentiated twice on
    the CPU: hess at the bar and exactly symmetric, pred / jac torch.equal to sample_jacobian's, lap the ordered trace and at the
    bar, chunkings bit-identical, bf16 mode the fp32 bits, a four-channel model and a 'nonlinear' decoder, no CSR build / gno_bwd* /
    gno_fwd_knn* timing key; a captured sample_hessian replays to the eager result with new coordinates; refusals."""
import contextlib
import math
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gaot_oracle as orc  # noqa: E402  (checker only)
import gno_jet2_ref as REF  # noqa: E402
import parity as PAR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("linear", "nonlinear", "nonlinear_kernelonly")
KS = (1, 2, 4, 8, 16, 32)
NQS = (1, 7, 33, 1000)      # Nq * k below one 32-edge tile, ragged against it, and many workgroups
NSRC = 211
FP32_BAR = (1e-3, 0.99999)  # tests/test_coord_grad_gpu.py: max error relative to the reference's peak, cosine
AXES = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
GENERIC = ((0.3, -1.7, 0.9), (-2.1, 0.4, 0.6), (0.8, 0.5, -1.3), (1.9, 1.1, 0.2), (-0.4, -0.6, -2.2), (0.05, 2.4, -0.7))


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
    assert peak > 0, f"{name}: the reference is zero"
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


# ---- op level, GNO ----------------------------------------------------------------------------------------------------------------------
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
def test_gno_jets_value_tangent_and_second_derivative(nh, mode):
    from gaot_3d_amd import ops
    gen, y, f, ws, bs = _operands(nh, mode)
    yd, fd = y.to(DEV), f.to(DEV)
    wd, bd = [w.to(DEV) for w in ws], [b.to(DEV) for b in bs]
    t = None
    if mode != "linear":
        t = (f.double() @ ws[0][:, 6:].double().t()).float().to(DEV)       # the per-node term of layer 0, as the host layer forms it
        wd = [ws[0][:, :6].contiguous().to(DEV)] + wd[1:]
    fk = None if mode == "nonlinear_kernelonly" else fd
    worst = {"d1": [0.0, 1.0], "d2": [0.0, 1.0]}
    for qi, nq in enumerate(NQS):
        x = torch.rand(nq, 3, generator=gen) * 2 - 1
        xd = x.to(DEV)
        for ki, k in enumerate(KS):
            nd = (1, 3, 6)[(ki + qi) % 3]                # rotated with Nq: every k meets every nd
            nbr = torch.randint(0, NSRC, (nq * k,), generator=gen, dtype=torch.int32)        # repeats allowed
            nb = nbr.to(DEV)
            dirs = GENERIC[:nd]
            n0 = ops.launch_count()
            out, d1, d2 = ops.gno_forward_knn_jet2(mode, wd, bd, yd, xd, fk, t, nb, k, dirs)
            assert ops.launch_count() == n0 + 1                                              # ONE launch
            assert out.shape == (nq, 32) and d1.shape == d2.shape == (nd, nq, 32) and d1.is_contiguous() and d2.is_contiguous()
            val = ops.gno_forward_knn(mode, wd, bd, yd, xd, fk, t, nb, k, precision=0)
            assert torch.equal(out, val), (nq, k, (out - val).abs().max().item())
            # the reference evaluates the same fp32 operands (t is part of layer 0 there: W_0 with its feature columns)
            ro, r1, r2 = REF.gno_knn_jet2(ws, bs, y, x, nbr, k, f, mode, dirs)
            assert torch.allclose(out.cpu().double(), ro, rtol=1e-4, atol=1e-5), (nq, k)
            for name, got, ref in (("d1", d1, r1), ("d2", d2, r2)):
                rel, cos = check(f"gno_jet2_knn/{mode}/nh{nh}/nq{nq}/k{k}/nd{nd}/{name}", got, ref, quiet=True)
                worst[name] = [max(worst[name][0], rel), min(worst[name][1], cos)]
            # axis directions: the value again, and the tangent planes of the Jacobian kernel bit for bit
            oa, a1, a2 = ops.gno_forward_knn_jet2(mode, wd, bd, yd, xd, fk, t, nb, k, AXES)
            _, jac = ops.gno_forward_knn_jac(mode, wd, bd, yd, xd, fk, t, nb, k)
            assert torch.equal(oa, val)
            for d in range(3):
                assert torch.equal(a1[d], jac[d]), (nq, k, d, (a1[d] - jac[d]).abs().max().item())
            # a direction's planes do not depend on its company: alone, first of six, last of six; a zero direction gives zeros
            v = GENERIC[4]
            _, s1, s2 = ops.gno_forward_knn_jet2(mode, wd, bd, yd, xd, fk, t, nb, k, (v,))
            _, f1, f2 = ops.gno_forward_knn_jet2(mode, wd, bd, yd, xd, fk, t, nb, k, (v, AXES[0], (0.0, 0.0, 0.0), *GENERIC[:3]))
            _, l1, l2 = ops.gno_forward_knn_jet2(mode, wd, bd, yd, xd, fk, t, nb, k, (*GENERIC[:3], (0.0, 0.0, 0.0), AXES[2], v))
            assert torch.equal(s1[0], f1[0]) and torch.equal(s2[0], f2[0]), (nq, k)
            assert torch.equal(s1[0], l1[5]) and torch.equal(s2[0], l2[5]), (nq, k)
            assert torch.equal(f1[1], jac[0]) and torch.equal(l1[4], jac[2]) and torch.equal(f2[1], a2[0]) and torch.equal(l2[4], a2[2])
            for z in (f1[2], f2[2], l1[3], l2[3]):
                assert torch.equal(z, torch.zeros_like(z)), (nq, k)
    for name in ("d1", "d2"):
        print(f"[parity] gno_jet2_knn/{mode}/nh{nh}/{name}: worst rel_to_peak={worst[name][0]:.3e} worst cosine={worst[name][1]:.7f} over "
              f"{len(NQS) * len(KS)} shapes (bar {FP32_BAR[0]:.0e} / {FP32_BAR[1]})")


def test_gno_bad_arguments_raise_before_any_launch():
    from gaot_3d_amd import ops
    from gaot_3d_amd._lib import GaotError
    gen, y, f, ws, bs = _operands(2, "linear")
    yd, fd = y.to(DEV), f.to(DEV)
    wd, bd = [w.to(DEV) for w in ws], [b.to(DEV) for b in bs]
    nq = 40
    xd = (torch.rand(nq, 3, generator=gen) * 2 - 1).to(DEV)
    nbr = torch.zeros(nq * 8, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    with pytest.raises(GaotError, match="gaot_gno_fwd_knn_jet2: nd must be"):
        ops.gno_forward_knn_jet2("linear", wd, bd, yd, xd, fd, None, nbr, 8, ())
    assert ops.launch_count() == n0
    with pytest.raises(GaotError, match="gaot_gno_fwd_knn_jet2: nd must be"):
        ops.gno_forward_knn_jet2("linear", wd, bd, yd, xd, fd, None, nbr, 8, (*GENERIC, AXES[0]))
    assert ops.launch_count() == n0
    with pytest.raises(GaotError, match="gaot_gno_fwd_knn_jet2: k must be"):
        ops.gno_forward_knn_jet2("linear", wd, bd, yd, xd, fd, None, torch.zeros(nq * 3, dtype=torch.int32, device=DEV), 3, AXES)
    assert ops.launch_count() == n0
    with pytest.raises(GaotError, match="nbr must hold"):
        ops.gno_forward_knn_jet2("linear", wd, bd, yd, xd, fd, None, nbr[:-1], 8, AXES)
    assert ops.launch_count() == n0
    with pytest.raises(GaotError):
        ops.gno_forward_knn_jet2("linear", wd, bd, yd, xd.cpu(), fd, None, nbr, 8, AXES)
    assert ops.launch_count() == n0
    with pytest.raises(GaotError, match="host"):
        ops.gno_forward_knn_jet2("linear", wd, bd, yd, xd, fd, None, nbr, 8, torch.tensor(AXES, device=DEV))
    assert ops.launch_count() == n0
    ops.gno_forward_knn_jet2("linear", wd, bd, yd, xd, fd, None, nbr, 8, torch.tensor(AXES))   # a good call, directions as a CPU tensor
    assert ops.launch_count() == n0 + 1


# ---- op level, projection ---------------------------------------------------------------------------------------------------------------
ROWS = (1, 31, 33, 129, 1000)


@pytest.mark.parametrize("hidden", [64, 128, 256])
def test_projection_jets(hidden):
    from gaot_3d_amd import ops
    gen = torch.Generator().manual_seed(hidden)
    worst = [0.0, 1.0]
    for oc in (1, 2, 3, 4):
        w1 = torch.randn(hidden, 32, generator=gen) / math.sqrt(32)
        b1 = 0.1 * torch.randn(hidden, generator=gen)
        w2 = torch.randn(oc, hidden, generator=gen) / math.sqrt(hidden)
        b2 = 0.1 * torch.randn(oc, generator=gen)
        wd = [t.to(DEV) for t in (w1, b1, w2, b2)]
        for rows in ROWS:
            x = torch.randn(rows, 32, generator=gen)
            x[::3] *= 4.0                                                              # saturated rows: |z| up to 10 and beyond
            dxs = [torch.randn(rows, 32, generator=gen) for _ in range(3)]
            ddxs = [torch.randn(rows, 32, generator=gen) for _ in range(3)]
            xd, dd, ddd = x.to(DEV), [d.to(DEV) for d in dxs], [d.to(DEV) for d in ddxs]
            for nd in (1, 2, 3):
                for bias in (True, False):
                    b2d, b2c = (wd[3], b2) if bias else (None, None)
                    n0 = ops.launch_count()
                    y, d1, d2 = ops.mlp2_jet2(xd, dd[:nd], ddd[:nd], wd[0], wd[1], wd[2], b2d)
                    assert ops.launch_count() == n0 + 1
                    assert y.shape == (rows, oc) and d1.shape == d2.shape == (rows, oc, nd)
                    yv, jv = ops.mlp2_jvp(xd, dd[:nd], wd[0], wd[1], wd[2], b2d)
                    assert torch.equal(y, yv), (rows, oc, nd, bias)
                    assert torch.equal(d1, jv), (rows, oc, nd, bias, (d1 - jv).abs().max().item())
                    ry, r1, r2 = REF.mlp_jet2(w1, b1, w2, b2c, x, dxs[:nd], ddxs[:nd])
                    rel, cos = check(f"mlp2_jet2/h{hidden}/oc{oc}/rows{rows}/nd{nd}/d2", d2, r2, quiet=True)
                    worst = [max(worst[0], rel), min(worst[1], cos)]
            # without the value; zero planes; a slice of the rows
            yn, e1, e2 = ops.mlp2_jet2(xd, dd, ddd, wd[0], wd[1], wd[2], wd[3], store_y=False)
            assert yn is None and torch.equal(e1, d1) and torch.equal(e2, d2)
            zero = [torch.zeros_like(xd)] * 3
            _, z1, z2 = ops.mlp2_jet2(xd, zero, zero, wd[0], wd[1], wd[2], wd[3])
            assert torch.equal(z1, torch.zeros_like(z1)) and torch.equal(z2, torch.zeros_like(z2))
            if rows >= 129:
                a, b = 37, rows - 5
                ys, s1, s2 = ops.mlp2_jet2(xd[a:b], [d[a:b] for d in dd], [d[a:b] for d in ddd], wd[0], wd[1], wd[2], wd[3])
                yf, _, _ = ops.mlp2_jet2(xd, dd, ddd, wd[0], wd[1], wd[2], wd[3])
                assert torch.equal(ys, yf[a:b]) and torch.equal(s1, d1[a:b]) and torch.equal(s2, d2[a:b]), rows
    print(f"[parity] mlp2_jet2/h{hidden}/d2: worst rel_to_peak={worst[0]:.3e} worst cosine={worst[1]:.7f} (bar {FP32_BAR[0]:.0e} / {FP32_BAR[1]})")


@pytest.mark.parametrize("kind", ["linear", "channel"])
def test_jet2_rows_six_directions_and_refusal(kind):
    from gaot_3d_amd.model.layers.mlp import ChannelMLP, LinearChannelMLP
    torch.manual_seed(5)
    mlp = (LinearChannelMLP([32, 256, 4]) if kind == "linear" else ChannelMLP(32, 4, 256, n_layers=2)).to(DEV).eval()
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(333, 32, generator=gen).to(DEV)
    dxs = [torch.randn(333, 32, generator=gen).to(DEV) for _ in range(6)]
    ddxs = [torch.randn(333, 32, generator=gen).to(DEV) for _ in range(6)]
    y, d1, d2 = mlp.jet2_rows(x, dxs, ddxs)
    assert y.shape == (333, 4) and d1.shape == d2.shape == (333, 4, 6) and not d2.requires_grad
    yv, jv = mlp.jvp_rows(x, dxs[:3])
    yw, jw = mlp.jvp_rows(x, dxs[3:])
    assert torch.equal(y, yv) and all(torch.equal(d1[:, :, d], (jv + jw)[d]) for d in range(6))
    w = [(fc.weight[:, :, 0] if fc.weight.dim() == 3 else fc.weight).detach().cpu() for fc in mlp.fcs]
    b = [fc.bias.detach().cpu() for fc in mlp.fcs]
    _, _, r2 = REF.mlp_jet2(w[0], b[0], w[1], b[1], x.cpu(), [d.cpu() for d in dxs], [d.cpu() for d in ddxs])
    check(f"jet2_rows/{kind}/d2", d2, r2)
    other = (LinearChannelMLP([32, 96, 4]) if kind == "linear" else ChannelMLP(32, 4, 96, n_layers=2)).to(DEV).eval()
    with pytest.raises(NotImplementedError):
        other.jet2_rows(x, dxs[:3], ddxs[:3])


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
    _MODELS[key] = (model, bd, td, cfg)
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
    return (any(k.startswith("gno_jet2_knn") for k in keys) and any(k.startswith("mlp2_jet2") for k in keys) and seen["csr"] == 0
            and not any(k.startswith("csr_build") or k.startswith("gno_bwd") or k.startswith("gno_fwd_knn") for k in keys))


def _queries(batch, n_points=300, n_random=300):
    gen = torch.Generator().manual_seed(7)
    rnd = (torch.rand(n_random, 3, generator=gen) * 2.4 - 1.2).to(DEV)                  # some of them outside the grid's box
    return torch.cat([batch.pos[:n_points], rnd]).contiguous()


_REFS = {}


def _oracle_hessian(key, model, cfg, lat, q):
    """(pred [Nq, out], jac [Nq, out, 3], hess [Nq, out, 3, 3]) of the fp64 oracle's decoder on the CPU, its edges built from the ids
    knn_to_grid returned for these queries (the same lists), differentiated twice; computed once per (model, query set) and shared"""
    if key in _REFS:
        return _REFS[key]
    from gaot_3d_amd import graph as device_graph
    k = int(model.decoder.k_neighbors)
    tok = model._tokens(1, q.device, None, None)[0]
    with torch.no_grad():                 # the plan of the forward alone, as the sampling calls ask for it
        grid = model.decoder._stream_grid(lat, q, tok)
    assert grid is not None
    ids = device_graph.knn_to_grid(q, grid, k).reshape(-1).long().cpu()
    ei = torch.stack([ids, torch.arange(q.shape[0]).repeat_interleave(k)])
    ns = types.SimpleNamespace(**{f"decoder_edge_index_s{si}": ei for si in range(len(cfg.magno.scales))})
    sd = {n: v.detach().double().cpu() for n, v in model.state_dict().items()}
    lat64, tok64 = lat.detach().double().cpu(), tok.double().cpu()
    xg = q.detach().double().cpu().requires_grad_(True)
    p = orc.magno_decoder(sd, cfg.magno, lat64, xg, tok64, ns)
    oc = p.shape[1]
    jac, hess = torch.zeros(q.shape[0], oc, 3, dtype=torch.float64), torch.zeros(q.shape[0], oc, 3, 3, dtype=torch.float64)
    for o in range(oc):
        (g,) = torch.autograd.grad(p[:, o].sum(), xg, create_graph=True)
        jac[:, o] = g.detach()
        for i in range(3):
            (gg,) = torch.autograd.grad(g[:, i].sum(), xg, retain_graph=True)
            hess[:, o, i] = gg
    _REFS[key] = (p.detach(), jac, hess)
    return _REFS[key]


def _check_hessian(name, hess, ref_h):
    i3 = torch.arange(3)
    off = ~torch.eye(3, dtype=torch.bool)
    check(f"{name}/hess_diagonal", hess[:, :, i3, i3], ref_h[:, :, i3, i3])
    check(f"{name}/hess_off_diagonal", hess[:, :, off], ref_h[:, :, off])


def test_sample_hessian_and_laplacian_against_the_oracle(monkeypatch):
    model, batch, tokens, cfg = _setup()
    q = _queries(batch)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    ref_p, ref_j, ref_h = _oracle_hessian("cfg0", model, cfg, lat, q)
    with _watch(monkeypatch) as seen:
        pred, jac, hess = model.sample_hessian(lat, q)
        pl, lap = model.sample_laplacian(lat, q)
    assert _streamed(seen), seen
    assert pred.shape == (600, 1) and jac.shape == (600, 1, 3) and hess.shape == (600, 1, 3, 3) and lap.shape == (600, 1)
    for t in (pred, jac, hess, pl, lap):
        assert not t.requires_grad and t.grad_fn is None
    pj, jj = model.sample_jacobian(lat, q)
    assert torch.equal(pred, pj) and torch.equal(jac, jj) and torch.equal(pl, pj)
    assert torch.allclose(pred.cpu().double(), ref_p, rtol=1e-4, atol=1e-5)
    check("sample_hessian/jac", jac, ref_j)
    _check_hessian("sample_hessian", hess, ref_h)
    for i in range(3):
        for j in range(i):
            assert torch.equal(hess[..., i, j], hess[..., j, i]), (i, j)
    assert torch.equal(lap, hess[..., 0, 0] + hess[..., 1, 1] + hess[..., 2, 2])
    check("sample_laplacian", lap, ref_h[..., 0, 0] + ref_h[..., 1, 1] + ref_h[..., 2, 2])
    # a latent that requires grad still gives results outside autograd
    lat_g = model.latent(batch, tokens)
    assert lat_g.requires_grad
    assert not any(t.requires_grad for t in model.sample_hessian(lat_g, q[:100]))


def test_chunkings_and_bf16_mode_are_bit_identical():
    model, batch, tokens, cfg = _setup()
    q = _queries(batch, 1000, 2000)
    with torch.no_grad():
        lat = model.latent(batch, tokens)               # ONE fp32 latent tensor for both modes
    whole = model.sample_hessian(lat, q)
    lap = model.sample_laplacian(lat, q)
    for chunk in (700, 1500):
        for a, b in zip(model.sample_hessian(lat, q, chunk_points=chunk), whole):
            assert torch.equal(a, b), chunk
        for a, b in zip(model.sample_laplacian(lat, q, chunk_points=chunk), lap):
            assert torch.equal(a, b), chunk
    with _precision("bf16"):
        hb = model.sample_hessian(lat, q, chunk_points=700)
        lb = model.sample_laplacian(lat, q, chunk_points=700)
    assert all(torch.equal(a, b) for a, b in zip(hb, whole)) and all(torch.equal(a, b) for a, b in zip(lb, lap))


SHAPES = {
    "four_channels": dict(out=4),
    "nonlinear": dict(out_gno_transform_type="nonlinear"),
    "two_scales": dict(out=2, scales=[1.0, 2.0], use_scale_weights=True),
    "four_layers": dict(out_gno_channel_mlp_hidden_layers=[64, 64, 64, 64]),
}


@pytest.mark.parametrize("case", list(SHAPES))
def test_other_models_stream(case, monkeypatch):
    model, batch, tokens, cfg = _setup("shape/" + case, **SHAPES[case])
    q = _queries(batch, 0, 300)
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    ref_p, ref_j, ref_h = _oracle_hessian("shape/" + case, model, cfg, lat, q)
    with _watch(monkeypatch) as seen:
        pred, jac, hess = model.sample_hessian(lat, q, chunk_points=128)
        _, lap = model.sample_laplacian(lat, q, chunk_points=128)
    assert _streamed(seen), seen
    pj, jj = model.sample_jacobian(lat, q)
    assert torch.equal(pred, pj) and torch.equal(jac, jj)
    _check_hessian(f"sample_hessian/{case}", hess, ref_h)
    assert torch.equal(lap, hess[..., 0, 0] + hess[..., 1, 1] + hess[..., 2, 2])


REFUSALS = {
    "radius": dict(neighbor_strategy=["knn", "radius"], gno_radius=0.45),
    "bidirectional": dict(neighbor_strategy="bidirectional", gno_radius=0.45),
    "use_attn": dict(use_attn=True),
    "geoembed": dict(use_geoembed=[True, True], embedding_method="pointnet"),
    "k3": dict(k=3),
    "projection96": dict(projection_channels=96),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_other_configurations_are_refused(case):
    from gaot_3d_amd import ops
    model, batch, tokens, cfg = _setup("refuse/" + case, **REFUSALS[case])
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    torch.cuda.synchronize()
    for method in (model.sample_hessian, model.sample_laplacian):
        n0 = ops.launch_count()
        with pytest.raises(NotImplementedError, match="second derivatives"):
            method(lat, batch.pos[:200])
        assert ops.launch_count() == n0


def test_reverse_and_chunk_points_raise_value_errors():
    model, batch, tokens, cfg = _setup()
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    for method in (model.sample_hessian, model.sample_laplacian):
        with pytest.raises(ValueError, match="chunk_points"):
            method(lat, batch.pos[:100], chunk_points=0)
        model.decoder.decoder_strategy = "reverse"
        try:
            with pytest.raises(ValueError, match="reverse"):
                method(lat, batch.pos[:100])
        finally:
            model.decoder.decoder_strategy = "knn"


# ---- graph replay -----------------------------------------------------------------------------------------------------------------------
def test_sample_hessian_graph_replay_equals_eager():
    model, batch, tokens, cfg = _setup()
    qs = _queries(batch, 1500, 1500)
    q1, q2 = qs[:1500].contiguous(), qs[1500:].contiguous()
    with torch.no_grad():
        lat = model.latent(batch, tokens)
    buf = q1.clone()
    e1 = model.sample_hessian(lat, buf, chunk_points=600)          # the eager call: describes the grid, warms the allocator
    e2 = model.sample_hessian(lat, q2, chunk_points=600)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model.sample_hessian(lat, buf, chunk_points=600)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, e1))
    buf.copy_(q2)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, e2))
    assert not torch.equal(e1[2], e2[2])
