"""CPU: the second-derivative interface of the sampled field is in place -- gaot_gno_fwd_knn_jet2, gaot_mlp2_jet2_supported and
gaot_mlp2_jet2 are declared in the header, bound in _lib.SIGNATURES with the header's argument counts and exported by the library,
with the ABI still version 11; none of the jet kernels of the built library uses scratch; the host layers exist with their signatures; the argument rules that need no device raise on the
host; and the closed-form references the GPU tests compare against (tests/gno_jet2_ref.py) equal fp64 autograd DOUBLE backward
(create_graph=True) through the oracle's integral transform and through a GELU MLP, saturated rows included.  (The kernels
themselves are covered by tests/test_field_hessian_gpu.py.)"""
import inspect
import math
import os
import re
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gaot_oracle as orc  # noqa: E402  (checker only)
import gno_jet2_ref as REF  # noqa: E402

SYMBOLS = {"gaot_gno_fwd_knn_jet2": 15, "gaot_mlp2_jet2_supported": 5, "gaot_mlp2_jet2": 24}
MODES = ("linear", "nonlinear", "nonlinear_kernelonly")


@pytest.mark.parametrize("name", list(SYMBOLS))
def test_symbols_declared_bound_and_exported(name):
    from gaot_3d_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gaot3d_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
    assert m, f"{name} is not declared in include/gaot3d_hip.h"
    assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == SYMBOLS[name], f"{name}: header and SIGNATURES disagree"
    assert hasattr(lib, name), f"{name} is not exported by libgaot3d_hip.so"
    assert lib.gaot_abi_version() == 11


def _kernel_scratch_sizes(path):
    """{kernel name: private_segment_fixed_size} from the code-object metadata (msgpack) embedded in the built library: the
    alphabetically ordered kernel maps hold `.name` before `.private_segment_fixed_size`"""
    blob = open(path, "rb").read()

    def mp_int(i):
        t = blob[i]
        if t < 0x80:
            return t
        return int.from_bytes(blob[i + 1:i + 1 + {0xcc: 1, 0xcd: 2, 0xce: 4, 0xcf: 8}[t]], "big")

    def mp_str(i):
        t = blob[i]
        if t in (0xd9, 0xda, 0xdb):
            w = {0xd9: 1, 0xda: 2, 0xdb: 4}[t]
            n = int.from_bytes(blob[i + 1:i + 1 + w], "big")
            return blob[i + 1 + w:i + 1 + w + n].decode()
        return blob[i + 1:i + 1 + (t & 0x1f)].decode()

    sizes = {}
    for m in re.finditer(rb"\.private_segment_fixed_size", blob):
        sizes[mp_str(blob.rfind(b".name", 0, m.start()) + 5)] = mp_int(m.end())
    return sizes


def test_jet_kernels_have_no_scratch():
    """the hard condition of the jet kernels, checked on the library as built: at three and four hidden layers it rests on the
    recomputation of gelu' / gelu'' staying inside the direction loop (gno_jet2.hip: opaque), which a compiler may undo silently"""
    from gaot_3d_amd import _lib
    lib = _lib.load()
    sizes = _kernel_scratch_sizes(lib._name)
    gno = {k: v for k, v in sizes.items() if "k_gno_fwd_knn_jet2" in k}
    mlp = {k: v for k, v in sizes.items() if "k_mlp2_jet2" in k}
    assert len(gno) == 12 and len(mlp) == 9, (sorted(gno), sorted(mlp))
    assert not any(gno.values()) and not any(mlp.values()), {k: v for k, v in {**gno, **mlp}.items() if v}
    assert any(sizes.values())           # the reader does see a kernel that uses scratch when there is one


def test_supported_accepts_exactly_the_family():
    from gaot_3d_amd import ops
    gelu = ops.ACT["gelu"]
    for in_dim in (16, 32, 64):
        for hidden in (32, 64, 96, 128, 256, 512):
            for oc in (0, 1, 2, 3, 4, 5):
                for nd in (0, 1, 2, 3, 4):
                    for act in (gelu, ops.ACT["relu"]):
                        want = in_dim == 32 and hidden in (64, 128, 256) and 1 <= oc <= 4 and 1 <= nd <= 3 and act == gelu
                        assert ops.mlp2_jet2_supported(in_dim, hidden, oc, nd, act) == want, (in_dim, hidden, oc, nd, act)


def test_host_layers_exist_with_their_signatures():
    from gaot_3d_amd import ops
    from gaot_3d_amd.model.gaot_3d import GAOT3D
    from gaot_3d_amd.model.layers.integral_transform import IntegralTransform
    from gaot_3d_amd.model.layers.magno import MAGNODecoder
    from gaot_3d_amd.model.layers.mlp import ChannelMLP, LinearChannelMLP
    names = lambda fn: list(inspect.signature(fn).parameters)
    assert names(ops.gno_forward_knn_jet2) == ["mode", "weights", "biases", "y_pos", "x_pos", "f_y", "src_table", "nbr", "k", "dirs"]
    assert callable(ops.mlp2_jet2) and callable(ops.mlp2_jet2_supported)
    assert names(IntegralTransform.jet2_knn) == ["self", "y_pos", "x_pos", "nbr", "k", "f_y", "dirs"]
    for cls in (LinearChannelMLP, ChannelMLP):
        assert names(cls.jet2_rows) == ["self", "x", "dxs", "ddxs", "out"]
        assert inspect.signature(cls.jet2_rows).parameters["out"].default is None
    for fn in (MAGNODecoder.sample_hessian, MAGNODecoder.sample_laplacian):
        assert names(fn) == ["self", "rndata_flat", "query_pos", "latent_tokens_pos", "chunk_points"]
    for fn in (GAOT3D.sample_hessian, GAOT3D.sample_laplacian):
        assert names(fn) == ["self", "latent", "query_pos", "tokens_pos", "chunk_points"]


def _model(strategy="knn"):
    from gaot_3d_amd.model import init_model
    from gaot_3d_amd.model.layers.attn import AttentionConfig, FFNConfig, TransformerConfig
    from gaot_3d_amd.model.layers.magno import MAGNOConfig
    cfg = types.SimpleNamespace(
        magno=MAGNOConfig(gno_coord_dim=3, lifting_channels=32, encoder_feature_attr="pos", mlp_type="linear",
                          use_geoembed=False, neighbor_strategy=strategy, k_neighbors=8),
        transformer=TransformerConfig(patch_size=2, hidden_size=64, num_layers=1, positional_embedding="rope",
                                      attn_config=AttentionConfig(hidden_size=64, num_heads=2, num_kv_heads=2, atten_dropout=0.0),
                                      ffn_config=FFNConfig(hidden_size=128)),
        latent_tokens=(4, 4, 4))
    return init_model(3, 1, "gaot_3d", cfg)


@pytest.mark.parametrize("method", ["sample_hessian", "sample_laplacian"])
def test_argument_rules_raise_on_the_host(method):
    with pytest.raises(ValueError, match="reverse"):
        getattr(_model(["knn", "reverse"]), method)(torch.zeros(64, 32), torch.zeros(5, 3))
    model = _model()
    with pytest.raises(ValueError, match="ONE sample"):
        getattr(model, method)(torch.zeros(128, 32), torch.zeros(5, 3))
    with pytest.raises(ValueError, match="chunk_points"):
        getattr(model, method)(torch.zeros(64, 32), torch.zeros(5, 3), chunk_points=0)
    with pytest.raises(NotImplementedError, match="radius"):
        getattr(_model(["knn", "radius"]), method)(torch.zeros(64, 32), torch.zeros(5, 3))


def _autograd_hessian(fn, x):
    """fn: x [N, D] -> [N, C] row by row.  -> (jac [N, C, D], hess [N, C, D, D]) by fp64 autograd, the second pass through the graph
    of the first (create_graph=True)"""
    xg = x.clone().requires_grad_(True)
    o = fn(xg)
    n, c, d = o.shape[0], o.shape[1], x.shape[1]
    jac, hess = torch.zeros(n, c, d, dtype=x.dtype), torch.zeros(n, c, d, d, dtype=x.dtype)
    for ch in range(c):
        (g,) = torch.autograd.grad(o[:, ch].sum(), xg, create_graph=True)
        jac[:, ch] = g.detach()
        for i in range(d):
            (gg,) = torch.autograd.grad(g[:, i].sum(), xg, retain_graph=True)
            hess[:, ch, i] = gg
    return o.detach(), jac, hess


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nh", [1, 2, 3, 4])
def test_gno_reference_is_double_backward_through_the_oracle(nh, mode):
    nq, nsrc, k = 20, 50, 4
    gen = torch.Generator().manual_seed(10 * nh + len(mode))
    cin = 0 if mode == "linear" else 32
    dims = [6 + cin] + [64] * nh + [32]
    ws = [torch.randn(dims[i + 1], dims[i], generator=gen, dtype=torch.float64) / math.sqrt(dims[i]) for i in range(len(dims) - 1)]
    bs = [0.1 * torch.randn(dims[i + 1], generator=gen, dtype=torch.float64) for i in range(len(dims) - 1)]
    y = torch.rand(nsrc, 3, generator=gen, dtype=torch.float64) * 2 - 1
    x = torch.rand(nq, 3, generator=gen, dtype=torch.float64) * 2 - 1
    f = torch.randn(nsrc, 32, generator=gen, dtype=torch.float64)
    nbr = torch.randint(0, nsrc, (nq * k,), generator=gen, dtype=torch.int32)                  # repeats allowed
    ei = torch.stack([nbr.long(), torch.arange(nq).repeat_interleave(k)])
    sd = {}
    for l, (w, b) in enumerate(zip(ws, bs)):
        sd[f"channel_mlp.fcs.{l}.weight"] = w
        sd[f"channel_mlp.fcs.{l}.bias"] = b
    o, jac, hess = _autograd_hessian(lambda xx: orc.integral_transform(sd, "", y, xx, ei, f, mode, False, 3), x)
    assert hess.abs().max() > 0
    close = lambda a, b: torch.allclose(a, b, rtol=1e-10, atol=1e-12)
    # the six directions of the Hessian: the value, the Jacobian from the axis planes, the Hessian by polarisation
    out, d1, d2 = REF.gno_knn_jet2(ws, bs, y, x, nbr, k, f, mode, REF.HESSIAN_DIRS)
    assert out.shape == (nq, 32) and d1.shape == d2.shape == (6, nq, 32) and d2.dtype == torch.float64
    assert close(out, o), (out - o).abs().max().item()
    assert close(d1[:3].permute(1, 2, 0), jac), (d1[:3].permute(1, 2, 0) - jac).abs().max().item()
    got = REF.hessian_from_jets(d2.permute(1, 2, 0))
    assert close(got, hess), (got - hess).abs().max().item()
    off = [hess[:, :, i, j] for i, j in REF.HESSIAN_PAIRS]
    assert min(o_.abs().max().item() for o_ in off) > 0
    for n, (i, j) in enumerate(REF.HESSIAN_PAIRS):                                     # the polarisation identity, entry by entry
        assert close(0.5 * (d2[3 + n] - d2[i] - d2[j]), hess[:, :, i, j]), (i, j)
    # generic directions, neither axis-aligned nor unit: D_v = J v, D_v^2 = v^T H v
    v = torch.tensor([[0.3, -1.7, 0.9], [-2.1, 0.4, 0.6]], dtype=torch.float64)
    _, g1, g2 = REF.gno_knn_jet2(ws, bs, y, x, nbr, k, f, mode, v.tolist())
    for n in range(2):
        assert close(g1[n], jac @ v[n]), n
        assert close(g2[n], torch.einsum("i,qcij,j->qc", v[n], hess, v[n])), n


def test_mlp_reference_is_double_backward_saturated_rows_included():
    gen = torch.Generator().manual_seed(3)
    w1 = torch.randn(64, 32, generator=gen, dtype=torch.float64) / math.sqrt(32)
    b1 = 0.1 * torch.randn(64, generator=gen, dtype=torch.float64)
    w2 = torch.randn(3, 64, generator=gen, dtype=torch.float64) / 8
    b2 = 0.1 * torch.randn(3, generator=gen, dtype=torch.float64)
    x = torch.randn(24, 32, generator=gen, dtype=torch.float64)
    x[16:] *= torch.linspace(3.0, 6.0, 8, dtype=torch.float64)[:, None]                  # rows whose |z| reaches 6-10
    zmax = (x @ w1.t() + b1).abs().amax(1)
    assert zmax[16:].max() >= 6.0 and zmax[:16].max() < 6.0, zmax
    dxs = [torch.randn(24, 32, generator=gen, dtype=torch.float64) for _ in range(3)]
    ddxs = [torch.randn(24, 32, generator=gen, dtype=torch.float64) for _ in range(3)]
    o, jac, hess = _autograd_hessian(lambda xx: torch.nn.functional.gelu(xx @ w1.t() + b1) @ w2.t() + b2, x)     # [N,3,32], [N,3,32,32]
    y, d1, d2 = REF.mlp_jet2(w1, b1, w2, b2, x, dxs, ddxs)
    assert y.shape == (24, 3) and d1.shape == d2.shape == (24, 3, 3)
    close = lambda a, b: torch.allclose(a, b, rtol=1e-10, atol=1e-12)
    assert close(y, o)
    for d in range(3):                       # along a curve x(t) with x' = dx, x'' = ddx: y' = J dx, y'' = dx^T H dx + J ddx
        assert close(d1[:, :, d], torch.einsum("nci,ni->nc", jac, dxs[d])), d
        want = torch.einsum("ni,ncij,nj->nc", dxs[d], hess, dxs[d]) + torch.einsum("nci,ni->nc", jac, ddxs[d])
        assert want.abs().max() > 0 and close(d2[:, :, d], want), (d, (d2[:, :, d] - want).abs().max().item())
    yb, _, _ = REF.mlp_jet2(w1, b1, w2, None, x, dxs, ddxs)
    assert close(yb + b2, y)


def test_polarisation_reproduces_an_autograd_hessian():
    """a smooth scalar field with a full Hessian: six second directional derivatives along HESSIAN_DIRS give every entry"""
    gen = torch.Generator().manual_seed(8)
    a = torch.randn(5, 3, generator=gen, dtype=torch.float64)
    fn = lambda xx: torch.stack([torch.sin(xx @ a[c]) * torch.exp(0.3 * xx[:, 0] * xx[:, 2]) for c in range(5)], dim=1)
    x = torch.randn(11, 3, generator=gen, dtype=torch.float64)
    _, _, hess = _autograd_hessian(fn, x)
    d2 = torch.stack([torch.einsum("i,qcij,j->qc", v, hess, v) for v in torch.tensor(REF.HESSIAN_DIRS, dtype=torch.float64)], dim=-1)
    got = REF.hessian_from_jets(d2)
    assert torch.equal(got, got.transpose(2, 3))
    assert min(hess[:, :, i, j].abs().max().item() for i, j in REF.HESSIAN_PAIRS) > 0
    assert torch.allclose(got, hess, rtol=1e-10, atol=1e-12), (got - hess).abs().max().item()
