"""CPU: the field-Jacobian interface is in place -- gaot_gno_fwd_knn_jac (the fused GNO forward on a regular k-neighbour list with
three forward-mode tangents) is declared in the header, bound in _lib.SIGNATURES with the header's argument count and exported by
the library, with the ABI still version 11; ops.gno_forward_knn_jac, IntegralTransform.jacobian_knn, jvp_rows on both MLP classes,
MAGNODecoder.sample_jacobian and GAOT3D.sample_jacobian exist; the argument rules that need no device raise on the host; and the
closed-form reference the GPU tests compare against (tests/gno_jac_ref.py) is torch.autograd through the oracle's integral transform
in fp64.  (jvp_rows runs HIP kernels only: it is covered by tests/test_field_jacobian_gpu.py.)"""
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
import gno_jac_ref as REF  # noqa: E402

NAME = "gaot_gno_fwd_knn_jac"


def test_jacobian_symbol_declared_bound_and_exported():
    from gaot_3d_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gaot3d_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    m = re.search(r"\b" + NAME + r"\s*\(([^)]*)\)", src)
    assert m, f"{NAME} is not declared in include/gaot3d_hip.h"
    assert NAME in _lib.SIGNATURES, f"{NAME} is not in _lib.SIGNATURES"
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[NAME][1]) == 12, f"{NAME}: header and SIGNATURES disagree on the arguments"
    assert hasattr(lib, NAME), f"{NAME} is not exported by libgaot3d_hip.so"
    assert lib.gaot_abi_version() == 11


def test_host_layers_exist():
    from gaot_3d_amd import ops
    from gaot_3d_amd.model.gaot_3d import GAOT3D
    from gaot_3d_amd.model.layers.integral_transform import IntegralTransform
    from gaot_3d_amd.model.layers.magno import MAGNODecoder
    from gaot_3d_amd.model.layers.mlp import ChannelMLP, LinearChannelMLP
    assert callable(ops.gno_forward_knn_jac)
    assert callable(IntegralTransform.jacobian_knn)
    assert callable(LinearChannelMLP.jvp_rows) and callable(ChannelMLP.jvp_rows)
    assert callable(MAGNODecoder.sample_jacobian)
    assert callable(GAOT3D.sample_jacobian)


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


def test_reverse_decoder_is_refused():
    model = _model(["knn", "reverse"])
    with pytest.raises(ValueError, match="reverse"):
        model.sample_jacobian(torch.zeros(64, 32), torch.zeros(5, 3))


def test_sample_jacobian_takes_one_graph_and_a_positive_chunk():
    model = _model()
    with pytest.raises(ValueError, match="ONE sample"):
        model.sample_jacobian(torch.zeros(128, 32), torch.zeros(5, 3))
    with pytest.raises(ValueError, match="chunk_points"):
        model.sample_jacobian(torch.zeros(64, 32), torch.zeros(5, 3), chunk_points=0)


@pytest.mark.parametrize("mode", ["linear", "nonlinear", "nonlinear_kernelonly"])
@pytest.mark.parametrize("k", [1, 4])
def test_reference_is_autograd_through_the_oracle(k, mode):
    """both sides are fp64 evaluations of the same expression: one summed-channel backward per channel through the oracle"""
    nq, nsrc, nh = 7, 23, 2
    gen = torch.Generator().manual_seed(10 * k + len(mode))
    cin = 0 if mode == "linear" else 32
    dims = [6 + cin] + [64] * nh + [32]
    ws = [torch.randn(dims[i + 1], dims[i], generator=gen, dtype=torch.float64) / math.sqrt(dims[i]) for i in range(len(dims) - 1)]
    bs = [0.1 * torch.randn(dims[i + 1], generator=gen, dtype=torch.float64) for i in range(len(dims) - 1)]
    y = torch.rand(nsrc, 3, generator=gen, dtype=torch.float64) * 2 - 1
    x = torch.rand(nq, 3, generator=gen, dtype=torch.float64) * 2 - 1
    f = torch.randn(nsrc, 32, generator=gen, dtype=torch.float64)
    nbr = torch.randint(0, nsrc, (nq * k,), generator=gen, dtype=torch.int32)                  # repeats allowed
    ei = torch.stack([nbr.long(), torch.arange(nq).repeat_interleave(k)])
    out, jac = REF.gno_knn_jac(ws, bs, y, x, nbr, k, f, mode)
    assert out.shape == (nq, 32) and jac.shape == (3, nq, 32) and out.dtype == jac.dtype == torch.float64
    sd = {}
    for l, (w, b) in enumerate(zip(ws, bs)):
        sd[f"channel_mlp.fcs.{l}.weight"] = w
        sd[f"channel_mlp.fcs.{l}.bias"] = b
    xg = x.clone().requires_grad_(True)
    o = orc.integral_transform(sd, "", y, xg, ei, f, mode, False, 3)
    assert torch.allclose(out, o.detach(), rtol=1e-10, atol=1e-12), (out - o.detach()).abs().max().item()
    ref = torch.stack([torch.autograd.grad(o[:, c].sum(), xg, retain_graph=True)[0] for c in range(32)], dim=-1)   # [Nq, 3, C]
    ref = ref.permute(1, 0, 2)
    assert jac.abs().max() > 0
    assert torch.allclose(jac, ref, rtol=1e-10, atol=1e-12), (jac - ref).abs().max().item()
