"""CPU: the forward-only field-sampling interface is in place -- gaot_gno_fwd_knn (the fused GNO forward on a regular k-neighbour
list) is declared in the header, bound in _lib.SIGNATURES with the header's argument count and exported by the library, with the
ABI still version 11; ops.gno_forward_knn, IntegralTransform.forward_knn, MAGNODecoder.sample and GAOT3D.latent / GAOT3D.sample
exist; and the argument rules that need no device (reverse decoder, a batch of several graphs) raise on the host."""
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gaot_gno_fwd_knn"


def test_knn_forward_symbol_declared_bound_and_exported():
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
    assert callable(ops.gno_forward_knn) and ops.GNO_KNN_K == (1, 2, 4, 8, 16, 32)
    assert callable(IntegralTransform.forward_knn)
    assert callable(MAGNODecoder.sample)
    assert callable(GAOT3D.latent) and callable(GAOT3D.sample)


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
        model.sample(torch.zeros(64, 32), torch.zeros(5, 3))


def test_sample_takes_one_graph():
    model = _model()
    with pytest.raises(ValueError, match="ONE sample"):
        model.sample(torch.zeros(128, 32), torch.zeros(5, 3))
    with pytest.raises(ValueError, match="chunk_points"):
        model.sample(torch.zeros(64, 32), torch.zeros(5, 3), chunk_points=0)
