"""CPU: training the decoder through the sampled field is in place -- the four gaot_mlp2_bwd_f32 symbols are declared in the header, bound
in _lib.SIGNATURES with the header's argument counts and exported by the library at ABI version 11; gaot_mlp2_bwd_f32_supported is 1
for exactly the family 32 -> {64, 128, 256} -> 1..4 with erf-GELU; the three instantiations of the kernel use no scratch; the host
layers exist with their signatures; and ops.mlp2_backward_f32, sample_vjp_params and sample_autograd_params refuse on
the host what they refuse, before a device is touched."""
import inspect
import os
import re
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_field_hessian_cpu as hc  # noqa: E402  (_kernel_scratch_sizes)

NAMES = {"gaot_mlp2_bwd_f32_supported": 4, "gaot_mlp2_bwd_f32_workspace_bytes": 2, "gaot_mlp2_bwd_f32_parts": 1, "gaot_mlp2_bwd_f32": 16}


@pytest.mark.parametrize("name", list(NAMES))
def test_symbols_declared_bound_and_exported(name):
    from gaot_3d_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gaot3d_hip.h")).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
    assert m, f"{name} is not declared in include/gaot3d_hip.h"
    assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == NAMES[name], f"{name}: header and SIGNATURES disagree"
    assert hasattr(_lib.load(), name), f"{name} is not exported by libgaot3d_hip.so"
    assert _lib.load().gaot_abi_version() == 11


def test_supported_is_exactly_the_family():
    from gaot_3d_amd import ops
    gelu = ops.ACT["gelu"]
    for in_dim in (3, 16, 31, 32, 33, 64):
        for hidden in (0, 32, 63, 64, 96, 128, 192, 256, 257, 512):
            for out in (0, 1, 2, 3, 4, 5, 32):
                for act in (ops.ACT["none"], gelu, ops.ACT["relu"], ops.ACT["silu"], ops.ACT["gelu_tanh"]):
                    want = in_dim == 32 and hidden in (64, 128, 256) and 1 <= out <= 4 and act == gelu
                    assert ops.mlp2_bwd_f32_supported(in_dim, hidden, out, act) == want, (in_dim, hidden, out, act)


def test_parts_and_workspace():
    from gaot_3d_amd import _lib
    lib = _lib.load()
    assert [lib.gaot_mlp2_bwd_f32_parts(n) for n in (0, 1, 128, 129, 1 << 20, 1 << 33)] == [0, 1, 1, 2, 512, 512]
    for hidden in (64, 128, 256):
        for out in (1, 4):
            assert lib.gaot_mlp2_bwd_f32_workspace_bytes(hidden, out) >= 4 * 512 * (hidden * 32 + hidden + out * hidden)


def test_kernels_have_no_scratch():
    from gaot_3d_amd import _lib
    sizes = hc._kernel_scratch_sizes(_lib.load()._name)
    mine = {k: v for k, v in sizes.items() if "k_mlp2_bwd_f32" in k}
    assert len(mine) == 3, sorted(mine)
    assert not any(mine.values()), mine


def test_host_layers_exist_with_their_signatures():
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd import ops
    from gaot_3d_amd.model.gaot_3d import GAOT3D
    from gaot_3d_amd.model.layers.magno import MAGNODecoder
    names = lambda fn: list(inspect.signature(fn).parameters)
    assert names(ops.mlp2_backward_f32) == ["x", "w1", "b1", "w2", "dout"]
    assert names(ops.mlp2_bwd_f32_supported) == ["in_dim", "hidden", "out_dim", "act"]
    assert names(MAGNODecoder.sample_vjp_params) == ["self", "rndata_flat", "query_pos", "cotangent", "latent_tokens_pos", "chunk_points"]
    assert names(GAOT3D.sample_vjp_params) == ["self", "latent", "query_pos", "cotangent", "tokens_pos", "chunk_points"]
    assert names(GAOT3D.sample_autograd_params) == names(GAOT3D.sample_autograd) == ["self", "latent", "query_pos", "tokens_pos", "chunk_points"]
    assert issubclass(GF.SampleTrainFn, torch.autograd.Function)


def test_mlp2_backward_f32_argument_rules_raise_on_the_host():
    from gaot_3d_amd import ops
    from gaot_3d_amd._lib import GaotError
    x, w1, b1, w2, g = torch.zeros(10, 32), torch.zeros(256, 32), torch.zeros(256), torch.zeros(2, 256), torch.zeros(10, 2)
    bad = [
        (x.double(), w1, b1, w2, g), (x, w1, b1, w2, g[:5]), (x, w1, b1[:5], w2, g), (x, w1.t(), b1, w2, g), (x[0], w1, b1, w2, g),
        (x, torch.zeros(96, 32), torch.zeros(96), torch.zeros(2, 96), g),                   # hidden outside the family
        (torch.zeros(10, 16), torch.zeros(256, 16), b1, w2, g),                             # input width
        (x, w1, b1, torch.zeros(5, 256), torch.zeros(10, 5)),                               # five outputs
        (x, w1, b1, w2, None),
        (x, w1, b1, w2, g),                                                                 # host tensors: no CPU fallback
    ]
    for i, args in enumerate(bad):
        with pytest.raises(GaotError):
            ops.mlp2_backward_f32(*args)


def _cpu_model(out=1, **magno):
    from gaot_3d_amd.model import init_model
    from gaot_3d_amd.model.layers.attn import AttentionConfig, FFNConfig, TransformerConfig
    from gaot_3d_amd.model.layers.magno import MAGNOConfig
    kw = dict(gno_coord_dim=3, lifting_channels=32, encoder_feature_attr="pos", mlp_type="linear", use_geoembed=False,
              neighbor_strategy="knn", k_neighbors=8)
    kw.update(magno)
    cfg = types.SimpleNamespace(
        magno=MAGNOConfig(**kw),
        transformer=TransformerConfig(patch_size=2, hidden_size=64, num_layers=1, positional_embedding="rope",
                                      attn_config=AttentionConfig(hidden_size=64, num_heads=2, num_kv_heads=2, atten_dropout=0.0),
                                      ffn_config=FFNConfig(hidden_size=128)),
        latent_tokens=(4, 4, 4))
    torch.manual_seed(3)
    return init_model(3, out, "gaot_3d", cfg)


def _args(nq=5, out=1):
    return torch.zeros(64, 32), torch.zeros(nq, 3), torch.zeros(nq, out)


def test_argument_rules_raise_on_the_host():
    lat, q, g = _args()
    model = _cpu_model(neighbor_strategy=["knn", "reverse"])
    with pytest.raises(ValueError, match="reverse"):
        model.sample_vjp_params(lat, q, g)
    model = _cpu_model()
    with pytest.raises(ValueError, match="ONE sample"):
        model.sample_vjp_params(torch.zeros(128, 32), q, g)
    with pytest.raises(ValueError, match="chunk_points"):
        model.sample_vjp_params(lat, q, g, chunk_points=0)
    for bad in (g.double(), torch.zeros(5, 2), torch.zeros(4, 1), torch.zeros(5), [[0.0]] * 5):
        with pytest.raises(ValueError, match="cotangent"):
            model.sample_vjp_params(lat, q, bad)
    with pytest.raises(ValueError, match="query_pos requires grad"):
        model.sample_autograd_params(lat, q.clone().requires_grad_(True))
    model.decoder._shard_group = object()
    with pytest.raises(NotImplementedError, match="point-sharded"):
        model.sample_vjp_params(lat, q, g)


REFUSALS = {
    "four_hidden_layers": (dict(out_gno_channel_mlp_hidden_layers=[64, 64, 64, 64]), "4 hidden layers"),
    "use_attn": (dict(use_attn=True), "use_attn"),
    "geoembed": (dict(use_geoembed=[False, True], embedding_method="pointnet"), "GeoEmbed"),
    "nonlinear": (dict(out_gno_transform_type="nonlinear"), "'nonlinear'"),
    "k3": (dict(k_neighbors=3), "k_neighbors = 3"),
    "host_operands": (dict(), "do not stream"),          # tokens and queries on the host: nothing streams there
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_configurations_are_refused_by_name(case):
    kw, msg = REFUSALS[case]
    model = _cpu_model(**kw)
    lat, q, g = _args()
    with pytest.raises(NotImplementedError, match=msg):
        model.sample_vjp_params(lat, q, g)
    if case != "four_hidden_layers":       # the model's autograd form names sample_vjp's refusals first (host operands do not stream)
        with pytest.raises(NotImplementedError, match=msg):
            model.sample_autograd_params(lat.clone().requires_grad_(True), q)
