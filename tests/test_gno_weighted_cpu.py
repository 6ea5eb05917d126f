"""CPU: the weighted fused GNO entry points (gaot_gno_fwd_w / gaot_gno_bwd_w / gaot_gno_bwd_w_workspace_bytes) are part of the C ABI --
declared in the header, bound in _lib.SIGNATURES with the header's argument counts, exported by the library, ABI still version 11 --
the host layers exist, and the fp64 reference of the GPU tests (tests/gno_w_ref.py) has teeth: with softmax weights it is the oracle's
attention-weighted transform, with 1/deg the mean transform, and its dalpha is the first-order change of the output."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gaot_oracle as orc  # noqa: E402
import gno_w_ref as WR  # noqa: E402

NAMES = ("gaot_gno_fwd_w", "gaot_gno_bwd_w", "gaot_gno_bwd_w_workspace_bytes")


def test_weighted_symbols_declared_bound_and_exported():
    from gaot_3d_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gaot3d_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
        assert m, f"{name} is not declared in include/gaot3d_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), f"{name}: header and SIGNATURES disagree on the arguments"
        assert hasattr(lib, name), f"{name} is not exported by libgaot3d_hip.so"
    assert lib.gaot_abi_version() == 11


def test_host_layers_exist():
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd import ops
    from gaot_3d_amd.model.layers.integral_transform import IntegralTransform
    assert callable(ops.gno_w_forward) and callable(ops.gno_w_backward)
    assert issubclass(GF.GnoWFn, torch.autograd.Function)
    assert callable(IntegralTransform._fused_attn_plan) and callable(IntegralTransform._attn_weights)


def _sd(case, cd, attention_type, gen):
    sd = {}
    for l, (w, b) in enumerate(zip(case["ws"], case["bs"])):
        sd[f"channel_mlp.fcs.{l}.weight"] = w.double()
        sd[f"channel_mlp.fcs.{l}.bias"] = b.double()
    if attention_type == "dot_product":
        for n in ("query_proj", "key_proj"):
            sd[f"{n}.weight"] = torch.randn(64, cd, dtype=torch.float64, generator=gen)
            sd[f"{n}.bias"] = torch.randn(64, dtype=torch.float64, generator=gen)
    return sd


def _scores(sd, case, cd, attention_type):
    s, q = case["ei"][0].long(), case["ei"][1].long()
    qc, kc = case["x"].double()[q][:, :cd], case["y"].double()[s][:, :cd]
    if attention_type == "dot_product":
        qq = torch.nn.functional.linear(qc, sd["query_proj.weight"], sd["query_proj.bias"])
        kk = torch.nn.functional.linear(kc, sd["key_proj.weight"], sd["key_proj.bias"])
        return (qq * kk).sum(-1) / 8.0
    return (torch.nn.functional.normalize(qc, dim=-1) * torch.nn.functional.normalize(kc, dim=-1)).sum(-1)


@pytest.mark.parametrize("attention_type", ["cosine", "dot_product"])
@pytest.mark.parametrize("mode", WR.MODES)
def test_reference_with_softmax_weights_is_the_oracle_attention_transform(mode, attention_type):
    case = WR.w_case("tail", mode, 129, 2)
    gen = torch.Generator().manual_seed(4)
    for cd in (3, 2):                                   # the scores see the first coord_dim coordinates
        sd = _sd(case, cd, attention_type, gen)
        alpha = orc._segment_softmax(_scores(sd, case, cd, attention_type), case["ei"][1].long(), case["n_dst"])
        got = WR.w_ref(case, alpha=alpha)["out"]
        ref = orc.integral_transform(sd, "", case["y"].double(), case["x"].double(), case["ei"], case["f"].double(), mode, True, cd,
                                     attention_type)
        torch.testing.assert_close(got, ref, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("mode", WR.MODES)
def test_reference_with_inverse_degree_weights_is_the_mean_transform(mode):
    case = WR.w_case("mid", mode, WR.MID_E, 3)
    q = case["ei"][1].long()
    deg = torch.bincount(q, minlength=case["n_dst"]).double()
    got = WR.w_ref(case, alpha=(1.0 / deg)[q])["out"]
    sd = _sd(case, 3, "cosine", None)
    ref = orc.integral_transform(sd, "", case["y"].double(), case["x"].double(), case["ei"], case["f"].double(), mode, None, 3)
    torch.testing.assert_close(got, ref, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("mode", WR.MODES)
def test_reference_dalpha_is_the_first_order_change_of_the_output(mode):
    case = WR.w_case("tail", mode, 33, 2)
    base = WR.w_ref(case)
    gout = case["gout"].double()
    for e in (0, 17, 32):
        delta = 1e-6
        a2 = case["alpha"].double().clone()
        a2[e] += delta
        moved = WR.w_ref(case, alpha=a2)["out"]
        change = ((moved - base["out"]) * gout).sum()             # out is linear in alpha: exact up to rounding
        torch.testing.assert_close(change, base["dalpha"][e] * delta, rtol=1e-7, atol=1e-16)
        q = int(case["ei"][1][e])
        rows = torch.ones(case["n_dst"], dtype=torch.bool)
        rows[q] = False
        assert torch.equal(moved[rows], base["out"][rows])        # only the edge's query row moves
