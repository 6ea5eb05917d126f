"""CPU: the fused projection-tangent kernel is in place -- gaot_mlp2_jvp_supported and gaot_mlp2_jvp are declared in the header, bound
in _lib.SIGNATURES with the header's argument counts and exported by the library, with the ABI still version 11;
gaot_mlp2_jvp_supported accepts exactly 32 -> {64, 128, 256} -> 1..4 with 0..3 tangents and erf-GELU; ``jvp_rows`` of both MLP classes
takes ``fused`` and ``out``; and the closed-form reference the GPU tests compare against (tests/mlp_jvp_ref.py) is
torch.autograd.functional.jvp of the same MLP in fp64, rows with a saturated GELU' included."""
import inspect
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_jvp_ref as REF  # noqa: E402

NAMES = {"gaot_mlp2_jvp_supported": 5, "gaot_mlp2_jvp": 20}      # arguments in the header


@pytest.mark.parametrize("name", list(NAMES))
def test_symbols_declared_bound_and_exported(name):
    from gaot_3d_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gaot3d_hip.h")).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
    assert m, f"{name} is not declared in include/gaot3d_hip.h"
    assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == NAMES[name], f"{name}: header and SIGNATURES disagree"
    lib = _lib.load()
    assert hasattr(lib, name), f"{name} is not exported by libgaot3d_hip.so"
    assert lib.gaot_abi_version() == 11


def test_supported_is_exactly_the_family():
    from gaot_3d_amd import _lib, ops
    lib = _lib.load()
    gelu = ops.ACT["gelu"]
    for hidden in (64, 128, 256):
        for oc in (1, 2, 3, 4):
            for t in (0, 1, 2, 3):
                assert lib.gaot_mlp2_jvp_supported(32, hidden, oc, t, gelu) == 1, (hidden, oc, t)
    for bad in ((16, 256, 1, 3), (48, 256, 1, 3), (32, 32, 1, 3), (32, 96, 1, 3), (32, 256, 0, 3), (32, 256, 5, 3), (32, 256, 1, 4),
                (32, 256, 1, -1), (32, 512, 1, 3)):
        assert lib.gaot_mlp2_jvp_supported(*bad, gelu) == 0, bad
    for name, act in ops.ACT.items():
        assert lib.gaot_mlp2_jvp_supported(32, 256, 4, 3, act) == (1 if act == gelu else 0), name
    assert lib.gaot_mlp2_jvp_supported(32, 256, 4, 3, 99) == 0


def test_host_layers_take_fused_and_out():
    from gaot_3d_amd import ops
    from gaot_3d_amd.model.layers.mlp import ChannelMLP, LinearChannelMLP
    assert callable(ops.mlp2_jvp)
    for cls in (LinearChannelMLP, ChannelMLP):
        par = inspect.signature(cls.jvp_rows).parameters
        assert list(par) == ["self", "x", "dxs", "fused", "out"], cls
        assert par["fused"].default is None and par["out"].default is None, cls


def test_reference_is_autograd_jvp_in_fp64():
    """H = 64, out = 3, 40 rows; rows 30.. are scaled so that |z| reaches 6-10, where gelu' is 0 or 1 to fp64 rounding"""
    gen = torch.Generator().manual_seed(11)
    n, hid, oc = 40, 64, 3
    w1 = torch.randn(hid, 32, generator=gen, dtype=torch.float64) / 32 ** 0.5
    b1 = 0.1 * torch.randn(hid, generator=gen, dtype=torch.float64)
    w2 = torch.randn(oc, hid, generator=gen, dtype=torch.float64) / hid ** 0.5
    b2 = 0.1 * torch.randn(oc, generator=gen, dtype=torch.float64)
    x = torch.randn(n, 32, generator=gen, dtype=torch.float64)
    x[30:] *= 4.0
    dxs = [torch.randn(n, 32, generator=gen, dtype=torch.float64) for _ in range(3)]
    z = x @ w1.t() + b1
    big = z[30:].abs()
    assert ((big > 6) & (big < 10)).any() and z[:30].abs().max() < 6
    for bias2 in (b2, None):
        f = lambda xx: torch.nn.functional.gelu(xx @ w1.t() + b1) @ w2.t() + (0 if bias2 is None else bias2)
        y, dys = REF.mlp_jvp(w1, b1, w2, bias2, x, dxs)
        assert y.dtype == torch.float64 and y.shape == (n, oc) and len(dys) == 3
        for d in range(3):
            yr, dr = torch.autograd.functional.jvp(f, x, dxs[d])
            assert torch.allclose(y, yr, rtol=1e-12, atol=1e-13)
            assert dys[d].shape == (n, oc) and dys[d].abs().max() > 0.1
            assert torch.allclose(dys[d], dr, rtol=1e-10, atol=1e-12), (dys[d] - dr).abs().max().item()
    assert torch.equal(REF.mlp_jvp(w1, b1, w2, b2, x, [torch.zeros_like(x)])[1][0], torch.zeros(n, oc, dtype=torch.float64))
