"""CPU: the yardstick of the coordinate-gradient tests (tests/test_coord_grad_gpu.py) -- the oracle's integral transform and
statistical GeoEmbed features differentiate correctly in the coordinates (torch.autograd.gradcheck, fp64) -- and the new
C ABI entry points are declared."""
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gaot_oracle as orc  # noqa: E402  (checker only)


def _graph():
    # 7 sources, 5 queries: degrees 3, 1, 0, 4, 2 (an empty row, a row of degree 1)
    src = torch.tensor([0, 3, 5, 1, 2, 4, 6, 0, 1, 6])
    dst = torch.tensor([0, 0, 0, 1, 3, 3, 3, 3, 4, 4])
    return torch.stack([src, dst])


def test_oracle_integral_transform_gradcheck():
    g = torch.Generator().manual_seed(0)
    ei = _graph()
    sd = {}
    dims = [6, 8, 8, 4]
    for i in range(3):
        sd[f"channel_mlp.fcs.{i}.weight"] = torch.randn(dims[i + 1], dims[i], generator=g, dtype=torch.float64) * 0.5
        sd[f"channel_mlp.fcs.{i}.bias"] = torch.randn(dims[i + 1], generator=g, dtype=torch.float64) * 0.1
    y = torch.rand(7, 3, generator=g, dtype=torch.float64).requires_grad_()
    x = torch.rand(5, 3, generator=g, dtype=torch.float64).requires_grad_()
    f = torch.randn(7, 4, generator=g, dtype=torch.float64)
    assert torch.autograd.gradcheck(lambda a, b: orc.integral_transform(sd, "", a, b, ei, f), (y, x))


def test_oracle_geoembed_stat_features_gradcheck():
    g = torch.Generator().manual_seed(1)
    ei = _graph()
    s = torch.rand(7, 3, generator=g, dtype=torch.float64).requires_grad_()
    q = torch.rand(5, 3, generator=g, dtype=torch.float64).requires_grad_()
    assert torch.autograd.gradcheck(lambda a, b: orc.geoembed_stat_features(a, b, ei), (s, q))


def test_coordinate_gradient_symbols_declared():
    hdr = open(os.path.join(ROOT, "include", "gaot3d_hip.h")).read()
    sys.path.insert(0, ROOT)
    from gaot_3d_amd import _lib
    for name in ("gaot_gno_bwd_coords", "gaot_geoembed_from_moments_bwd", "gaot_geoembed_from_moments_bwd_workspace_bytes",
                 "gaot_geoembed_moments_bwd"):
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in _lib.SIGNATURES, name
