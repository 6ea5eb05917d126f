"""Closed-form fp64 reference of the projection MLP's forward-mode tangent (csrc/mlp2_jvp.hip, ``jvp_rows``), in plain torch:
    z = x W1^T + b1,  y = gelu(z) W2^T + b2,  dy_d = (gelu'(z) * (dx_d W1^T)) W2^T
with erf-GELU, gelu'(z) = Phi(z) + z phi(z).  tests/test_projection_jvp_cpu.py checks it against torch.autograd.functional.jvp."""
import math

import torch


def gelu_grad(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def mlp_jvp(w1, b1, w2, b2, x, dxs):
    """-> (y [N, out], [dy_d [N, out]]) in fp64 from operands of any float dtype (b2 may be None)"""
    w1, b1, w2, x = w1.double(), b1.double(), w2.double(), x.double()
    z = x @ w1.t() + b1
    y = torch.nn.functional.gelu(z) @ w2.t()
    if b2 is not None:
        y = y + b2.double()
    g = gelu_grad(z)
    return y, [(g * (d.double() @ w1.t())) @ w2.t() for d in dxs]


def weights_of(mlp):
    """(w1, b1, w2, b2) of a two-layer LinearChannelMLP / ChannelMLP as CPU tensors"""
    fcs = list(mlp.fcs)
    w = [(fc.weight[:, :, 0] if fc.weight.dim() == 3 else fc.weight).detach().cpu() for fc in fcs]
    b = [None if fc.bias is None else fc.bias.detach().cpu() for fc in fcs]
    return w[0], b[0], w[1], b[1]
