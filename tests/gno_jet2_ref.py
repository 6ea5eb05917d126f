"""Closed-form fp64 references of the directional 2-jet kernels: gaot_gno_fwd_knn_jet2 (the fused GNO transform on a regular
k-neighbour list with its first and second directional derivative with respect to the query coordinate, the list held fixed),
gaot_mlp2_jet2 (the same for the two-layer projection MLP), and the polarisation that turns six directions into a Hessian.  Plain
torch, erf-GELU with its exact first and second derivative, no autograd.

Per edge e = (s, q), hidden layers l = 0..NH-1, last layer L, direction v (W_0 = [W_0y | W_0x | W_0f], the feature block only in the
nonlinear modes):
    z_0 = W_0 [y_s ; x_q ; f_s] + b_0       z'_0 = W_0[:, 3:6] v          z''_0 = 0
    h_l = gelu(z_l)                         h'_l = gelu'(z_l) z'_l        h''_l = gelu''(z_l) z'_l^2 + gelu'(z_l) z''_l
    z_{l+1} = W_{l+1} h_l + b_{l+1}         z'_{l+1} = W_{l+1} h'_l       z''_{l+1} = W_{l+1} h''_l
    out_q = (1/k) sum_e z_L * f[s_e]        d1_q = (1/k) sum_e z'_L * f[s_e]      d2_q = (1/k) sum_e z''_L * f[s_e]
(nonlinear_kernelonly: without f).  gelu''(z) = phi(z) (2 - z^2).
"""
import math

import torch

HESSIAN_DIRS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 1.0, 0.0), (0.0, 1.0, 1.0), (1.0, 0.0, 1.0))
HESSIAN_PAIRS = ((0, 1), (1, 2), (0, 2))


def gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def gelu_d1(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def gelu_d2(z):
    return torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi) * (2.0 - z * z)


def gno_knn_jet2(ws, bs, y, x, nbr, k, f, mode, dirs):
    """ws / bs: the kernel MLP's weights [out, in] / biases (layer 0 with its feature columns in the nonlinear modes); y [Ns, 3],
    x [Nq, 3], nbr [Nq * k] source ids, f [Ns, C], mode 'linear' / 'nonlinear' / 'nonlinear_kernelonly', dirs [nd][3].
    -> (out [Nq, C], d1 [nd, Nq, C], d2 [nd, Nq, C]) in fp64."""
    ws = [w.double() for w in ws]
    bs = [b.double() for b in bs]
    y, x, f = y.double(), x.double(), f.double()
    v = torch.as_tensor(dirs, dtype=torch.float64).reshape(-1, 3)
    nq = x.shape[0]
    s = nbr.long().reshape(nq, k)
    inp = torch.cat([y[s], x[:, None, :].expand(nq, k, 3)], dim=-1)                # [Nq, k, 6]
    if mode != "linear":
        inp = torch.cat([inp, f[s]], dim=-1)
    z = inp @ ws[0].t() + bs[0]                                                     # [Nq, k, H]
    dz = (v @ ws[0][:, 3:6].t())[:, None, None, :].expand(v.shape[0], nq, k, -1)    # [nd, Nq, k, H]
    ddz = torch.zeros_like(dz)
    for w, b in zip(ws[1:], bs[1:]):
        g1, g2 = gelu_d1(z)[None], gelu_d2(z)[None]
        h, dh, ddh = gelu(z), g1 * dz, g2 * dz * dz + g1 * ddz
        z, dz, ddz = h @ w.t() + b, dh @ w.t(), ddh @ w.t()
    if mode != "nonlinear_kernelonly":
        z, dz, ddz = z * f[s], dz * f[s][None], ddz * f[s][None]
    return z.sum(1) / k, dz.sum(2) / k, ddz.sum(2) / k


def mlp_jet2(w1, b1, w2, b2, x, dxs, ddxs):
    """y = w2 gelu(w1 x + b1) + b2 with, per direction, its first and second directional derivative given the first-order plane
    dxs[d] and the second-order plane ddxs[d] of x.  -> (y [N, out], d1 [N, out, nd], d2 [N, out, nd]) in fp64."""
    w1, b1, w2 = w1.double(), b1.double(), w2.double()
    z = x.double() @ w1.t() + b1
    y = gelu(z) @ w2.t()
    if b2 is not None:
        y = y + b2.double()
    g1, g2 = gelu_d1(z), gelu_d2(z)
    d1, d2 = [], []
    for dx, ddx in zip(dxs, ddxs):
        u, w = dx.double() @ w1.t(), ddx.double() @ w1.t()
        d1.append((g1 * u) @ w2.t())
        d2.append((g2 * u * u + g1 * w) @ w2.t())
    return y, torch.stack(d1, dim=-1), torch.stack(d2, dim=-1)


def hessian_from_jets(d2):
    """d2 [..., 6]: the second directional derivatives along HESSIAN_DIRS -> the Hessian [..., 3, 3] by polarisation,
    H_ii = D^2_{e_i}, H_ij = (D^2_{e_i + e_j} - D^2_{e_i} - D^2_{e_j}) / 2"""
    h = d2.new_empty(*d2.shape[:-1], 3, 3)
    for i in range(3):
        h[..., i, i] = d2[..., i]
    for n, (i, j) in enumerate(HESSIAN_PAIRS):
        off = 0.5 * (d2[..., 3 + n] - d2[..., i] - d2[..., j])
        h[..., i, j] = off
        h[..., j, i] = off
    return h
