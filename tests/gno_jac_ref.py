"""Closed-form fp64 reference of gaot_gno_fwd_knn_jac: the fused GNO transform on a regular k-neighbour list and its derivative with
respect to the query coordinate, the neighbour list held fixed.  Plain torch, erf-GELU and its exact derivative, no autograd.

Per edge e = (s, q), hidden layers l = 0..NH-1, last layer L, direction d = 0..2 (W_0 = [W_0y | W_0x | W_0f], the feature block only
in the nonlinear modes):
    z_0 = W_0 [y_s ; x_q ; f_s] + b_0,   h_0 = gelu(z_0),   dh_0^d = gelu'(z_0) * W_0[:, 3 + d]
    z_l = W_l h_{l-1} + b_l,            h_l = gelu(z_l),   dh_l^d = gelu'(z_l) * (W_l dh_{l-1}^d)
    k   = W_L h_{NH-1} + b_L,                               dk^d   = W_L dh_{NH-1}^d
    out_q = (1/k) sum_e k_e * f[s_e],   jac_q^d = (1/k) sum_e dk_e^d * f[s_e]          (nonlinear_kernelonly: without f)
"""
import math

import torch


def _gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def _gelu_grad(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def gno_knn_jac(ws, bs, y, x, nbr, k, f, mode):
    """ws / bs: the kernel MLP's weights [out, in] / biases (layer 0 with its feature columns in the nonlinear modes); y [Ns, 3],
    x [Nq, 3], nbr [Nq * k] source ids, f [Ns, C], mode 'linear' / 'nonlinear' / 'nonlinear_kernelonly'.
    -> (out [Nq, C], jac [3, Nq, C]) in fp64."""
    ws = [w.double() for w in ws]
    bs = [b.double() for b in bs]
    y, x, f = y.double(), x.double(), f.double()
    nq = x.shape[0]
    s = nbr.long().reshape(nq, k)
    inp = torch.cat([y[s], x[:, None, :].expand(nq, k, 3)], dim=-1)                # [Nq, k, 6]
    if mode != "linear":
        inp = torch.cat([inp, f[s]], dim=-1)
    z = inp @ ws[0].t() + bs[0]
    h = _gelu(z)
    dh = _gelu_grad(z)[None] * ws[0][:, 3:6].t()[:, None, None, :]                 # [3, Nq, k, H]
    for w, b in zip(ws[1:-1], bs[1:-1]):
        z = h @ w.t() + b
        h = _gelu(z)
        dh = _gelu_grad(z)[None] * (dh @ w.t())
    kv = h @ ws[-1].t() + bs[-1]
    dk = dh @ ws[-1].t()
    if mode != "nonlinear_kernelonly":
        kv = kv * f[s]
        dk = dk * f[s][None]
    return kv.sum(1) / k, dk.sum(2) / k
