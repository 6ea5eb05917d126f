"""Closed-form fp64 reference of gaot_gno_fwd_jet2: the fused GNO transform on RAGGED rows -- the by-query list (src, dst, rowptr) of any
graph -- with its first and second directional derivative with respect to the query coordinate, every query's list held fixed.  The
per-edge recurrences are tests/gno_jet2_ref.py's (gno_knn_jet2: erf-GELU with its exact first and second derivative, no autograd),
evaluated edge by edge; a row is the MEAN over its edges and an empty row is zero in all 1 + 2 nd planes:
    out_q = (1/deg_q) sum_{e -> q} z_L * f[s_e],   d1_q = (1/deg_q) sum_{e -> q} z'_L * f[s_e],   d2_q = (1/deg_q) sum_{e -> q} z''_L * f[s_e]
(nonlinear_kernelonly: without f).
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gno_jet2_ref import gelu, gelu_d1, gelu_d2  # noqa: E402


def gno_rows_jet2(ws, bs, y, x, src, dst, rowptr, f, mode, dirs):
    """ws / bs: the kernel MLP's weights [out, in] / biases (layer 0 with its feature columns in the nonlinear modes); y [Ns, 3],
    x [Nq, 3]; src / dst [E]: source and query of every edge, sorted by query; rowptr [Nq + 1]; f [Ns, C]; mode 'linear' /
    'nonlinear' / 'nonlinear_kernelonly'; dirs [nd][3].  -> (out [Nq, C], d1 [nd, Nq, C], d2 [nd, Nq, C]) in fp64."""
    ws = [w.double() for w in ws]
    bs = [b.double() for b in bs]
    y, x, f = y.double(), x.double(), f.double()
    v = torch.as_tensor(dirs, dtype=torch.float64).reshape(-1, 3)
    nq, nd = x.shape[0], v.shape[0]
    s, q = src.long(), dst.long()
    deg = (rowptr[1:] - rowptr[:-1]).long()
    assert rowptr.numel() == nq + 1 and int(rowptr[-1]) == s.numel() == q.numel()
    assert torch.equal(q, torch.repeat_interleave(torch.arange(nq), deg)), "dst is not the row index of rowptr"
    inp = torch.cat([y[s], x[q]], dim=-1)                                          # [E, 6]
    if mode != "linear":
        inp = torch.cat([inp, f[s]], dim=-1)
    z = inp @ ws[0].t() + bs[0]                                                    # [E, H]
    dz = (v @ ws[0][:, 3:6].t())[:, None, :].expand(nd, s.numel(), -1)             # [nd, E, H]
    ddz = torch.zeros_like(dz)
    for w, b in zip(ws[1:], bs[1:]):
        g1, g2 = gelu_d1(z)[None], gelu_d2(z)[None]
        h, dh, ddh = gelu(z), g1 * dz, g2 * dz * dz + g1 * ddz
        z, dz, ddz = h @ w.t() + b, dh @ w.t(), ddh @ w.t()
    if mode != "nonlinear_kernelonly":
        z, dz, ddz = z * f[s], dz * f[s][None], ddz * f[s][None]
    c = z.shape[1]
    out = torch.zeros(nq, c, dtype=torch.float64).index_add_(0, q, z)
    d1 = torch.zeros(nd, nq, c, dtype=torch.float64).index_add_(1, q, dz)
    d2 = torch.zeros(nd, nq, c, dtype=torch.float64).index_add_(1, q, ddz)
    inv = torch.where(deg > 0, 1.0 / deg.clamp(min=1).double(), torch.zeros(nq, dtype=torch.float64))
    return out * inv[:, None], d1 * inv[None, :, None], d2 * inv[None, :, None]
