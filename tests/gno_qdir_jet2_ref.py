"""Closed-form fp64 references of the directional 2-jet kernels along PER-QUERY directions (gaot_gno_fwd_knn_jet2_qd on a regular
k-neighbour list, gaot_gno_fwd_jet2_qd on ragged rows): tests/gno_jet2_ref.py's gno_knn_jet2 and tests/gno_rows_jet2_ref.py's
gno_rows_jet2 with a direction tensor v [Nq, nd, 3], so that the first-layer tangent is per query,
    z'_0[i, e] = W_0[:, 3:6] v[q_e, i]        (q_e the query of edge e),        z''_0 = 0,
and everything after it -- the recurrences through the layers, the product with f, the row means, empty rows zero -- is theirs.  Plain
torch, erf-GELU with its exact first and second derivative, no autograd.  With the same directions for every query the results are
those of the two references (same expressions on the same numbers)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gno_jet2_ref import gelu, gelu_d1, gelu_d2  # noqa: E402


def _layers(ws, bs, z, dz):
    """z [..edges.., H], dz [nd, ..edges.., H] through the hidden activations and the remaining layers -> (z_L, z'_L, z''_L)"""
    ddz = torch.zeros_like(dz)
    for w, b in zip(ws[1:], bs[1:]):
        g1, g2 = gelu_d1(z)[None], gelu_d2(z)[None]
        h, dh, ddh = gelu(z), g1 * dz, g2 * dz * dz + g1 * ddz
        z, dz, ddz = h @ w.t() + b, dh @ w.t(), ddh @ w.t()
    return z, dz, ddz


def gno_knn_jet2_qd(ws, bs, y, x, nbr, k, f, mode, qdirs):
    """ws / bs, y [Ns, 3], x [Nq, 3], nbr [Nq * k], f [Ns, C], mode as in gno_jet2_ref.gno_knn_jet2; qdirs [Nq, nd, 3].
    -> (out [Nq, C], d1 [nd, Nq, C], d2 [nd, Nq, C]) in fp64."""
    ws = [w.double() for w in ws]
    bs = [b.double() for b in bs]
    y, x, f = y.double(), x.double(), f.double()
    v = torch.as_tensor(qdirs, dtype=torch.float64)
    nq, nd = x.shape[0], v.shape[1]
    assert v.shape == (nq, nd, 3)
    s = nbr.long().reshape(nq, k)
    inp = torch.cat([y[s], x[:, None, :].expand(nq, k, 3)], dim=-1)                # [Nq, k, 6]
    if mode != "linear":
        inp = torch.cat([inp, f[s]], dim=-1)
    z = inp @ ws[0].t() + bs[0]                                                     # [Nq, k, H]
    dz = (v @ ws[0][:, 3:6].t()).permute(1, 0, 2)[:, :, None, :].expand(nd, nq, k, -1)   # [nd, Nq, k, H]: per query
    z, dz, ddz = _layers(ws, bs, z, dz)
    if mode != "nonlinear_kernelonly":
        z, dz, ddz = z * f[s], dz * f[s][None], ddz * f[s][None]
    return z.sum(1) / k, dz.sum(2) / k, ddz.sum(2) / k


def gno_rows_jet2_qd(ws, bs, y, x, src, dst, rowptr, f, mode, qdirs):
    """the operands of gno_rows_jet2_ref.gno_rows_jet2 with qdirs [Nq, nd, 3] -> (out [Nq, C], d1 [nd, Nq, C], d2 [nd, Nq, C]) in fp64"""
    ws = [w.double() for w in ws]
    bs = [b.double() for b in bs]
    y, x, f = y.double(), x.double(), f.double()
    v = torch.as_tensor(qdirs, dtype=torch.float64)
    nq, nd = x.shape[0], v.shape[1]
    assert v.shape == (nq, nd, 3)
    s, q = src.long(), dst.long()
    deg = (rowptr[1:] - rowptr[:-1]).long()
    assert rowptr.numel() == nq + 1 and int(rowptr[-1]) == s.numel() == q.numel()
    assert torch.equal(q, torch.repeat_interleave(torch.arange(nq), deg)), "dst is not the row index of rowptr"
    inp = torch.cat([y[s], x[q]], dim=-1)                                          # [E, 6]
    if mode != "linear":
        inp = torch.cat([inp, f[s]], dim=-1)
    z = inp @ ws[0].t() + bs[0]                                                    # [E, H]
    dz = (v @ ws[0][:, 3:6].t()).permute(1, 0, 2)[:, q, :]                         # [nd, E, H]: the direction of the edge's query
    z, dz, ddz = _layers(ws, bs, z, dz)
    if mode != "nonlinear_kernelonly":
        z, dz, ddz = z * f[s], dz * f[s][None], ddz * f[s][None]
    c = z.shape[1]
    out = torch.zeros(nq, c, dtype=torch.float64).index_add_(0, q, z)
    d1 = torch.zeros(nd, nq, c, dtype=torch.float64).index_add_(1, q, dz)
    d2 = torch.zeros(nd, nq, c, dtype=torch.float64).index_add_(1, q, ddz)
    inv = torch.where(deg > 0, 1.0 / deg.clamp(min=1).double(), torch.zeros(nq, dtype=torch.float64))
    return out * inv[:, None], d1 * inv[None, :, None], d2 * inv[None, :, None]
