"""Closed-form fp64 reference of gaot_gno_fwd_jac: the fused GNO transform on RAGGED rows -- the by-query list (src, dst, rowptr) of any
graph -- and its derivative with respect to the query coordinate, every query's list held fixed.  The per-edge part is
tests/gno_jac_ref.py's (erf-GELU and its exact derivative, no autograd), evaluated edge by edge; a row is the MEAN over its edges and
an empty row is zero in all four planes:
    out_q = (1/deg_q) sum_{e -> q} k_e * f[s_e],   jac_q^d = (1/deg_q) sum_{e -> q} dk_e^d * f[s_e]      (nonlinear_kernelonly: without f)
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gno_jac_ref import _gelu, _gelu_grad  # noqa: E402


def gno_rows_jac(ws, bs, y, x, src, dst, rowptr, f, mode):
    """ws / bs: the kernel MLP's weights [out, in] / biases (layer 0 with its feature columns in the nonlinear modes); y [Ns, 3],
    x [Nq, 3]; src / dst [E]: source and query of every edge, sorted by query; rowptr [Nq + 1]; f [Ns, C]; mode 'linear' /
    'nonlinear' / 'nonlinear_kernelonly'.  -> (out [Nq, C], jac [3, Nq, C]) in fp64."""
    ws = [w.double() for w in ws]
    bs = [b.double() for b in bs]
    y, x, f = y.double(), x.double(), f.double()
    nq = x.shape[0]
    s, q = src.long(), dst.long()
    deg = (rowptr[1:] - rowptr[:-1]).long()
    assert rowptr.numel() == nq + 1 and int(rowptr[-1]) == s.numel() == q.numel()
    assert torch.equal(q, torch.repeat_interleave(torch.arange(nq), deg)), "dst is not the row index of rowptr"
    inp = torch.cat([y[s], x[q]], dim=-1)                                          # [E, 6]
    if mode != "linear":
        inp = torch.cat([inp, f[s]], dim=-1)
    z = inp @ ws[0].t() + bs[0]
    h = _gelu(z)
    dh = _gelu_grad(z)[None] * ws[0][:, 3:6].t()[:, None, :]                       # [3, E, H]
    for w, b in zip(ws[1:-1], bs[1:-1]):
        z = h @ w.t() + b
        h = _gelu(z)
        dh = _gelu_grad(z)[None] * (dh @ w.t())
    kv = h @ ws[-1].t() + bs[-1]                                                   # [E, C]
    dk = dh @ ws[-1].t()                                                           # [3, E, C]
    if mode != "nonlinear_kernelonly":
        kv = kv * f[s]
        dk = dk * f[s][None]
    c = kv.shape[1]
    out = torch.zeros(nq, c, dtype=torch.float64).index_add_(0, q, kv)
    jac = torch.zeros(3, nq, c, dtype=torch.float64).index_add_(1, q, dk)
    inv = torch.where(deg > 0, 1.0 / deg.clamp(min=1).double(), torch.zeros(nq, dtype=torch.float64))
    return out * inv[:, None], jac * inv[None, :, None]


def ragged_list(degrees, nsrc, gen):
    """(src int32 [E], dst int32 [E], rowptr int32 [Nq + 1]) with the given row lengths and random sources (repeats allowed)"""
    deg = torch.as_tensor(degrees, dtype=torch.long)
    rowptr = torch.zeros(deg.numel() + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(deg, 0).to(torch.int32)
    dst = torch.repeat_interleave(torch.arange(deg.numel(), dtype=torch.int32), deg)
    src = torch.randint(0, nsrc, (int(deg.sum()),), generator=gen, dtype=torch.int32)
    return src, dst, rowptr
