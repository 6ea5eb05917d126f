"""fp64 restatement of the sampled field's adjoint, for tests/test_field_adjoint_{cpu,gpu}.py (checker only, plain torch on the CPU):

  * ``gno_linear``: the 'linear' integral transform on a by-query list, out_q = (1/deg q) sum_{e -> q} K(y_s, x_q) * f[s] (empty row: 0);
  * ``gno_adjoint``: its gradient with respect to f for a cotangent g, by autograd of <g, out>;
  * ``gno_adjoint_closed``: the same as the closed form the kernel evaluates, df[t] = sum_{e: src = t} K_e * g[q_e] / deg(q_e);
  * ``decoder_vjp``: the decoder-level vector-Jacobian product with respect to the latent through scale mix and projection, written out
    step by step (projection cotangent dx = ((g W_2) * act'(z)) W_1, scale cotangents w_s dx, one closed-form adjoint per scale).

Everything is float64; the lists are (src, dst, rowptr) with dst ascending, as ``ops.csr_build(edge_index, 1, Nq)`` keeps them."""
import math

import torch


def _f64(t):
    return t.detach().double().cpu()


def kernel_mlp(ws, bs, y, x, src, dst):
    """K [E, C]: the per-edge kernel MLP of [y[src], x[dst]], erf-GELU between the layers"""
    h = torch.cat([y[src.long()], x[dst.long()]], dim=1)
    for i, (w, b) in enumerate(zip(ws, bs)):
        h = h @ w.t() + b
        if i < len(ws) - 1:
            h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
    return h


def _inv_deg(rowptr):
    deg = (rowptr[1:] - rowptr[:-1]).double()
    return torch.where(deg > 0, 1.0 / deg.clamp(min=1.0), torch.zeros_like(deg))


def gno_linear(ws, bs, y, x, src, dst, rowptr, f):
    ws, bs, y, x = [_f64(w) for w in ws], [_f64(b) for b in bs], _f64(y), _f64(x)
    f = f.double()
    k = kernel_mlp(ws, bs, y, x, src, dst) * f[src.long()]
    out = torch.zeros(x.shape[0], k.shape[1], dtype=torch.float64).index_add(0, dst.long(), k)
    return out * _inv_deg(rowptr)[:, None]


def gno_adjoint(ws, bs, y, x, src, dst, rowptr, g, num_src):
    """d <g, gno_linear(f)> / d f by autograd (the transform is linear in f: any f gives the same gradient)"""
    f = torch.zeros(num_src, g.shape[1], dtype=torch.float64, requires_grad=True)
    out = gno_linear(ws, bs, y, x, src, dst, rowptr, f)
    (df,) = torch.autograd.grad((out * _f64(g)).sum(), f)
    return df


def adjoint_terms(ws, bs, y, x, src, dst, rowptr, g):
    """the per-edge terms K_e * g[q_e] / deg(q_e) [E, C] the adjoint sums by source"""
    ws, bs, y, x = [_f64(w) for w in ws], [_f64(b) for b in bs], _f64(y), _f64(x)
    k = kernel_mlp(ws, bs, y, x, src, dst)
    return k * (_f64(g) * _inv_deg(rowptr)[:, None])[dst.long()]


def gno_adjoint_closed(ws, bs, y, x, src, dst, rowptr, g, num_src):
    t = adjoint_terms(ws, bs, y, x, src, dst, rowptr, g)
    return torch.zeros(num_src, t.shape[1], dtype=torch.float64).index_add(0, src.long(), t)


ACT_GRAD = {
    "gelu": lambda z: 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi),
    "relu": lambda z: (z > 0).double(),
}
ACT = {
    "gelu": lambda z: 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0))),
    "relu": lambda z: z.clamp(min=0.0),
}


def decoder_vjp(sd, lists, lat_pos, q, latent, g, use_scale_weights, act="gelu", prefix="decoder."):
    """grad of sum(g * decoder(latent)) with respect to latent [M, C], written out: ``sd`` the model's state dict, ``lists`` one
    (src, dst, rowptr) per scale.  -> (grad_latent [M, C], pred [Nq, out]) in fp64."""
    p = lambda name: _f64(sd[prefix + name])
    w2d = lambda w: w[:, :, 0] if w.dim() == 3 else w
    n = 0
    while f"{prefix}gno.channel_mlp.fcs.{n}.weight" in sd:
        n += 1
    ws = [w2d(p(f"gno.channel_mlp.fcs.{i}.weight")) for i in range(n)]
    bs = [p(f"gno.channel_mlp.fcs.{i}.bias") for i in range(n)]
    lat_pos, q, latent, g = _f64(lat_pos), _f64(q), _f64(latent), _f64(g)
    outs = [gno_linear(ws, bs, lat_pos, q, s, d, r, latent) for s, d, r in lists]
    if len(outs) == 1:
        wts = [torch.ones(q.shape[0], 1, dtype=torch.float64)]
    elif use_scale_weights:
        h = (q @ p("scale_weighting.0.weight").t() + p("scale_weighting.0.bias")).clamp(min=0.0)
        sm = torch.softmax(h @ p("scale_weighting.2.weight").t() + p("scale_weighting.2.bias"), dim=-1)
        wts = [sm[:, s:s + 1] for s in range(len(outs))]
    else:
        wts = [torch.ones(q.shape[0], 1, dtype=torch.float64)] * len(outs)
    x = sum(w * o for w, o in zip(wts, outs))
    w1, b1 = w2d(p("projection.fcs.0.weight")), p("projection.fcs.0.bias")
    w2, b2 = w2d(p("projection.fcs.1.weight")), p("projection.fcs.1.bias")
    z = x @ w1.t() + b1
    pred = ACT[act](z) @ w2.t() + b2
    dx = ((g @ w2) * ACT_GRAD[act](z)) @ w1
    grad = torch.zeros_like(latent)
    for (s, d, r), w in zip(lists, wts):
        grad = grad + gno_adjoint_closed(ws, bs, lat_pos, q, s, d, r, w * dx, latent.shape[0])
    return grad, pred


def random_list(degrees, num_src, gen):
    """a by-query list with the given row lengths and random sources (repeats allowed): (src, dst, rowptr) int32"""
    deg = torch.tensor(list(degrees), dtype=torch.int64)
    rowptr = torch.zeros(deg.numel() + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    e = int(rowptr[-1])
    src = torch.randint(0, num_src, (e,), generator=gen)
    dst = torch.repeat_interleave(torch.arange(deg.numel()), deg)
    return src.int(), dst.int(), rowptr.int()
