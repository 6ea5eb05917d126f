"""fp64 restatement of the adjoint of the field's Jacobian, for tests/test_field_jacobian_adjoint_{cpu,gpu}.py (checker only, plain
torch on the CPU; the pieces it shares with the value adjoint come from tests/gno_adj_ref.py):

  * ``kernel_jets``: K [E, C] and d_d K [3, E, C], the per-edge kernel MLP and its derivative in the QUERY coordinate d, by autograd
    of ``gno_adj_ref.kernel_mlp`` on a per-edge copy of the query rows;
  * ``gno_linear_jets``: out_q = (1/deg q) sum_e K_e f[s_e] and jac_q^d = (1/deg q) sum_e d_d K_e f[s_e] from those;
  * ``adjoint_jac_closed``: the closed form the kernel evaluates,
        df[t] = sum_{e: src = t} (K_e * G[q_e] + sum_d d_d K_e * J_d[q_e]) / deg(q_e);
  * ``adjoint_jac_autograd``: the same by torch.autograd.grad of <G, out> + sum_d <J_d, jac_d>, with jac_d a ``create_graph=True``
    derivative of the transform in x (``gno_adj_ref.gno_linear`` detaches its operands, so the transform is restated from
    ``kernel_mlp`` with x attached);
  * ``decoder_jac_vjp``: the decoder-level product with respect to the latent, written out step by step: the projection cotangent with
    act'', the scale mix cotangent with the tangents of the softmax weights, one closed-form adjoint per scale.

Everything is float64; the lists are (src, dst, rowptr) with dst ascending."""
import math

import torch

import gno_adj_ref as REF

_f64 = REF._f64


def kernel_jets(ws, bs, y, x, src, dst):
    """(K [E, C], dK [3, E, C]) with dK[d, e, c] = d K[e, c] / d x[dst_e, d]"""
    ws, bs, y, x = [_f64(w) for w in ws], [_f64(b) for b in bs], _f64(y), _f64(x)
    xe = x[dst.long()].clone()
    e = xe.shape[0]
    fn = lambda xq: REF.kernel_mlp(ws, bs, y, xq, src, torch.arange(e))
    dk = []
    for d in range(3):                                  # edge e's kernel depends on row e of xe alone: one tangent per axis
        v = torch.zeros_like(xe)
        v[:, d] = 1.0
        k, t = torch.autograd.functional.jvp(fn, xe, v)
        dk.append(t.detach())
    return k.detach(), torch.stack(dk)


def gno_linear_jets(ws, bs, y, x, src, dst, rowptr, f):
    """(out [Nq, C], jac [3, Nq, C]) of the 'linear' transform, the lists held fixed"""
    k, dk = kernel_jets(ws, bs, y, x, src, dst)
    fs = _f64(f)[src.long()]
    inv = REF._inv_deg(rowptr)[:, None]
    nq = _f64(x).shape[0]
    red = lambda t: torch.zeros(nq, t.shape[1], dtype=torch.float64).index_add(0, dst.long(), t) * inv
    return red(k * fs), torch.stack([red(dk[d] * fs) for d in range(3)])


def adjoint_jac_terms(ws, bs, y, x, src, dst, rowptr, g, gj, jets=None):
    """the per-edge terms (K_e * G[q_e] + sum_d d_d K_e * J_d[q_e]) / deg(q_e) [E, C] the adjoint sums by source (``jets``: the
    result of ``kernel_jets`` on these operands, when the caller has it)"""
    k, dk = jets if jets is not None else kernel_jets(ws, bs, y, x, src, dst)
    inv = REF._inv_deg(rowptr)[:, None]
    t = k * (_f64(g) * inv)[dst.long()]
    for d in range(3):
        t = t + dk[d] * (_f64(gj[d]) * inv)[dst.long()]
    return t


def adjoint_jac_closed(ws, bs, y, x, src, dst, rowptr, g, gj, num_src, jets=None):
    t = adjoint_jac_terms(ws, bs, y, x, src, dst, rowptr, g, gj, jets)
    return torch.zeros(num_src, t.shape[1], dtype=torch.float64).index_add(0, src.long(), t)


def adjoint_jac_autograd(ws, bs, y, x, src, dst, rowptr, g, gj, num_src):
    """d (<G, out(f)> + sum_d <J_d, jac_d(f)>) / d f with jac_d = d out / d x_d by a create_graph=True derivative"""
    ws, bs, y = [_f64(w) for w in ws], [_f64(b) for b in bs], _f64(y)
    xg = _f64(x).requires_grad_(True)
    f = torch.zeros(num_src, g.shape[1], dtype=torch.float64, requires_grad=True)
    k = REF.kernel_mlp(ws, bs, y, xg, src, dst) * f[src.long()]
    out = torch.zeros(xg.shape[0], k.shape[1], dtype=torch.float64).index_add(0, dst.long(), k) * REF._inv_deg(rowptr)[:, None]
    loss = (out * _f64(g)).sum()
    for c in range(out.shape[1]):
        (dx,) = torch.autograd.grad(out[:, c].sum(), xg, create_graph=True)     # [Nq, 3]: out[q, c] depends on x[q] alone
        loss = loss + (dx * _f64(gj)[:, :, c].t()).sum()
    (df,) = torch.autograd.grad(loss, f)
    return df


ACT = REF.ACT
ACT_GRAD = REF.ACT_GRAD
ACT_GRAD2 = {
    "gelu": lambda z: torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi) * (2.0 - z * z),
    "relu": lambda z: torch.zeros_like(z),
}


def decoder_jac_vjp(sd, lists, lat_pos, q, latent, gy, gj, use_scale_weights, act="gelu", prefix="decoder."):
    """grad of sum(gy * pred) + sum(gj * jac) with respect to the latent [M, C], jac[q, o, d] = d pred[q, o] / d q[q, d] with the lists
    held fixed, written out: ``sd`` the model's state dict, ``lists`` one (src, dst, rowptr) per scale, ``gy`` [Nq, out] or None,
    ``gj`` [Nq, out, 3].  -> (grad_latent [M, C], pred [Nq, out], jac [Nq, out, 3]) in fp64."""
    p = lambda name: _f64(sd[prefix + name])
    w2d = lambda w: w[:, :, 0] if w.dim() == 3 else w
    n = 0
    while f"{prefix}gno.channel_mlp.fcs.{n}.weight" in sd:
        n += 1
    ws = [w2d(p(f"gno.channel_mlp.fcs.{i}.weight")) for i in range(n)]
    bs = [p(f"gno.channel_mlp.fcs.{i}.bias") for i in range(n)]
    lat_pos, q, latent, gj = _f64(lat_pos), _f64(q), _f64(latent), _f64(gj)
    nq, ns = q.shape[0], len(lists)
    jets = [gno_linear_jets(ws, bs, lat_pos, q, s, d, r, latent) for s, d, r in lists]       # (o_s, o'_s)
    one, zero = torch.ones(nq, 1, dtype=torch.float64), torch.zeros(nq, 1, dtype=torch.float64)
    if ns > 1 and use_scale_weights:
        # w = softmax(l), l = V_2 relu(V_1 q + c_1) + c_2:  d_d l = V_2 (1[pre > 0] * V_1[:, d]),  w'_s,d = w_s (d_d l_s - sum_t w_t d_d l_t)
        v1, c1, v2, c2 = (p("scale_weighting.0.weight"), p("scale_weighting.0.bias"), p("scale_weighting.2.weight"),
                          p("scale_weighting.2.bias"))
        pre = q @ v1.t() + c1
        sm = torch.softmax(pre.clamp(min=0.0) @ v2.t() + c2, dim=-1)
        wts = [sm[:, s:s + 1] for s in range(ns)]
        dwts = []
        for d in range(3):
            dl = ((pre > 0).double() * v1[:, d]) @ v2.t()
            dsm = sm * (dl - (sm * dl).sum(-1, keepdim=True))
            dwts.append([dsm[:, s:s + 1] for s in range(ns)])
    else:
        wts, dwts = [one] * ns, [[zero] * ns for _ in range(3)]
    x = sum(w * o for w, (o, _) in zip(wts, jets))
    xd = [sum(wts[s] * jets[s][1][d] + dwts[d][s] * jets[s][0] for s in range(ns)) for d in range(3)]
    w1, b1 = w2d(p("projection.fcs.0.weight")), p("projection.fcs.0.bias")
    w2, b2 = w2d(p("projection.fcs.1.weight")), p("projection.fcs.1.bias")
    z = x @ w1.t() + b1
    a1, a2 = ACT_GRAD[act](z), ACT_GRAD2[act](z)
    u = [xd[d] @ w1.t() for d in range(3)]
    pred = ACT[act](z) @ w2.t() + b2
    jac = torch.stack([(a1 * u[d]) @ w2.t() for d in range(3)], dim=-1)
    # the projection's cotangent: a = g_y W_2, a_d = g_y'd W_2, dz = act' a + act'' sum_d u_d a_d, du_d = act' a_d
    a = torch.zeros_like(z) if gy is None else _f64(gy) @ w2
    ad = [gj[:, :, d] @ w2 for d in range(3)]
    dx = (a1 * a + a2 * sum(u[d] * ad[d] for d in range(3))) @ w1
    dxd = [(a1 * ad[d]) @ w1 for d in range(3)]
    grad = torch.zeros_like(latent)
    for s, (src, dst, rowptr) in enumerate(lists):
        g_s = wts[s] * dx + sum(dwts[d][s] * dxd[d] for d in range(3))
        j_s = torch.stack([wts[s] * dxd[d] for d in range(3)])
        grad = grad + adjoint_jac_closed(ws, bs, lat_pos, q, src, dst, rowptr, g_s, j_s, latent.shape[0])
    return grad, pred, jac
