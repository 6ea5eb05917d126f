"""fp64 restatement of the adjoint of the field's directional derivatives and Hessian, for
tests/test_field_directional_adjoint_{cpu,gpu}.py (checker only, plain torch on the CPU; the per-edge recurrences are
tests/gno_qdir_jet2_ref.py's, the lists and degrees tests/gno_adj_ref.py's):

  * ``kernel_jets2_qd``: K [E, C], D_v K [nd, E, C] and D_v^2 K [nd, E, C] of the per-edge kernel MLP along the directions of the EDGE'S
    QUERY, v = qdirs[q_e, i], by the closed-form recurrences (no autograd);
  * ``adjoint_jet2_qd_closed``: the closed form gaot_gno_adj_jet2_qd evaluates,
        df[t] = sum_{e: src = t} (K_e * G[q_e] + sum_i D_vi(q_e) K_e * P_i[q_e] + sum_i D^2_vi(q_e) K_e * S_i[q_e]) / deg(q_e),
    ``S`` [nd, Nq, C] or [1, Nq, C] (ONE plane for every direction);
  * ``adjoint_jet2_qd_autograd``: the same by torch.autograd.grad through ``gno_qdir_jet2_ref.gno_rows_jet2_qd`` with f a leaf;
  * ``jet2_cot_mid``: the elementwise middle of the projection's cotangent with a second-order cotangent per direction;
  * ``polarise`` / ``hessian_cot``: ``MAGNODecoder._polarise``'s expression and its transpose, the map of (cot_jac, cot_hess) to the
    cotangents of the jets along the six directions;
  * ``decoder_dir_vjp``: the decoder-level product with respect to the latent along per-query directions, step by step.

Everything is float64; the lists are (src, dst, rowptr) with dst ascending."""
import torch

import gno_adj_ref as REF
from gno_jet2_adj_ref import gelu_d3
from gno_jet2_ref import gelu, gelu_d1, gelu_d2
from gno_qdir_jet2_ref import _layers, gno_rows_jet2_qd

_f64 = REF._f64
HESSIAN_DIRS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 1.0, 0.0), (0.0, 1.0, 1.0), (1.0, 0.0, 1.0))
HESSIAN_PAIRS = ((0, 1), (1, 2), (0, 2))


def kernel_jets2_qd(ws, bs, y, x, src, dst, qdirs):
    ws, bs, y, x = [_f64(w) for w in ws], [_f64(b) for b in bs], _f64(y), _f64(x)
    v = _f64(torch.as_tensor(qdirs))
    s, q = src.long(), dst.long()
    z = torch.cat([y[s], x[q]], dim=-1) @ ws[0].t() + bs[0]
    dz = (v @ ws[0][:, 3:6].t()).permute(1, 0, 2)[:, q, :]               # [nd, E, H]: the direction of the edge's query
    return _layers(ws, bs, z, dz)


def adjoint_jet2_qd_closed(ws, bs, y, x, src, dst, rowptr, qdirs, g, p, s, num_src):
    k, d1, d2 = kernel_jets2_qd(ws, bs, y, x, src, dst, qdirs)
    nd = d1.shape[0]
    g, p, s = _f64(g), _f64(p), _f64(s)
    assert p.shape[0] == nd and s.shape[0] in (1, nd)
    inv = REF._inv_deg(rowptr)[:, None]
    q = dst.long()
    t = k * (g * inv)[q]
    for i in range(nd):
        t = t + d1[i] * (p[i] * inv)[q] + d2[i] * (s[i if s.shape[0] == nd else 0] * inv)[q]
    return torch.zeros(num_src, t.shape[1], dtype=torch.float64).index_add(0, src.long(), t)


def adjoint_jet2_qd_autograd(ws, bs, y, x, src, dst, rowptr, qdirs, g, p, s, num_src):
    f = torch.zeros(num_src, g.shape[1], dtype=torch.float64, requires_grad=True)
    out, d1, d2 = gno_rows_jet2_qd([_f64(w) for w in ws], [_f64(b) for b in bs], _f64(y), _f64(x), src, dst, rowptr, f, "linear", qdirs)
    s = _f64(s)
    loss = (out * _f64(g)).sum() + (d1 * _f64(p)).sum() + (d2 * (s if s.shape[0] == d2.shape[0] else s.expand_as(d2))).sum()
    (df,) = torch.autograd.grad(loss, f)
    return df


def jet2_cot_mid(z, u, s, a, ad, bd):
    """z [n, h] (WITH its bias), u / s [nd, n, h]; a [n, h] or None, ad / bd [nd, n, h] -> [1 + 2 nd, n, h] = [dz; du_i ...; ds_i ...]"""
    z, u, s, ad, bd = _f64(z), _f64(u), _f64(s), _f64(ad), _f64(bd)
    a = torch.zeros_like(z) if a is None else _f64(a)
    a1, a2, a3 = gelu_d1(z), gelu_d2(z), gelu_d3(z)
    dz = a1 * a + a2 * (u * ad).sum(0) + ((a3 * u * u + a2 * s) * bd).sum(0)
    return torch.cat([dz[None], a1 * ad + 2.0 * a2 * u * bd, a1 * bd])


def polarise(d1, d2):
    """``MAGNODecoder._polarise`` as an expression: d1 / d2 [n, out, 6] along HESSIAN_DIRS -> (jac [n, out, 3], hess [n, out, 3, 3])"""
    hess = [[None] * 3 for _ in range(3)]
    for a in range(3):
        hess[a][a] = d2[:, :, a]
    for n, (a, b) in enumerate(HESSIAN_PAIRS):
        hess[a][b] = hess[b][a] = 0.5 * (d2[:, :, 3 + n] - d2[:, :, a] - d2[:, :, b])
    return d1[:, :, :3], torch.stack([torch.stack(row, dim=-1) for row in hess], dim=-2)


def hessian_cot(cot_jac, cot_hess):
    """the transpose of ``polarise``, written out: with Cs = (C + C^T) / 2,  P_a = cot_jac_a, P_{3+n} = 0,
    S_a = C_aa - sum_{b != a} Cs_ab,  S_{3+n} = Cs_ab for pair n = (a, b)  -> (P, S) [n, out, 6]"""
    cj, ch = _f64(cot_jac), _f64(cot_hess)
    p = torch.cat([cj, torch.zeros_like(cj)], dim=-1)
    sym = 0.5 * (ch + ch.transpose(2, 3))
    diag = [sym[:, :, a, a] - sum(sym[:, :, a, b] for b in range(3) if b != a) for a in range(3)]
    return p, torch.stack(diag + [sym[:, :, a, b] for a, b in HESSIAN_PAIRS], dim=-1)


def decoder_dir_vjp(sd, lists, lat_pos, q, latent, qdirs, gy, g1, g2, use_scale_weights, prefix="decoder."):
    """grad of sum(gy * pred) + sum(g1 * d1) + sum(g2 * d2) with respect to the latent [M, C], d1[q, o, i] / d2[q, o, i] the first and
    second derivative of pred[q, o] along qdirs[q, i] with the lists held fixed, written out: ``sd`` the model's state dict, ``lists``
    one (src, dst, rowptr) per scale, ``qdirs`` [Nq, nd, 3], ``gy`` [Nq, out] or None, ``g1`` / ``g2`` [Nq, out, nd] or None.
    -> (grad_latent [M, C], pred [Nq, out], d1 [Nq, out, nd], d2 [Nq, out, nd]) in fp64."""
    p = lambda name: _f64(sd[prefix + name])
    w2d = lambda w: w[:, :, 0] if w.dim() == 3 else w
    n = 0
    while f"{prefix}gno.channel_mlp.fcs.{n}.weight" in sd:
        n += 1
    ws = [w2d(p(f"gno.channel_mlp.fcs.{i}.weight")) for i in range(n)]
    bs = [p(f"gno.channel_mlp.fcs.{i}.bias") for i in range(n)]
    lat_pos, q, latent, v = _f64(lat_pos), _f64(q), _f64(latent), _f64(qdirs)
    nq, ns, nd = q.shape[0], len(lists), v.shape[1]
    jets = [gno_rows_jet2_qd(ws, bs, lat_pos, q, s, d, r, latent, "linear", v) for s, d, r in lists]      # (o_s, o'_s, o''_s)
    one, zero = torch.ones(nq, 1, dtype=torch.float64), torch.zeros(nq, 1, dtype=torch.float64)
    if ns > 1 and use_scale_weights:
        # w = softmax(l), l = V_2 relu(V_1 q + c_1) + c_2 piecewise linear: along v, l' = V_2 (1[pre > 0] * V_1 v), l'' = 0,
        # w' = w (l' - m), m = sum_t w_t l'_t;   w'' = w' (l' - m) - w sum_t w'_t l'_t
        v1, c1, v2, c2 = (p("scale_weighting.0.weight"), p("scale_weighting.0.bias"), p("scale_weighting.2.weight"),
                          p("scale_weighting.2.bias"))
        pre = q @ v1.t() + c1
        sm = torch.softmax(pre.clamp(min=0.0) @ v2.t() + c2, dim=-1)
        wts = [sm[:, s:s + 1] for s in range(ns)]
        dwts, ddwts = [], []
        for i in range(nd):
            dl = ((pre > 0).double() * (v[:, i] @ v1.t())) @ v2.t()
            mean = (sm * dl).sum(-1, keepdim=True)
            dsm = sm * (dl - mean)
            ddsm = dsm * (dl - mean) - sm * (dsm * dl).sum(-1, keepdim=True)
            dwts.append([dsm[:, s:s + 1] for s in range(ns)])
            ddwts.append([ddsm[:, s:s + 1] for s in range(ns)])
    else:
        wts, dwts, ddwts = [one] * ns, [[zero] * ns for _ in range(nd)], [[zero] * ns for _ in range(nd)]
    x = sum(wts[s] * jets[s][0] for s in range(ns))
    xd = [sum(wts[s] * jets[s][1][i] + dwts[i][s] * jets[s][0] for s in range(ns)) for i in range(nd)]
    xdd = [sum(wts[s] * jets[s][2][i] + 2.0 * dwts[i][s] * jets[s][1][i] + ddwts[i][s] * jets[s][0] for s in range(ns))
           for i in range(nd)]
    w1, b1 = w2d(p("projection.fcs.0.weight")), p("projection.fcs.0.bias")
    w2, b2 = w2d(p("projection.fcs.1.weight")), p("projection.fcs.1.bias")
    z = x @ w1.t() + b1
    u = torch.stack([xd[i] @ w1.t() for i in range(nd)])
    sv = torch.stack([xdd[i] @ w1.t() for i in range(nd)])
    a1, a2 = gelu_d1(z), gelu_d2(z)
    pred = gelu(z) @ w2.t() + b2
    d1 = torch.stack([(a1 * u[i]) @ w2.t() for i in range(nd)], dim=-1)
    d2 = torch.stack([(a2 * u[i] * u[i] + a1 * sv[i]) @ w2.t() for i in range(nd)], dim=-1)
    zeros = torch.zeros(nq, pred.shape[1], nd, dtype=torch.float64)
    g1 = zeros if g1 is None else _f64(g1)
    g2 = zeros if g2 is None else _f64(g2)
    a = None if gy is None else _f64(gy) @ w2
    mid = jet2_cot_mid(z, u, sv, a, torch.stack([g1[:, :, i] @ w2 for i in range(nd)]), torch.stack([g2[:, :, i] @ w2 for i in range(nd)]))
    dx, dxd, dxdd = mid[0] @ w1, [mid[1 + i] @ w1 for i in range(nd)], [mid[1 + nd + i] @ w1 for i in range(nd)]
    grad = torch.zeros_like(latent)
    for s, (src, dst, rowptr) in enumerate(lists):
        g_s = wts[s] * dx + sum(dwts[i][s] * dxd[i] + ddwts[i][s] * dxdd[i] for i in range(nd))
        p_s = torch.stack([wts[s] * dxd[i] + 2.0 * dwts[i][s] * dxdd[i] for i in range(nd)])
        s_s = torch.stack([wts[s] * dxdd[i] for i in range(nd)])
        grad = grad + adjoint_jet2_qd_closed(ws, bs, lat_pos, q, src, dst, rowptr, v, g_s, p_s, s_s, latent.shape[0])
    return grad, pred, d1, d2


def decoder_hess_vjp(sd, lists, lat_pos, q, latent, gy, gj, gh, use_scale_weights, prefix="decoder."):
    """``decoder_dir_vjp`` along HESSIAN_DIRS on every query with the cotangents through ``hessian_cot`` -> (grad_latent, pred,
    jac [Nq, out, 3], hess [Nq, out, 3, 3]); ``gj`` [Nq, out, 3] / ``gh`` [Nq, out, 3, 3] or None"""
    nq = q.shape[0]
    v = torch.tensor(HESSIAN_DIRS, dtype=torch.float64)[None].expand(nq, 6, 3)
    oc = _f64(sd[prefix + "projection.fcs.1.weight"]).shape[0]
    cj = torch.zeros(nq, oc, 3, dtype=torch.float64) if gj is None else gj
    ch = torch.zeros(nq, oc, 3, 3, dtype=torch.float64) if gh is None else gh
    g1, g2 = hessian_cot(cj, ch)
    grad, pred, d1, d2 = decoder_dir_vjp(sd, lists, lat_pos, q, latent, v, gy, g1, g2, use_scale_weights, prefix)
    return (grad, pred, *polarise(d1, d2))
