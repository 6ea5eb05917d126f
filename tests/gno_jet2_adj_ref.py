"""fp64 restatement of the adjoint of the field's Laplacian, for tests/test_field_laplacian_adjoint_{cpu,gpu}.py (checker only, plain
torch on the CPU; the per-edge recurrences are tests/gno_jet2_ref.py's, the lists and degrees tests/gno_adj_ref.py's):

  * ``kernel_jets2``: K [E, C], D_v K [nd, E, C] and D_v^2 K [nd, E, C] of the per-edge kernel MLP along ``dirs`` in the QUERY coordinate,
    by the closed-form recurrences (erf-GELU with its exact first and second derivative, no autograd);
  * ``adjoint_jet2_closed``: the closed form the kernel evaluates,
        df[t] = sum_{e: src = t} (K_e * G[q_e] + sum_i D_vi K_e * P_i[q_e] + sum_i D_vi^2 K_e * S_i[q_e]) / deg(q_e),
    ``S`` [nd, Nq, C] or [1, Nq, C] (ONE plane for every direction);
  * ``adjoint_jet2_autograd``: the same by torch.autograd.grad of <G, out> + sum_i <P_i, d1_i> + sum_i <S_i, d2_i> through
    ``gno_rows_jet2_ref.gno_rows_jet2`` (value / D_v / D_v^2 planes) with f a leaf;
  * ``gelu_d3``: gelu''' = phi(z) z (z^2 - 4);
  * ``lap_cot_mid``: the elementwise middle of the projection's cotangent, plane by plane;
  * ``decoder_lap_vjp``: the decoder-level product with respect to the latent, written out step by step: the projection cotangent
    one order higher, the scale mix cotangent with the first and second derivatives of the softmax weights, one closed-form adjoint
    per scale along the three axes with one second-order plane.

Everything is float64; the lists are (src, dst, rowptr) with dst ascending."""
import math

import torch

import gno_adj_ref as REF
from gno_jet2_ref import gelu, gelu_d1, gelu_d2
from gno_rows_jet2_ref import gno_rows_jet2

_f64 = REF._f64
AXES = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))


def gelu_d3(z):
    return torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi) * z * (z * z - 4.0)


def kernel_jets2(ws, bs, y, x, src, dst, dirs):
    """(K [E, C], D1 [nd, E, C], D2 [nd, E, C]): the kernel MLP of [y[src], x[dst]] and its first and second directional derivative
    along dirs[i] in x[dst]"""
    ws, bs, y, x = [_f64(w) for w in ws], [_f64(b) for b in bs], _f64(y), _f64(x)
    v = torch.as_tensor(dirs, dtype=torch.float64).reshape(-1, 3)
    s, q = src.long(), dst.long()
    z = torch.cat([y[s], x[q]], dim=-1) @ ws[0].t() + bs[0]
    dz = (v @ ws[0][:, 3:6].t())[:, None, :].expand(v.shape[0], s.numel(), -1)
    ddz = torch.zeros_like(dz)
    for w, b in zip(ws[1:], bs[1:]):
        g1, g2 = gelu_d1(z)[None], gelu_d2(z)[None]
        h, dh, ddh = gelu(z), g1 * dz, g2 * dz * dz + g1 * ddz
        z, dz, ddz = h @ w.t() + b, dh @ w.t(), ddh @ w.t()
    return z, dz, ddz


def adjoint_jet2_terms(ws, bs, y, x, src, dst, rowptr, dirs, g, p, s, jets=None):
    """the per-edge terms (K_e * G[q_e] + sum_i D_vi K_e * P_i[q_e] + sum_i D_vi^2 K_e * S_i[q_e]) / deg(q_e) [E, C] the adjoint sums
    by source (``jets``: the result of ``kernel_jets2`` on these operands, when the caller has it)"""
    k, d1, d2 = jets if jets is not None else kernel_jets2(ws, bs, y, x, src, dst, dirs)
    nd = d1.shape[0]
    g, p, s = _f64(g), _f64(p), _f64(s)
    assert p.shape[0] == nd and s.shape[0] in (1, nd)
    inv = REF._inv_deg(rowptr)[:, None]
    q = dst.long()
    t = k * (g * inv)[q]
    for i in range(nd):
        t = t + d1[i] * (p[i] * inv)[q] + d2[i] * (s[i if s.shape[0] == nd else 0] * inv)[q]
    return t


def adjoint_jet2_closed(ws, bs, y, x, src, dst, rowptr, dirs, g, p, s, num_src, jets=None):
    t = adjoint_jet2_terms(ws, bs, y, x, src, dst, rowptr, dirs, g, p, s, jets)
    return torch.zeros(num_src, t.shape[1], dtype=torch.float64).index_add(0, src.long(), t)


def adjoint_jet2_autograd(ws, bs, y, x, src, dst, rowptr, dirs, g, p, s, num_src):
    """d (<G, out(f)> + sum_i <P_i, d1_i(f)> + sum_i <S_i, d2_i(f)>) / d f through the row-list jet reference"""
    f = torch.zeros(num_src, g.shape[1], dtype=torch.float64, requires_grad=True)
    out, d1, d2 = gno_rows_jet2([_f64(w) for w in ws], [_f64(b) for b in bs], _f64(y), _f64(x), src, dst, rowptr, f, "linear", dirs)
    s = _f64(s)
    loss = (out * _f64(g)).sum() + (d1 * _f64(p)).sum() + (d2 * (s if s.shape[0] == d2.shape[0] else s.expand_as(d2))).sum()
    (df,) = torch.autograd.grad(loss, f)
    return df


def lap_cot_mid(z, u, s, a, ad, al):
    """z [n, h] (WITH its bias), u [3, n, h], s [n, h]; a [n, h] or None, ad [3, n, h], al [n, h] -> [5, n, h] = [dz; du_0; du_1; du_2; ds]"""
    z, u, s, ad, al = _f64(z), _f64(u), _f64(s), _f64(ad), _f64(al)
    a = torch.zeros_like(z) if a is None else _f64(a)
    a1, a2, a3 = gelu_d1(z), gelu_d2(z), gelu_d3(z)
    dz = a1 * a + a2 * (u * ad).sum(0) + (a3 * (u * u).sum(0) + a2 * s) * al
    du = a1 * ad + 2.0 * a2 * u * al
    return torch.cat([dz[None], du, (a1 * al)[None]])


def decoder_lap_vjp(sd, lists, lat_pos, q, latent, gy, gj, gl, use_scale_weights, prefix="decoder."):
    """grad of sum(gy * pred) + sum(gj * jac) + sum(gl * lap) with respect to the latent [M, C], jac[q, o, d] = d pred[q, o] / d q[q, d]
    and lap[q, o] = sum_d d^2 pred[q, o] / d q[q, d]^2 with the lists held fixed, written out: ``sd`` the model's state dict, ``lists``
    one (src, dst, rowptr) per scale, ``gy`` [Nq, out] or None, ``gj`` [Nq, out, 3] or None, ``gl`` [Nq, out].
    -> (grad_latent [M, C], pred [Nq, out], jac [Nq, out, 3], lap [Nq, out]) in fp64."""
    p = lambda name: _f64(sd[prefix + name])
    w2d = lambda w: w[:, :, 0] if w.dim() == 3 else w
    n = 0
    while f"{prefix}gno.channel_mlp.fcs.{n}.weight" in sd:
        n += 1
    ws = [w2d(p(f"gno.channel_mlp.fcs.{i}.weight")) for i in range(n)]
    bs = [p(f"gno.channel_mlp.fcs.{i}.bias") for i in range(n)]
    lat_pos, q, latent, gl = _f64(lat_pos), _f64(q), _f64(latent), _f64(gl)
    nq, ns = q.shape[0], len(lists)
    jets = [gno_rows_jet2(ws, bs, lat_pos, q, s, d, r, latent, "linear", AXES) for s, d, r in lists]      # (o_s, o'_s, o''_s)
    one, zero = torch.ones(nq, 1, dtype=torch.float64), torch.zeros(nq, 1, dtype=torch.float64)
    if ns > 1 and use_scale_weights:
        # w = softmax(l), l = V_2 relu(V_1 q + c_1) + c_2 piecewise linear:  l'_d = V_2 (1[pre > 0] * V_1[:, d]),  l'' = 0,
        # w'_d = w (l'_d - m_d), m_d = sum_t w_t l'_t,d;   w''_d = w'_d (l'_d - m_d) - w sum_t w'_t,d l'_t,d
        v1, c1, v2, c2 = (p("scale_weighting.0.weight"), p("scale_weighting.0.bias"), p("scale_weighting.2.weight"),
                          p("scale_weighting.2.bias"))
        pre = q @ v1.t() + c1
        sm = torch.softmax(pre.clamp(min=0.0) @ v2.t() + c2, dim=-1)
        wts = [sm[:, s:s + 1] for s in range(ns)]
        dwts, ddwts = [], []
        for d in range(3):
            dl = ((pre > 0).double() * v1[:, d]) @ v2.t()
            mean = (sm * dl).sum(-1, keepdim=True)
            dsm = sm * (dl - mean)
            ddsm = dsm * (dl - mean) - sm * (dsm * dl).sum(-1, keepdim=True)
            dwts.append([dsm[:, s:s + 1] for s in range(ns)])
            ddwts.append([ddsm[:, s:s + 1] for s in range(ns)])
    else:
        wts, dwts, ddwts = [one] * ns, [[zero] * ns for _ in range(3)], [[zero] * ns for _ in range(3)]
    x = sum(wts[s] * jets[s][0] for s in range(ns))
    xd = [sum(wts[s] * jets[s][1][d] + dwts[d][s] * jets[s][0] for s in range(ns)) for d in range(3)]
    xdd = sum(sum(wts[s] * jets[s][2][d] + 2.0 * dwts[d][s] * jets[s][1][d] + ddwts[d][s] * jets[s][0] for s in range(ns))
              for d in range(3))
    w1, b1 = w2d(p("projection.fcs.0.weight")), p("projection.fcs.0.bias")
    w2, b2 = w2d(p("projection.fcs.1.weight")), p("projection.fcs.1.bias")
    z = x @ w1.t() + b1
    u = torch.stack([xd[d] @ w1.t() for d in range(3)])
    sv = xdd @ w1.t()
    a1, a2 = gelu_d1(z), gelu_d2(z)
    pred = gelu(z) @ w2.t() + b2
    jac = torch.stack([(a1 * u[d]) @ w2.t() for d in range(3)], dim=-1)
    lap = (a2 * (u * u).sum(0) + a1 * sv) @ w2.t()
    a = None if gy is None else _f64(gy) @ w2
    ad = torch.stack([(torch.zeros_like(gl) if gj is None else _f64(gj)[:, :, d]) @ w2 for d in range(3)])
    mid = lap_cot_mid(z, u, sv, a, ad, gl @ w2)
    dx, dxd, dxdd = mid[0] @ w1, [mid[1 + d] @ w1 for d in range(3)], mid[4] @ w1
    lw = [sum(ddwts[d][s] for d in range(3)) for s in range(ns)]
    grad = torch.zeros_like(latent)
    for s, (src, dst, rowptr) in enumerate(lists):
        g_s = wts[s] * dx + sum(dwts[d][s] * dxd[d] for d in range(3)) + lw[s] * dxdd
        p_s = torch.stack([wts[s] * dxd[d] + 2.0 * dwts[d][s] * dxdd for d in range(3)])
        grad = grad + adjoint_jet2_closed(ws, bs, lat_pos, q, src, dst, rowptr, AXES, g_s, p_s, (wts[s] * dxdd)[None], latent.shape[0])
    return grad, pred, jac, lap
