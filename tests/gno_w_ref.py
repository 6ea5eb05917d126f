"""fp64 statement of the WEIGHTED fused GNO transform (the WFwd / WBwd instantiations of csrc/gno.hip, gno_bf16.hip and
gno_bwd3_bf16.hip; gaot_gno_fwd_w / gaot_gno_bwd_w) and of its backward, for an ARBITRARY SIGNED weight per edge:

    k[e]   = MLP(W_0c [y_s, x_q] + b_0 (+ t[s]), ...)               e = (s -> q);  t = f W_0f^T in the two nonlinear modes
    out[q] = sum_{e -> q} alpha[e] * k[e] * f[s]                     ('nonlinear_kernelonly': without f)

With softmax weights a missing factor can hide behind sum alpha = 1; a signed alpha shows it.  The backward is torch autograd of
that statement with t as a leaf, which is how the kernels see it: ``grad_f`` is the alpha g k term alone and ``dt`` the sum of dz_0
over a source's edges (the per-node products through t are the caller's), ``dalpha[e] = sum_c gout[q, c] k[e, c] f[s, c]``.
alpha / dalpha are in the order of the edge list that is passed in.  Works on any device; its teeth: tests/test_gno_weighted_cpu.py."""
from __future__ import annotations

import torch

import gno_nl_ref as _NL
import gno_ref as _G
from gno_ref import rand_graph  # noqa: F401

Tensor = torch.Tensor
MODES = ("linear", "nonlinear", "nonlinear_kernelonly")


def gelu_erf(x: Tensor) -> Tensor:
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def gno_w(mode: str, ws, bs, y: Tensor, x: Tensor, f: Tensor | None, alpha: Tensor, gout: Tensor, src: Tensor, dst: Tensor,
          dtype=torch.float64) -> dict:
    """-> {"out", "grad_f" (None: kernel-only), "dt" (None: linear), "dW0" (the coordinate block), "db0", "dW1".., "db1".., "dalpha"}.
    ws[0] is [H, 2 cd] ('linear') or [H, 2 cd + C_in]; f [n_src, C_in]; alpha [E]; gout [n_dst, C_out]."""
    assert mode in MODES, mode
    cd, nh = y.shape[1], len(ws) - 1
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)  # noqa: E731
    src, dst = src.long(), dst.long()
    y, x, gout = y.detach().to(dtype), x.detach().to(dtype), gout.detach().to(dtype)
    w0 = ws[0].detach().to(dtype)
    w0c = leaf(w0[:, :2 * cd])
    w = [w0c] + [leaf(t) for t in ws[1:]]
    b = [leaf(t) for t in bs]
    a = leaf(alpha)
    fl = leaf(f) if mode != "nonlinear_kernelonly" else None
    t = None
    if mode != "linear":
        assert w0.shape[1] == 2 * cd + f.shape[1]
        t = leaf(f.detach().to(dtype) @ w0[:, 2 * cd:].t())
    else:
        assert w0.shape[1] == 2 * cd
    z = torch.cat([y[src], x[dst]], dim=1) @ w[0].t() + b[0]
    if t is not None:
        z = z + t[src]
    h = gelu_erf(z)
    for l in range(1, nh):
        h = gelu_erf(h @ w[l].t() + b[l])
    k = h @ w[nh].t() + b[nh]
    val = k if fl is None else k * fl[src]
    out = torch.zeros(x.shape[0], k.shape[1], dtype=dtype, device=y.device).index_add(0, dst, a[:, None] * val)
    wanted = [("dalpha", a)] + [(f"dW{l}", w[l]) for l in range(nh + 1)] + [(f"db{l}", b[l]) for l in range(nh + 1)]
    if fl is not None:
        wanted.append(("grad_f", fl))
    if t is not None:
        wanted.append(("dt", t))
    grads = torch.autograd.grad((out * gout).sum(), [v for _, v in wanted], allow_unused=True)
    res = {"out": out.detach(), "grad_f": None, "dt": None}
    for (name, v), gr in zip(wanted, grads):
        res[name] = torch.zeros_like(v) if gr is None else gr
    return res


def w_case(kind: str, mode: str, e: int, nh: int) -> dict:
    """one case on the CPU (fp32): the builders of gno_ref.py ('linear') / gno_nl_ref.py (the nonlinear modes) -- "tail" 40 sources /
    23 queries with one long source row, "mid" 3000 / 700 with a query row of E / 10 edges, a heavy source row and empty rows on both
    sides -- plus a random SIGNED alpha [E] in the order of the case's edge list"""
    c = dict(_G.gno_case(kind, e, nh)) if mode == "linear" else dict(_NL.nl_case(kind, mode, e, nh))
    c["mode"] = mode
    c["tag"] = f"w_{mode}_{kind}_e{e}_nh{nh}"
    c["alpha"] = torch.randn(e, generator=torch.Generator().manual_seed(31 * e + nh + 5))
    return c


def w_ref(case: dict, device="cpu", alpha: Tensor | None = None) -> dict:
    c = case
    mv = lambda t: t.to(device)  # noqa: E731
    return gno_w(c["mode"], [mv(t) for t in c["ws"]], [mv(t) for t in c["bs"]], mv(c["y"]), mv(c["x"]), mv(c["f"]),
                 mv(c["alpha"] if alpha is None else alpha), mv(c["gout"]), mv(c["ei"][0]), mv(c["ei"][1]))


TILE_E = (1, 31, 32, 33, 127, 128, 129)      # around the 16- / 32-edge tiles and the 128-edge workgroup pass of the backward
MID_E = 2003
