"""Restatement of the bf16 GNO integral transform (csrc/gno_bf16.hip, csrc/gno_bwd3_bf16.hip) and of the fused projection MLP
(csrc/mlp2.hip) in three forms, and the cases of tests/test_gno_bf16_fp64_gpu.py (their teeth: tests/test_gno_ref_cpu.py).

  E  the exact form: fp64, erf-GELU, nothing rounded (equal to oracle/gaot_oracle.py's integral_transform and its autograd).
  R  the rounding model: fp64 arithmetic, values rounded exactly where the kernels round them, the kernels' polynomial GELU.
  F  an fp32 realisation of R: the same rounding points, every product and sum in fp32, contractions in 16-wide chunks taken in a
     shuffled order, the edges (rows) shuffled; ``seed`` picks the shuffle.  F samples how far a correct fp32-accumulating
     implementation lands from R, one-ulp bf16 flips at rounding boundaries included.

A kernel result is accepted by Report.model (block_ref.py): rms(got - R) <= 1/4 rms(R - E) and max|got - R| <= 2 max|R - E|, exact
zeros where R = E = 0.  The yardstick R - E is the model's own bf16 error; nothing in the rule comes from the kernel.

Rounding points of the GNO (G = the polynomial GELU of csrc/common.h:149-187, gelu_e2_2 / gelu_e2_pair2):
  forward (gno_bf16.hip)
    z_0 = W_0 [y_s, x_q] + b_0 in fp32 on the exact-fp32 MFMA (:186-196), h_0 = bf16(G(z_0)) (:198-205, to_frags :25-31)
    z_l = bf16(W_l) h_{l-1} + b_l (images :79-87, products :209-228), h_l = bf16(G(z_l)) (:230-239), l = 1..NH-1
    k = bf16(W_NH) h_{NH-1} + b_NH (:89-94, :245-254), k * f[s] in fp32 (:256-265), row mean = sum / deg (gno_common.h segment_walk)
  backward (gno_bwd3_bf16.hip; gs = grad_out / deg: gno.hip k_scale_by_inv_deg)
    h_l as in the forward (activate :308-326, frag_of :41-43); gp_l = G'(z_l) rounded toward zero to f16 (cvt_pkrtz :318)
    grad_f[s] += gs k, both fp32 (:378); dk = bf16(gs f[s]) (:414-416)
    dz_{NH-1} = (bf16(W_NH)^T dk) gp_{NH-1} (:422-434); dz_{l-1} = (bf16(W_l)^T bf16(dz_l)) gp_{l-1} (:437-458; images :126-150)
    per-edge coordinate gradient W_0^T dz_0 from the unrounded dz_0 and the fp32 W_0 (:460-479)
    dW_NH = sum_e dk h_{NH-1}^T, db_NH = sum_e dk (:499-503); dW_l = sum_e bf16(dz_l) h_{l-1}^T, db_l = sum_e bf16(dz_l) (:488-497)
    dW_0 = sum_e bf16(dz_0) bf16([y_s, x_q])^T -- the coordinates are rounded here only (:258-260) -- db_0 = sum_e bf16(dz_0) (:482, :505-511)
Rounding points of the projection MLP (mlp2.hip)
    z = bf16(x) bf16(W1)^T + b1 (stage_x :31-49, w1_frag :52-59), h = G(z) and out = h W2^T + b2 in fp32 (:106-128)
    dz = (dout W2) G'(z) in fp32 (:219-231); dW2 = dout^T h, db1 = sum dz unrounded (:227-234)
    dW1 = bf16(dz)^T bf16(x) (:235-238), dx = bf16(dz) bf16(W1) (:243-249)
Works on any device: the GPU test computes R and E on the GPU, the CPU test and ``python tests/gno_ref.py`` (the floor table of
profiles/gno_bf16_fp64_parity.txt) on the CPU."""
from __future__ import annotations

import math

import torch

Tensor = torch.Tensor

# ---- the polynomial GELU of csrc/common.h, restated (tests/test_gno_ref_cpu.py compares these with the header) ---------------------
GELU_A_MAX = 5.5
GELU_P = (-1.000106314, -1.149296311, -0.465028396, -0.04579698, 0.004187508)
_LN2 = 0.6931471805599453


def _f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float32))


_P32 = tuple(_f32(p) for p in GELU_P)                                                    # the header's float literals
_Q32 = (1.0,) + tuple(_f32(_LN2 * float(k) * GELU_P[k]) for k in range(1, 5))            # (float)(ln 2 * k * P_k)


def gelu_poly(x: Tensor):
    """-> (G, G'): a = min(|x|, 5.5), t = 2^P(a), G = max(x, 0) - a t, G' = 1/2 + sign(x) (1/2 - t Q(a)), in x's dtype"""
    a = x.abs().clamp(max=GELU_A_MAX)
    p = a * _P32[4] + _P32[3]
    q = a * _Q32[4] + _Q32[3]
    for k in (2, 1, 0):
        p = a * p + _P32[k]
        q = a * q + _Q32[k]
    t = torch.exp2(p)
    return x.clamp(min=0) - a * t, torch.copysign(0.5 - t * q, x) + 0.5


def gelu_erf(x: Tensor):
    """-> (gelu, gelu') of the erf form"""
    cdf = 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))
    return x * cdf, cdf + x * torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))


def rb(t: Tensor) -> Tensor:
    """round to bf16 (nearest even), back to t's dtype"""
    return t.to(torch.bfloat16).to(t.dtype)


def trunc_bf16(t: Tensor) -> Tensor:
    """truncate to bf16 (what a kernel that drops the low half of the fp32 word does)"""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(t.dtype)


def rtz_f16(t: Tensor) -> Tensor:
    """round toward zero to f16: the low 13 mantissa bits of the fp32 value cleared (below 2^-14, f16's subnormals, within 2^-24)"""
    return (t.float().contiguous().view(torch.int32) & -8192).view(torch.float32).to(t.dtype)


class _Arith:
    """the arithmetic of one form: dtype, rounding on / off, the activation, and the products"""
    BLOCK = 1 << 15     # edges (rows) per pass: bounds the memory of the per-edge tensors

    def __init__(self, form: str, seed: int, gelu: str | None = None, rounding: bool | None = None):
        assert form in ("E", "R", "F"), form
        self.form = form
        self.dt = torch.float32 if form == "F" else torch.float64
        self.rounding = (form != "E") if rounding is None else rounding
        self.act = {"erf": gelu_erf, "poly": gelu_poly}[gelu or ("erf" if form == "E" else "poly")]
        self.gen = torch.Generator().manual_seed(1000 + seed) if form == "F" else None

    def rb(self, t):
        return rb(t) if self.rounding else t

    def rtz(self, t):
        return rtz_f16(t) if self.rounding else t

    def order(self, n: int, device) -> Tensor:
        """the order the edges (rows) are visited in: shuffled for F"""
        return torch.randperm(n, generator=self.gen).to(device) if self.form == "F" else torch.arange(n, device=device)

    def mm(self, a: Tensor, w: Tensor, bias: Tensor | None = None) -> Tensor:
        """a [n, K] @ w [K, m] (+ bias, the accumulator's start value); F: 16-wide chunks of K in a shuffled order"""
        k = a.shape[1]
        if self.form != "F" or k <= 16:
            out = a @ w
            return out if bias is None else bias + out
        acc = None if bias is None else bias.expand(a.shape[0], -1)
        for c in torch.randperm(k // 16, generator=self.gen).tolist():
            part = a[:, 16 * c:16 * c + 16] @ w[16 * c:16 * c + 16]
            acc = part if acc is None else acc + part
        return acc

    def rows(self, a: Tensor, b: Tensor) -> Tensor:
        """a^T b over the rows (a weight gradient); F: fp32 partial products of 16 rows each, then summed"""
        if self.form != "F":
            return a.t() @ b
        n = a.shape[0]
        pad = (-n) % 16
        if pad:
            a = torch.cat([a, a.new_zeros(pad, a.shape[1])])
            b = torch.cat([b, b.new_zeros(pad, b.shape[1])])
        return torch.bmm(a.view(-1, 16, a.shape[1]).transpose(1, 2), b.view(-1, 16, b.shape[1])).sum(0)


def gno(form: str, ws, bs, y: Tensor, x: Tensor, f: Tensor, gout: Tensor, src: Tensor, dst: Tensor, seed: int = 0,
        gelu: str | None = None, rounding: bool | None = None, damage: dict | None = None) -> dict:
    """the GNO integral transform and its backward in one form -> {"out", "grad_f", "dW0".., "db0".., "grad_y", "grad_x"}.
    ws / bs: the kernel MLP ([64, 6], [64, 64] x (NH - 1), [32, 64]); y [n_src, 3], x [n_dst, 3], f [n_src, 32], gout [n_dst, 32];
    src / dst: the edge list.  ``gelu`` / ``rounding`` override the form's activation and rounding (R without rounding and with
    erf-GELU is E).  ``damage`` (test_gno_ref_cpu.py only) plants a fault a kernel could have:
      "deg": the degrees to divide by (the edge list given lacks an edge the degrees still count)
      "round_h": what replaces the bf16 rounding of h_l
      "dk_scale": [n_dst] factor on gs inside dk alone
      "swap_tile": the 16-edge tile (list order) whose dW_0 terms see [x_q, y_s] for [y_s, x_q]"""
    ar = _Arith(form, seed, gelu, rounding)
    dt, dev = ar.dt, y.device
    damage = damage or {}
    nh = len(ws) - 1
    n_src, n_dst, ne = y.shape[0], x.shape[0], int(src.shape[0])
    src, dst = src.long().to(dev), dst.long().to(dev)
    w0 = ws[0].detach().to(dt)
    w = [w0] + [ar.rb(wl.detach().to(dt)) for wl in ws[1:]]
    b = [bl.detach().to(dt) for bl in bs]
    y, x, f, gout = (t.detach().to(dt) for t in (y, x, f, gout))
    deg = damage.get("deg")
    if deg is None:
        deg = torch.bincount(dst, minlength=n_dst)
    degf = deg.to(dt)
    inv = torch.where(deg > 0, 1.0 / degf.clamp(min=1), torch.zeros_like(degf))
    gs = gout * inv[:, None]
    round_h = damage.get("round_h", ar.rb)
    dk_scale = damage.get("dk_scale")
    swap_tile = damage.get("swap_tile")

    res = {"out": torch.zeros(n_dst, 32, dtype=dt, device=dev), "grad_f": torch.zeros(n_src, 32, dtype=dt, device=dev),
           "grad_y": torch.zeros(n_src, 3, dtype=dt, device=dev), "grad_x": torch.zeros(n_dst, 3, dtype=dt, device=dev)}
    for l in range(nh + 1):
        res[f"dW{l}"] = torch.zeros_like(w[l])
        res[f"db{l}"] = torch.zeros_like(b[l])
    order = ar.order(ne, dev)
    for lo in range(0, ne, ar.BLOCK):
        idx = order[lo:lo + ar.BLOCK]
        s, q = src[idx], dst[idx]
        cin = torch.cat([y[s], x[q]], dim=1)
        # ---- the kernel MLP -----------------------------------------------------------------------------------------------------
        hs, gps = [], []
        z = ar.mm(cin, w[0].t(), b[0])
        for l in range(nh):
            if l > 0:
                z = ar.mm(hs[-1], w[l].t(), b[l])
            g, gp = ar.act(z)
            hs.append(round_h(g) if ar.rounding else g)
            gps.append(ar.rtz(gp))
        k = ar.mm(hs[-1], w[nh].t(), b[nh])
        fs, gq = f[s], gs[q]
        res["out"].index_add_(0, q, k * fs)
        # ---- backward -----------------------------------------------------------------------------------------------------------
        res["grad_f"].index_add_(0, s, gq * k)
        dk = ar.rb((gq if dk_scale is None else gq * dk_scale.to(dt)[q][:, None]) * fs)
        res[f"dW{nh}"] += ar.rows(dk, hs[-1])
        res[f"db{nh}"] += dk.sum(0)
        d = ar.mm(dk, w[nh]) * gps[nh - 1]
        for l in range(nh - 1, 0, -1):
            dzb = ar.rb(d)
            res[f"dW{l}"] += ar.rows(dzb, hs[l - 1])
            res[f"db{l}"] += dzb.sum(0)
            d = ar.mm(dzb, w[l]) * gps[l - 1]
        gc = ar.mm(d, w[0])
        res["grad_y"].index_add_(0, s, gc[:, :3])
        res["grad_x"].index_add_(0, q, gc[:, 3:])
        dzb = ar.rb(d)
        cb = ar.rb(cin)
        if swap_tile is not None:
            hit = (idx // 16) == swap_tile
            cb = torch.where(hit[:, None], torch.cat([cb[:, 3:], cb[:, :3]], dim=1), cb)
        res["dW0"] += ar.rows(dzb, cb)
        res["db0"] += dzb.sum(0)
    res["out"] = torch.where(deg[:, None] > 0, res["out"] / degf.clamp(min=1)[:, None], torch.zeros_like(res["out"]))
    return res


def mlp2(form: str, x: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor | None, dout: Tensor, seed: int = 0) -> dict:
    """the projection MLP out = W2 gelu(W1 x + b1) + b2 and its backward in one form -> {"out", "dx", "dW1", "db1", "dW2"};
    x [rows, 32], w1 [H, 32], w2 [OC, H], dout [rows, OC]"""
    ar = _Arith(form, seed)
    dt, dev = ar.dt, x.device
    n = x.shape[0]
    xb, w1b = ar.rb(x.detach().to(dt)), ar.rb(w1.detach().to(dt))
    b1, w2, dout = (t.detach().to(dt) for t in (b1, w2, dout))
    b2 = torch.zeros(w2.shape[0], dtype=dt, device=dev) if b2 is None else b2.detach().to(dt)
    res = {"out": torch.zeros(n, w2.shape[0], dtype=dt, device=dev), "dx": torch.zeros(n, x.shape[1], dtype=dt, device=dev),
           "dW1": torch.zeros_like(w1b), "db1": torch.zeros_like(b1), "dW2": torch.zeros_like(w2)}
    order = ar.order(n, dev)
    for lo in range(0, n, ar.BLOCK):
        idx = order[lo:lo + ar.BLOCK]
        xr, dor = xb[idx], dout[idx]
        g, gp = ar.act(ar.mm(xr, w1b.t(), b1))
        res["out"][idx] = ar.mm(g, w2.t(), b2)
        dz = ar.mm(dor, w2) * gp
        res["dW2"] += ar.rows(dor, g)
        res["db1"] += dz.sum(0)
        dzb = ar.rb(dz)
        res["dW1"] += ar.rows(dzb, xr)
        res["dx"][idx] = ar.mm(dzb, w1b)
    return res


# ---- the cases (shared by the CPU condition on the inputs, the floor table and the GPU test) ------------------------------------------
def rand_graph(n_src: int, n_dst: int, e: int, seed: int, heavy_dst: int, heavy_src: int) -> Tensor:
    """random edge list [2, e] with rows that are never hit, one query row (n_dst // 2) on the first ``heavy_dst`` edges and one
    source row (7) on the next ``heavy_src``"""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n_src, (e,), generator=g)
    dst = torch.randint(0, n_dst, (e,), generator=g)
    if e > 0:
        m = dst % 7 == 3
        dst[m] = (dst[m] + 1) % n_dst
        dst[:heavy_dst] = n_dst // 2
        src[heavy_dst:heavy_dst + heavy_src] = 7
    return torch.stack([src, dst]).to(torch.int32)


def _mlp_weights(layers, gen):
    ws, bs = [], []
    for i in range(len(layers) - 1):
        bound = 1.0 / layers[i] ** 0.5
        ws.append((torch.rand(layers[i + 1], layers[i], generator=gen) * 2 - 1) * bound)
        bs.append((torch.rand(layers[i + 1], generator=gen) * 2 - 1) * bound)
    return ws, bs


TAIL_E = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)      # around the 16 / 32 / 64 / 128-edge tiles of the two kernels
FWD_PASS_E = (767, 768, 769)                                           # 12 waves x 64 edges: one forward workgroup pass
NHS = (1, 2, 3, 4)


def gno_case(kind: str, e: int, nh: int) -> dict:
    """the inputs of one GNO case on the CPU (fp32): kind "tail" (n_src 40, n_dst 23, one long source row), "mid" (3000 / 700, empty
    rows and a > 32-edge row on each side: E = 20 011, 70 001, the forward-pass sizes) or "steady" (30 000 / 7000, a query row
    of 5000 edges and a source row of 3000)"""
    n_src, n_dst = {"tail": (40, 23), "mid": (3000, 700), "steady": (30000, 7000)}[kind]
    seed = 7919 * nh + e
    if kind == "tail":
        ei = rand_graph(n_src, n_dst, e, seed, heavy_dst=e // 10, heavy_src=0)
        ei[0, : max(1, (2 * e) // 3)] = 7
    elif kind == "mid":
        ei = rand_graph(n_src, n_dst, e, seed, heavy_dst=e // 10, heavy_src=max(e // 60, 40))
    else:
        ei = rand_graph(n_src, n_dst, e, seed, heavy_dst=5000, heavy_src=3000)
    gen = torch.Generator().manual_seed(seed + 1)
    ws, bs = _mlp_weights([6] + [64] * nh + [32], gen)
    return {"tag": f"{kind}_e{e}_nh{nh}", "ws": ws, "bs": bs, "ei": ei, "n_src": n_src, "n_dst": n_dst,
            "y": torch.rand(n_src, 3, generator=gen) * 2 - 1, "x": torch.rand(n_dst, 3, generator=gen) * 2 - 1,
            "f": torch.randn(n_src, 32, generator=gen), "gout": torch.randn(n_dst, 32, generator=gen)}


def gno_forms(case: dict, form: str, device="cpu", seed: int = 0, **kw) -> dict:
    c = case
    mv = lambda t: t.to(device)  # noqa: E731
    return gno(form, [mv(t) for t in c["ws"]], [mv(t) for t in c["bs"]], mv(c["y"]), mv(c["x"]), mv(c["f"]), mv(c["gout"]),
               mv(c["ei"][0]), mv(c["ei"][1]), seed=seed, **kw)


SMALL_GNO = [("tail", e, nh) for e in TAIL_E for nh in NHS] + [("mid", e, 3) for e in FWD_PASS_E] + [("mid", 20011, nh) for nh in NHS]
LARGE_GNO = [("steady", 400003, 3), ("steady", 400003, 4), ("mid", 70001, 2), ("mid", 70001, 4)]
GNO_TENSORS = ("out", "grad_f", "grad_y", "grad_x")

# the projection MLP: rows x (hidden, out).  MLP2_BWD_GRID / MLP2_FWD_GRID: the grid caps of mlp2.hip's launch code (MLP_BWD_GRID,
# fwd_oc) -- a workgroup takes a second 128-row tile from one row past 128 x the cap
MLP2_ROWS_PER_TILE, MLP2_BWD_GRID, MLP2_FWD_GRID = 128, 256, 2048
MLP_ROWS = (1, 127, 128, 129, 300, 4097)
MLP_SHAPES = ((64, 1), (128, 3), (256, 4))
SMALL_MLP = [(r, h, oc, True) for r in MLP_ROWS for (h, oc) in MLP_SHAPES] + [(300, 128, 3, False)]
LARGE_MLP = [(MLP2_ROWS_PER_TILE * MLP2_BWD_GRID + 1, 128, 3, True), (MLP2_ROWS_PER_TILE * MLP2_FWD_GRID + 1, 64, 1, True)]


def mlp_case(rows: int, hidden: int, oc: int, with_b2: bool) -> dict:
    gen = torch.Generator().manual_seed(31 * rows + hidden + oc)
    (w1, w2), (b1, b2) = _mlp_weights([32, hidden, oc], gen)
    return {"tag": f"mlp2_r{rows}_h{hidden}_o{oc}" + ("" if with_b2 else "_nob2"), "w1": w1, "b1": b1, "w2": w2,
            "b2": b2 if with_b2 else None, "x": torch.randn(rows, 32, generator=gen), "dout": torch.randn(rows, oc, generator=gen)}


def mlp_forms(case: dict, form: str, device="cpu", seed: int = 0) -> dict:
    c = case
    mv = lambda t: None if t is None else t.to(device)  # noqa: E731
    return mlp2(form, mv(c["x"]), mv(c["w1"]), mv(c["b1"]), mv(c["w2"]), mv(c["b2"]), mv(c["dout"]), seed=seed)


SEEDS = (0, 1, 2)
FLOOR_RMS, FLOOR_MAX = 1.0 / 12.0, 2.0 / 3.0       # the condition on the inputs: every F within these fractions of the yardsticks


def floors(tag: str, forms, case: dict, report=None):
    """the condition on the inputs of one case: every tensor of the three F realisations against (R, E) -> the Report"""
    import block_ref
    rep = report or block_ref.Report(tag)
    r, e = forms(case, "R"), forms(case, "E")
    for seed in SEEDS:
        got = forms(case, "F", seed=seed)
        for name in r:
            rep.model(f"{name}/F{seed}", got[name], r[name], e[name], rms_factor=FLOOR_RMS, max_factor=FLOOR_MAX)
    return rep


if __name__ == "__main__":
    # the floor table of profiles/gno_bf16_fp64_parity.txt: `python tests/gno_ref.py` = the large cases, `... all` = every case
    import os
    import sys
    import time
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    every = len(sys.argv) > 1 and sys.argv[1] == "all"
    missed = 0
    for kind, e_, nh_ in (SMALL_GNO if every else []) + LARGE_GNO:
        t0 = time.time()
        cs = gno_case(kind, e_, nh_)
        rp = floors(cs["tag"], gno_forms, cs)
        missed += len(rp.failures)
        print(f"# {cs['tag']}: {time.time() - t0:.1f} s", flush=True)
    for args in (SMALL_MLP if every else []) + LARGE_MLP:
        t0 = time.time()
        cs = mlp_case(*args)
        rp = floors(cs["tag"], mlp_forms, cs)
        missed += len(rp.failures)
        print(f"# {cs['tag']}: {time.time() - t0:.1f} s", flush=True)
    print(f"# {missed} tensor(s) missed the condition on the inputs")
    sys.exit(1 if missed else 0)
