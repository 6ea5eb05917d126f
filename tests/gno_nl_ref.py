"""Restatement of the fused GNO integral transform for transform_type 'nonlinear' / 'nonlinear_kernelonly' (the MODE_NONLINEAR /
MODE_KERNELONLY instantiations of csrc/gno_bf16.hip and csrc/gno_bwd3_bf16.hip plus the per-node products of
gaot_3d_amd/model/layers/integral_transform.py) in the three forms of tests/gno_ref.py, and the cases of
tests/test_gno_nonlinear_bf16_fp64_gpu.py (their teeth: tests/test_gno_nl_ref_cpu.py).

  E  the exact form: fp64, erf-GELU, nothing rounded (equal to oracle/gaot_oracle.py's integral_transform and its autograd).
  R  the rounding model: fp64 arithmetic, values rounded exactly where the kernels round them, the kernels' polynomial GELU.
  F  an fp32 realisation of R (shuffled edge order, 16-wide contraction chunks in a shuffled order; ``seed`` picks the shuffle).

The operator, with W_0 = [W_0c | W_0f] (coordinate columns, then feature columns) and the edges e = (s -> q):
    t[s] = W_0f f[s];  z_0[e] = W_0c [y_s, x_q] + b_0 + t[s];  k[e] = the rest of the kernel MLP
    out[q] = mean_e k[e] * f[s]  ('nonlinear', C_in == C_out)        out[q] = mean_e k[e]  ('nonlinear_kernelonly')
Output channels are taken in passes of 32 (integral_transform.py `_forward_fused`); every pass has its own dk and dz chain.

Rounding points -- everything gno_ref.py lists for the linear transform holds unchanged; what the two modes add or change:
  per-node products (integral_transform.py `_forward_fused`, GF.linear with precision=0: fp32, never rounded to bf16)
    t = f W_0f^T;  dW_0f = dt^T f;  grad_f += dt W_0f
  forward (gno_bf16.hip)
    the layer-0 accumulator starts from b_0 + t[s] in fp32 (:159-173), then W_0c [y_s, x_q] on the exact-fp32 MFMA (:174-179)
    'nonlinear_kernelonly': the staged value is k itself, no f gather (:241-242)
  backward (gno_bwd3_bf16.hip)
    layer 0 recomputed from b_0 + t[s] in fp32 (:364-366; t rows requested one tile ahead, :258-262)
    'nonlinear': grad_f[s] += gs k and dk = bf16(gs f[s]) as in the linear transform; 'nonlinear_kernelonly': dk = bf16(gs), no gs k
    term (:402, :449-452)
    dt[s] = sum over the edges of s of the fp32 dz_0, BEFORE its bf16 rounding, by a segmented scan along the edge lanes (:519-541, seg_scan_step :92-105); dW_0c / db_0 from bf16(dz_0) as before
    per-edge coordinate gradient W_0c^T dz_0 from the unrounded dz_0 and the fp32 W_0c, as before
Works on any device.  ``python tests/gno_nl_ref.py`` writes the floor table of profiles/gno_nl_bf16_fp64_parity.txt."""
from __future__ import annotations

import torch

import gno_ref as _G
from gno_ref import _Arith, _mlp_weights, gelu_erf, gelu_poly, rand_graph  # noqa: F401  (the GELU forms: re-exported for the tests)

Tensor = torch.Tensor
MODES = ("nonlinear", "nonlinear_kernelonly")


def gno_nl(form: str, mode: str, ws, bs, y: Tensor, x: Tensor, f: Tensor, gout: Tensor, src: Tensor, dst: Tensor, seed: int = 0,
           gelu: str | None = None, rounding: bool | None = None) -> dict:
    """the transform and its backward in one form -> {"out", "grad_f", "dt", "dW0c", "dW0f", "db0", "dW1".., "db1".., "grad_y",
    "grad_x"}.  ws / bs: the kernel MLP ([H0, 2 cd + C_in], [H1, H0], .., [C_out, H]); y [n_src, cd], x [n_dst, cd], f [n_src, C_in],
    gout [n_dst, C_out]; src / dst: the edge list.  ``dt`` has H0 columns."""
    assert mode in MODES, mode
    ar = _Arith(form, seed, gelu, rounding)
    dt_, dev = ar.dt, y.device
    nh, cd, cin, cout = len(ws) - 1, y.shape[1], f.shape[1], ws[-1].shape[0]
    assert ws[0].shape[1] == 2 * cd + cin and (mode == "nonlinear_kernelonly" or cin == cout)
    n_src, n_dst, ne = y.shape[0], x.shape[0], int(src.shape[0])
    src, dst = src.long().to(dev), dst.long().to(dev)
    w0 = ws[0].detach().to(dt_)
    w0c, w0f = w0[:, :2 * cd], w0[:, 2 * cd:]
    w = [w0c] + [ar.rb(wl.detach().to(dt_)) for wl in ws[1:]]
    b = [bl.detach().to(dt_) for bl in bs]
    y, x, f, gout = (t.detach().to(dt_) for t in (y, x, f, gout))
    deg = torch.bincount(dst, minlength=n_dst)
    degf = deg.to(dt_)
    inv = torch.where(deg > 0, 1.0 / degf.clamp(min=1), torch.zeros_like(degf))
    gs = gout * inv[:, None]
    kpad = (-cin) % 16                                                 # _Arith.mm cuts K into 16-wide chunks
    t = ar.mm(torch.nn.functional.pad(f, (0, kpad)), torch.nn.functional.pad(w0f, (0, kpad)).t())   # per-node product, never rounded

    res = {"out": torch.zeros(n_dst, cout, dtype=dt_, device=dev), "grad_f": torch.zeros(n_src, cin, dtype=dt_, device=dev),
           "dt": torch.zeros(n_src, w0.shape[0], dtype=dt_, device=dev),
           "grad_y": torch.zeros(n_src, cd, dtype=dt_, device=dev), "grad_x": torch.zeros(n_dst, cd, dtype=dt_, device=dev),
           "dW0c": torch.zeros_like(w0c), "db0": torch.zeros_like(b[0])}
    for l in range(1, nh + 1):
        res[f"dW{l}"] = torch.zeros_like(w[l])
        res[f"db{l}"] = torch.zeros_like(b[l])
    order = ar.order(ne, dev)
    for lo in range(0, ne, ar.BLOCK):
        idx = order[lo:lo + ar.BLOCK]
        s, q = src[idx], dst[idx]
        cin_e = torch.cat([y[s], x[q]], dim=1)
        hs, gps = [], []
        z = (b[0] + t[s]) + cin_e @ w[0].t()                           # the accumulator starts from b_0 + t[s]
        for l in range(nh):
            if l > 0:
                z = ar.mm(hs[-1], w[l].t(), b[l])
            g, gp = ar.act(z)
            hs.append(ar.rb(g))
            gps.append(ar.rtz(gp))
        k = ar.mm(hs[-1], w[nh].t(), b[nh])
        gq = gs[q]
        if mode == "nonlinear":
            fs = f[s]
            res["out"].index_add_(0, q, k * fs)
            res["grad_f"].index_add_(0, s, gq * k)
            dk_all = ar.rb(gq * fs)
        else:
            res["out"].index_add_(0, q, k)
            dk_all = ar.rb(gq)
        cb = ar.rb(cin_e)
        for c0 in range(0, cout, 32):                                  # one pass of the 32-channel kernels
            dk = dk_all[:, c0:c0 + 32]
            res[f"dW{nh}"][c0:c0 + 32] += ar.rows(dk, hs[-1])
            res[f"db{nh}"][c0:c0 + 32] += dk.sum(0)
            d = ar.mm(dk, w[nh][c0:c0 + 32]) * gps[nh - 1]
            for l in range(nh - 1, 0, -1):
                dzb = ar.rb(d)
                res[f"dW{l}"] += ar.rows(dzb, hs[l - 1])
                res[f"db{l}"] += dzb.sum(0)
                d = ar.mm(dzb, w[l]) * gps[l - 1]
            res["dt"].index_add_(0, s, d)                              # the unrounded dz_0
            gc = d @ w[0]
            res["grad_y"].index_add_(0, s, gc[:, :cd])
            res["grad_x"].index_add_(0, q, gc[:, cd:])
            dzb = ar.rb(d)
            res["dW0c"] += ar.rows(dzb, cb)
            res["db0"] += dzb.sum(0)
    res["out"] = torch.where(deg[:, None] > 0, res["out"] / degf.clamp(min=1)[:, None], torch.zeros_like(res["out"]))
    res["dW0f"] = ar.rows(res["dt"], f)                                # per-node products of the caller
    res["grad_f"] = res["grad_f"] + ar.mm(res["dt"], w0f)
    return res


# The condition on the inputs (test_gno_nl_ref_cpu.py): on every case the fp32 realisations F sit within 1/12 (rms) and 2/3 (max) of the
# yardstick.  On a graph of a few dozen edges one bf16 flip of an activation that the fp32 and fp64 evaluations round differently is a
# visible fraction of every sum; the cases below drew such inputs and take the next draw that meets the condition (a property of the
# inputs and the model alone: no kernel result enters).
SALT = {("tail", "nonlinear", 32, 3, 32, 32, 64, 3): 1, ("tail", "nonlinear", 128, 4, 32, 32, 64, 3): 1,
        ("tail", "nonlinear", 257, 4, 32, 32, 64, 3): 1, ("tail", "nonlinear_kernelonly", 32, 3, 32, 32, 64, 3): 1}


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def nl_case(kind: str, mode: str, e: int, nh: int, cin: int = 32, cout: int = 32, hidden: int = 64, cd: int = 3) -> dict:
    """the inputs of one case on the CPU (fp32).  kind "tail" (n_src 40, n_dst 23: source 7 carries two thirds of the edges, so from
    E = 49 its row spans more than two 16-edge tiles and from E = 193 crosses the backward's 128-edge pass; sources without an edge),
    "mid" (3000 / 700: empty rows, a source row of max(E / 60, 40) >= 200 edges across tiles and workgroup passes) or "steady"
    (20 000 / 7000, a query row of 5000 edges and a source row of 3000)"""
    n_src, n_dst = {"tail": (40, 23), "mid": (3000, 700), "steady": (20000, 7000)}[kind]
    seed = 7919 * nh + e + 13 * cin + 17 * cout + hidden + cd + (1 if mode == "nonlinear" else 2)
    seed += 1000003 * SALT.get((kind, mode, e, nh, cin, cout, hidden, cd), 0)
    if kind == "tail":
        ei = rand_graph(n_src, n_dst, e, seed, heavy_dst=e // 10, heavy_src=0)
        ei[0, : max(1, (2 * e) // 3)] = 7
    elif kind == "mid":
        ei = rand_graph(n_src, n_dst, e, seed, heavy_dst=e // 10, heavy_src=max(e // 60, 200))
    else:
        ei = rand_graph(n_src, n_dst, e, seed, heavy_dst=5000, heavy_src=3000)
    gen = torch.Generator().manual_seed(seed + 1)
    ws, bs = _mlp_weights([2 * cd + cin] + [hidden] * nh + [cout], gen)
    tag = f"{mode}_{kind}_e{e}_nh{nh}" + ("" if (cin, cout, hidden, cd) == (32, 32, 64, 3) else f"_c{cin}-{cout}_h{hidden}_d{cd}")
    return {"tag": tag, "mode": mode, "ws": ws, "bs": bs, "ei": ei, "n_src": n_src, "n_dst": n_dst,
            "y": torch.rand(n_src, cd, generator=gen) * 2 - 1, "x": torch.rand(n_dst, cd, generator=gen) * 2 - 1,
            "f": torch.randn(n_src, cin, generator=gen), "gout": torch.randn(n_dst, cout, generator=gen)}


def nl_forms(case: dict, form: str, device="cpu", seed: int = 0, **kw) -> dict:
    c = case
    mv = lambda t: t.to(device)  # noqa: E731
    return gno_nl(form, c["mode"], [mv(t) for t in c["ws"]], [mv(t) for t in c["bs"]], mv(c["y"]), mv(c["x"]), mv(c["f"]),
                  mv(c["gout"]), mv(c["ei"][0]), mv(c["ei"][1]), seed=seed, **kw)


# edge counts of gno_ref.py (around the backward's 16-edge tile and 128-edge pass, the forward's 32-edge tile and 64-edge macro
# tile); 193 and 257 added: the heavy source row of the "tail" graph (2 E / 3 edges) then crosses the 128-edge workgroup pass
TAIL_E = _G.TAIL_E + (193, 257)
NHS_BF16, NHS_FP32 = _G.NHS, (1, 2, 3)
# (kind, e, nh, cin, cout, hidden, cd) per mode
SHAPES = {"nonlinear": [("mid", 2003, 2, 16, 16, 64, 3), ("mid", 2003, 2, 64, 64, 64, 3), ("mid", 2003, 2, 32, 32, 48, 3),
                        ("mid", 2003, 2, 32, 32, 64, 2)],
          "nonlinear_kernelonly": [("mid", 2003, 2, 40, 32, 64, 3), ("mid", 2003, 2, 16, 16, 64, 3), ("mid", 2003, 2, 32, 32, 48, 3),
                                   ("mid", 2003, 2, 32, 32, 64, 2)]}


def small_cases(nhs=NHS_BF16):
    """every case but the steady-state one, both modes: (kind, mode, e, nh, cin, cout, hidden, cd)"""
    out = []
    for mode in MODES:
        out += [("tail", mode, e, nh, 32, 32, 64, 3) for e in TAIL_E for nh in nhs]
        out += [("mid", mode, e, 3, 32, 32, 64, 3) for e in _G.FWD_PASS_E]
        out += [("mid", mode, 20011, nh, 32, 32, 64, 3) for nh in nhs]
        out += [(k, mode, e, nh, ci, co, h, cd) for (k, e, nh, ci, co, h, cd) in SHAPES[mode]]
    return out


LARGE = [("steady", mode, 400003, 3, 32, 32, 64, 3) for mode in MODES]
SEEDS = _G.SEEDS
FLOOR_RMS, FLOOR_MAX = _G.FLOOR_RMS, _G.FLOOR_MAX
# (dW_0f = dt^T f and dt are fp32 products / sums of the unrounded dz_0, yet their yardstick R - E -- the bf16 error of the layers above
# -- is wide enough: F reaches the floor fractions for them on every case, so the one rule holds for every tensor)


def floors(case: dict, report=None):
    """the condition on the inputs of one case: every tensor of the three F realisations against (R, E) -> (Report, {tensor: worst
    (rms ratio, max ratio) of F over the seeds})"""
    import block_ref
    rep = report or block_ref.Report(case["tag"])
    r, e = nl_forms(case, "R"), nl_forms(case, "E")
    worst = {}
    for seed in SEEDS:
        got = nl_forms(case, "F", seed=seed)
        for name in r:
            rep.model(f"{name}/F{seed}", got[name], r[name], e[name], rms_factor=FLOOR_RMS, max_factor=FLOOR_MAX)
            a = rep.achieved[f"{name}/F{seed}"]
            w = worst.get(name, (0.0, 0.0))
            worst[name] = (max(w[0], a[0]), max(w[1], a[1]))
    return rep, worst


if __name__ == "__main__":
    # the floor table of profiles/gno_nl_bf16_fp64_parity.txt: `python tests/gno_nl_ref.py` = the shape cases, mid size and the steady
    # state; `... all` = every case
    import os
    import sys
    import time
    every = len(sys.argv) > 1 and sys.argv[1] == "all"
    cases = small_cases() if every else [c for c in small_cases() if c[0] == "mid" and c[2] in (2003, 20011) and c[3] in (2, 3)]
    missed = 0
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "profiles", "gno_nl_bf16_fp64_parity.txt"), "w") as fh:
        fh.write("# floor table: worst distance of the fp32 realisations F (three shuffle seeds) to the rounding model R, relative to the\n"
                 "# yardstick R - E: rms(F - R) / rms(R - E), max|F - R| / max|R - E| per tensor (condition on the inputs: 1/12 and 2/3;\n"
                 "# the kernels' rule: 1/4 and 2)\n")
        for args in cases + LARGE:
            t0 = time.time()
            cs = nl_case(args[0], args[1], *args[2:])
            rp, worst = floors(cs)
            missed += len(rp.failures)
            fh.write(f"{cs['tag']}: " + "  ".join(f"{n} {a:.3f}/{b:.3f}" for n, (a, b) in worst.items()) + "\n")
            fh.flush()
            print(f"# {cs['tag']}: {time.time() - t0:.1f} s", flush=True)
        fh.write(f"# {missed} tensor realisation(s) missed the condition on the inputs\n")
    print(f"# {missed} tensor realisation(s) missed the condition on the inputs")
    sys.exit(0)
