"""fp64 restatement of one bf16 Transformer block (reference attn.py:104-127, 146-157, 205-230), stage by stage, and the comparison
helpers of tests/test_block_bf16_fp64_gpu.py (their teeth: tests/test_block_ref_cpu.py).

Each stage takes the tensors its kernel reads and, where an upstream kernel hands a bf16 tensor on (yb, dag, u, dyb) or the row
constants 1/rms, that kernel's own output -- so a fault shows up in the launch that made it.  The arithmetic is fp64; values are
rounded to bf16 exactly where the kernels of csrc/ffn_fused.hip round them:
  * bf16(norm x)                  the A operand of q|k|v and of w1|w3 (k_norm_qkv, k_ffn_fwd<NORM>: written out as yb)
  * the inputs of a row-block product (o, dh, dqkv, the skip projection's xa / xb, the dx rows of k_qkv_bwd_norm<CATB>)
  * a | g and u = silu(a) g       (k_ffn_fwd, recomputed by k_ffn_bwd_dx: the SwiGLU runs on the ROUNDED a, g)
  * du = dy W2 and bf16(dy)       (k_ffn_bwd_dx: the derivative runs on the rounded du; dag is written as bf16)
  * every weight                  (the packed fragment images are bf16)
  * the attention image           (RoPE from the fp32 (cos, sin) table of ops.rope_table, q times ops._qscale(scale), then bf16)
Works on any device (the GPU test computes on the GPU, the CPU test on the CPU)."""
from __future__ import annotations

import torch

Tensor = torch.Tensor
D = 256


def rb(t: Tensor) -> Tensor:
    """round to bf16 (nearest even), back to fp64"""
    return t.to(torch.bfloat16).double()


def _d(t: Tensor) -> Tensor:
    return t.detach().double()


# ---- stages -----------------------------------------------------------------------------------------------------------------------
def norm(x: Tensor, w: Tensor, eps: float):
    """RMSNorm (attn.py:167-178): -> (n, 1/rms)"""
    x = _d(x)
    r = torch.rsqrt(x.square().mean(-1) + eps)
    return x * r[:, None] * _d(w), r


def rope_image(proj: Tensor, table: Tensor | None, s: int, nq: int, nk: int, qscale: float) -> Tensor:
    """the attention kernels' image before its bf16 rounding: q | k | v row-major, RoPE on the q and k heads from the fp32 [S][16][2]
    (cos, sin) table at position row % S (pairs of adjacent columns), q times qscale"""
    out = proj.clone()
    rows = proj.shape[0]
    if table is not None:
        t = _d(table)[torch.arange(rows, device=proj.device) % s]             # [rows, 16, 2]
        c, sn = t[:, None, :, 0], t[:, None, :, 1]
        qk = out[:, :(nq + nk) * 32].view(rows, nq + nk, 16, 2)
        v0, v1 = qk[..., 0].clone(), qk[..., 1].clone()
        qk[..., 0] = v0 * c - v1 * sn
        qk[..., 1] = v1 * c + v0 * sn
    out[:, :nq * 32] *= qscale
    return out


def head(x: Tensor, nw: Tensor, eps: float, wqkv: Tensor, yb: Tensor, table: Tensor | None, s: int, nq: int, nk: int, qscale: float):
    """gaot_norm_qkv_image: x fp32 [rows, 256] -> yb, rstd, image (fp64, unrounded); ``yb`` = the kernel's bf16 rows (the product's input)"""
    n, r = norm(x, nw, eps)
    img = rope_image(_d(yb) @ rb(wqkv).t(), table, s, nq, nk, qscale)
    return {"yb": n, "rstd": r, "image": img}


def skip_proj(xa: Tensor, xb: Tensor, wskip: Tensor, bskip: Tensor | None) -> Tensor:
    """the decoder block's x = skip_proj(cat([x, skip])) (attn.py:222-225) on bf16 inputs and weight, fp32 bias"""
    w = rb(wskip)
    out = rb(xa) @ w[:, :D].t() + rb(xb) @ w[:, D:].t()
    return out + _d(bskip) if bskip is not None else out


def cat_head(xa, xb, wskip, bskip, nw, eps, wqkv, yb, table, s, nq, nk, qscale):
    """gaot_cat_norm_qkv_image -> xo (fp32 output) and head()'s tensors of the projected rows"""
    xo = skip_proj(xa, xb, wskip, bskip)
    out = head(xo, nw, eps, wqkv, yb, table, s, nq, nk, qscale)
    out["xo"] = xo
    return out


def swiglu(yb: Tensor, w13: Tensor, f: int):
    """a | g = bf16(yb W13^T), u = bf16(silu(a) g) -> (a, g, u)"""
    ag = rb(_d(yb) @ rb(w13).t())
    a, g = ag[:, :f], ag[:, f:]
    return a, g, rb(torch.nn.functional.silu(a) * g)


def tail(o: Tensor, x: Tensor, wo: Tensor, nw: Tensor, eps: float, w2: Tensor, u: Tensor):
    """gaot_block_tail_fwd: h = x + o Wo^T, n = RMSNorm(h), y = n + u W2^T -> h, yb = n (rounded by the check), rstd, y.
    ``u``: bf16(silu(a) g) of the kernel's own yb as a kernel hands it on (gaot_ffn_bwd_norm recomputes it from the same rows) --
    the forward keeps it on chip; its own check is in ffn_bwd_norm()"""
    h = _d(x) + rb(o) @ rb(wo).t()
    n, r = norm(h, nw, eps)
    return {"h": h, "yb": n, "rstd": r, "y": n + _d(u) @ rb(w2).t()}


def norm_bwd(dn: Tensor, x: Tensor, nw: Tensor, rstd: Tensor, dres: Tensor | None = None, dtap: Tensor | None = None):
    """RMSNorm backward from d(norm x) (norm_bwd_epilogue): dx = r w dn - x r^3 mean(x w dn) (+ dres) (+ dtap);
    the weight gradient's per-element terms dn x r (its column sums and their mass)"""
    x, w, r = _d(x), _d(nw), _d(rstd)[:, None]
    c = (x * w * dn).sum(-1, keepdim=True) * r ** 3 / x.shape[1]
    dx = r * w * dn - x * c
    if dres is not None:
        dx = dx + _d(dres)
    if dtap is not None:
        dx = dx + _d(dtap)
    terms = dn * x * r
    return dx, terms.sum(0), terms.abs().sum(0)


def ffn_bwd_norm(yb, dy, w13, w2, f, h, nw, rstd, dag):
    """gaot_ffn_bwd_norm: dyb, u, dag (fp64, unrounded: the kernel re-rounds the a | g it recomputes), dh, the ffn_norm weight gradient.
    ``dag``: the kernel's bf16 output, the operand of dn = dag W13 + dy"""
    dy = _d(dy)
    dyb = rb(dy)
    a, g, _u = swiglu(yb, w13, f)
    du = rb(dyb @ rb(w2))
    sg = torch.sigmoid(a)
    dag_ref = torch.cat([du * g * sg * (1.0 + a * (1.0 - sg)), du * a * sg], dim=1)
    dn = _d(dag) @ rb(w13) + dy
    dh, dnw, mass = norm_bwd(dn, h, nw, rstd)
    return {"dyb": dy, "u": torch.nn.functional.silu(a) * g, "dag": dag_ref, "dh": dh, "dnw": dnw, "dnw_mass": mass}


def oproj_bwd(dh: Tensor, o: Tensor, wo: Tensor, b: int, s: int, nh: int):
    """gaot_oproj_bwd_image: d_o = bf16(dh) Wo (the bf16 dO image before its rounding) and delta[b, head, s] = sum over the head's 32
    columns of d_o * o"""
    do = rb(dh) @ rb(wo)
    delta = (do * _d(o)).view(b, s, nh, 32).sum(-1).permute(0, 2, 1).contiguous()
    return {"do": do, "delta": delta}


def qkv_bwd_norm(dqkv, wqkv, x, nw, rstd, dres=None, dtap=None):
    """gaot_qkv_bwd_norm: dx and the attn_norm weight gradient from d(norm x) = bf16(dqkv) Wqkv"""
    dx, dnw, mass = norm_bwd(rb(dqkv) @ rb(wqkv), x, nw, rstd, dres, dtap)
    return {"dx": dx, "dnw": dnw, "dnw_mass": mass}


def skip_bwd(dx: Tensor, wskip: Tensor, same: bool):
    """k_qkv_bwd_norm<CATB>'s second product: dxa = bf16(dx) Ws[:, :256], dxb = bf16(dx) Ws[:, 256:] (their sum when ``same``);
    ``dx`` = the kernel's fp32 dx rows (the bf16 tile is formed from them)"""
    w = rb(wskip)
    dxb16 = rb(dx)
    dxa, dxb = dxb16 @ w[:, :D], dxb16 @ w[:, D:]
    return {"dxa": dxa + dxb} if same else {"dxa": dxa, "dxb": dxb}


def dw(a: Tensor, b: Tensor):
    """a weight-gradient product a^T b over the rows on the bf16-rounded operands -> (fp64 value, mass sum_rows |a_ri b_rj|)"""
    a, b = rb(a), rb(b)
    return a.t() @ b, a.abs().t() @ b.abs()


# ---- comparisons ------------------------------------------------------------------------------------------------------------------
def ulp_distance(got: Tensor, ref: Tensor) -> Tensor:
    """|steps between two bf16 values| on the bf16 number line (sign-magnitude -> ordered integers; +0 and -0 are one value)"""
    def key(t):
        bits = t.to(torch.bfloat16).contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
        mag = bits & 0x7FFF
        return torch.where(bits >= 0x8000, -mag, mag)
    return (key(got) - key(ref)).abs()


class Report:
    """collects the checks of one case: every check prints one ``[parity]`` line with its achieved value and its bound, and done()
    fails with the list of every check that missed -- which tensor of which stage, by how much"""

    def __init__(self, tag: str):
        self.tag, self.failures, self.achieved = tag, [], {}

    def _out(self, name, ok, text):
        line = f"[parity] {self.tag}/{name}: {text}"
        print(line)
        if not ok:
            self.failures.append(line)
        return ok

    def fp32(self, name, got, ref, bound=1e-5):
        """max |got - ref| <= bound x max |ref|"""
        got, ref = _d(got), _d(ref)
        if got.shape != ref.shape:
            return self._out(name, False, f"shape {tuple(got.shape)} != {tuple(ref.shape)}")
        finite = bool(torch.isfinite(got).all())
        peak = ref.abs().max().item() if ref.numel() else 0.0
        err = (got - ref).abs().max().item() if (ref.numel() and finite) else (0.0 if finite else float("inf"))
        rel = err / max(peak, 1e-300)
        self.achieved[name] = rel
        return self._out(name, finite and rel <= bound, f"max|err|/peak={rel:.3e} (bound {bound:.1e}) peak={peak:.3e}")

    def bf16(self, name, got, ref, flips=1e-3, beyond=0.0, abs_tol=1e-5):
        """bf16 output against bf16(ref): an element is equal, one ulp off (a rounding-boundary flip: at most a fraction ``flips``), or
        more than one ulp off (at most a fraction ``beyond``).  An element within ``abs_tol`` x max|ref| of the fp64 value counts as equal:
        a result that cancels to near zero (|v| ~ 1e-5 of its terms) carries the fp32 accumulation's error in its leading bits"""
        if got.shape != ref.shape:
            return self._out(name, False, f"shape {tuple(got.shape)} != {tuple(ref.shape)}")
        refd = _d(ref)
        gotd = _d(got)
        finite = bool(torch.isfinite(gotd).all())
        peak = refd.abs().max().item() if refd.numel() else 0.0
        dist = ulp_distance(got, refd)
        tiny = (gotd - refd).abs() <= abs_tol * peak
        n = max(dist.numel(), 1)
        n1 = int(((dist == 1) & ~tiny).sum())
        nb = int(((dist > 1) & ~tiny).sum())
        worst = int(dist[~tiny].max()) if bool((~tiny).any()) else 0
        f1, fb = n1 / n, nb / n
        self.achieved[name] = (f1, fb)
        ok = finite and f1 <= flips and fb <= beyond
        return self._out(name, ok, f"one-ulp flips {n1}/{n} = {f1:.2e} (bound {flips:.1e}), beyond one ulp {nb} = {fb:.2e} "
                                   f"(bound {beyond:.1e}), worst {worst} ulp above the absolute floor")

    def exact(self, name, got, ref):
        """bit equality (two paths that must do the same arithmetic)"""
        same = bool(torch.equal(got, ref))
        self.achieved[name] = same
        return self._out(name, same, "bit-identical" if same else
                         f"DIFFER: max|diff|={(_d(got) - _d(ref)).abs().max().item():.3e}")

    def colsum(self, name, got, ref, mass, bound=1e-5):
        """a sum over the rows (a weight gradient): |got_j - ref_j| <= bound x sum_rows |term_ij| for every element j"""
        got, ref, mass = _d(got), _d(ref), _d(mass)
        if got.shape != ref.shape:
            return self._out(name, False, f"shape {tuple(got.shape)} != {tuple(ref.shape)}")
        finite = bool(torch.isfinite(got).all())
        rel = ((got - ref).abs() / mass.clamp_min(1e-300)).max().item() if finite else float("inf")
        self.achieved[name] = rel
        return self._out(name, finite and rel <= bound, f"max |err_j| / sum|term_ij| = {rel:.3e} (bound {bound:.1e})")

    def model(self, name, got, r, e, rms_factor=0.25, max_factor=2.0):
        """a result against a rounding model R and the exact form E (tests/gno_ref.py): rms(got - R) <= rms_factor x rms(R - E) and
        max|got - R| <= max_factor x max|R - E| -- the yardstick R - E is the model's own bf16 error, nothing of it comes from ``got`` --
        and exactly 0 wherever R = E = 0 (no edges, rows without edges)"""
        got, r, e = _d(got), _d(r), _d(e)
        if got.shape != r.shape:
            return self._out(name, False, f"shape {tuple(got.shape)} != {tuple(r.shape)}")
        if not bool(torch.isfinite(got).all()):
            self.achieved[name] = (float("inf"), float("inf"))
            return self._out(name, False, "not finite")
        n = max(r.numel(), 1)
        yard, err = r - e, got - r
        yrms, ymax = (yard.square().sum().item() / n) ** 0.5, yard.abs().max().item() if r.numel() else 0.0
        erms, emax = (err.square().sum().item() / n) ** 0.5, err.abs().max().item() if r.numel() else 0.0
        rr = 0.0 if erms == 0.0 else (erms / yrms if yrms > 0.0 else float("inf"))
        rm = 0.0 if emax == 0.0 else (emax / ymax if ymax > 0.0 else float("inf"))
        zero = (r == 0) & (e == 0)
        nz = int((got[zero] != 0).sum())
        self.achieved[name] = (rr, rm)
        ok = rr <= rms_factor and rm <= max_factor and nz == 0
        return self._out(name, ok, f"rms(got-R)/rms(R-E)={rr:.3e} (bound {rms_factor:.3g}) max|got-R|/max|R-E|={rm:.3e} (bound {max_factor:.3g}) "
                                   f"rms(R-E)={yrms:.3e} max|R-E|={ymax:.3e}" + (f" NONZERO where R = E = 0: {nz}" if nz else ""))

    def done(self):
        assert not self.failures, f"{len(self.failures)} check(s) missed:\n" + "\n".join(self.failures)
