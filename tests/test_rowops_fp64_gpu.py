"""The row / element kernels of csrc/rowops.hip and the activation table of csrc/common.h against the fp64 restatements of
tests/rowops_ref.py, at the shapes where each kernel takes another path: widths on both sides of the d = 256 RMSNorm kernel, row counts
around the 32-row block, the float4 and the scalar column sums with ld > N, more partials than one reduction stride, the grid-stride
loop of the MSE, every activation id at its kinks and thresholds.  Every comparison prints one ``[parity]`` line with the achieved
error; the bars are fp32 arithmetic's own (stated where they are used)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowops_ref as R  # noqa: E402
from parity import close  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-6
U = 2.0 ** -24          # fp32 unit roundoff


def gen(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def within(name, got, ref, bar):
    """|got - ref| <= bar element by element, got finite; prints the achieved error and the worst err / bar"""
    got = got.detach().double().cpu()
    ref, bar = ref.double(), bar.double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs()
    ratio = torch.where(err > 0, err / bar.clamp_min(1e-300), torch.zeros_like(err))
    worst = ratio.max().item() if ratio.numel() else 0.0
    print(f"[parity] {name}: max_abs={err.max().item() if err.numel() else 0.0:.3e} ref_peak={ref.abs().max().item() if ref.numel() else 0.0:.3e} "
          f"worst err/bar={worst:.3f}")
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    assert worst <= 1.0, f"{name}: error {worst:.3f} x its bar at element {int(ratio.flatten().argmax())}"


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---- activations -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _act_ref(name):
    v = R.act_grid()
    return R.act(name, v), R.act_grad(name, v)


@pytest.mark.parametrize("name", R.ACT_NAMES[1:])
def test_activation_kernels(name):
    """gaot_act_fwd / gaot_act_grad through ops.act_fwd / ops.act_bwd at the bar of rowops_ref.act_bar: 4e-6 |ref| + 4e-7 max(1, |v|)"""
    from gaot_3d_amd import ops
    code = ops.ACT[name]
    v = R.act_grid()
    ref, dref = _act_ref(name)
    vd = v.to(DEV)
    within(f"act/{name}/fwd", ops.act_fwd(vd, code), ref, R.act_bar(ref, v))
    dz1 = ops.act_bwd(vd, torch.ones_like(vd), code)
    within(f"act/{name}/grad", dz1, dref, R.act_bar(dref, v))
    # dz = dh * act'(z): one more product, one more rounding
    dh = gen(v.numel(), seed=3)
    want = dh.double() * dz1.double().cpu()
    # (a derivative below the smallest normal number, 2^-126, may be flushed, or keeps fewer bits: exp(-88), gelu' at -13)
    within(f"act/{name}/dz", ops.act_bwd(vd, dh.to(DEV), code), want, 2 * U * want.abs() + 2.0 ** -126 * (1.0 + dh.double().abs()))
    if name == "hardswish":     # AT the kinks: 0 and 1, the outer one-sided values, as torch's kernels give on this device too
        k = ops.act_bwd(torch.tensor([-3.0, 3.0], device=DEV), torch.ones(2, device=DEV), code)
        leaf = torch.tensor([-3.0, 3.0], device=DEV, requires_grad=True)
        torch.nn.functional.hardswish(leaf).sum().backward()
        assert k.tolist() == [0.0, 1.0] and leaf.grad.tolist() == [0.0, 1.0], (k, leaf.grad)


@pytest.mark.parametrize("name", R.ACT_NAMES)
def test_linear_with_every_activation(name, monkeypatch):
    """GF.linear(act=name): ids 1-3 run in the GEMM's epilogue and keep the pre-activation, 4+ as a pass of their own.  Column 0 of the
    pre-activation IS the activation grid (weight row (1, 0, 0), no bias there: exact in fp32), the others are unit-scale mixes.
    fp64 reference of the whole linear; bars of test_linear_family_autograd (gradients 1e-3 / 1e-4; the output at the suite's fp32
    output bar 1e-4 / 1e-5)"""
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd import ops
    monkeypatch.setitem(ops.ROWLIN, "enabled", False)      # none / relu at this shape would take the single-pass kernels (own tests)
    v = R.act_grid()
    m = v.numel()
    x = torch.stack([v, gen(m, seed=1), gen(m, seed=2)], dim=1)
    w, b, g = gen(5, 3, seed=3), gen(5, seed=4), gen(m, 5, seed=5)
    w[0] = torch.tensor([1.0, 0.0, 0.0])
    b[0] = 0.0
    y_ref, z = R.linear_fwd(x, w, b, name)
    assert torch.equal(z[:, 0], v.double())
    dx_ref, dw_ref, db_ref = R.linear_bwd(x, w, z, g, name)
    xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    before = ops.ROWLIN["fwd"]
    y = GF.linear(xd, wd, bd, act=name, precision=0)
    assert ops.ROWLIN["fwd"] == before
    (y * g.to(DEV)).sum().backward()
    close(f"linear/{name}/y", y, y_ref, 1e-4, 1e-5)
    close(f"linear/{name}/dx", xd.grad, dx_ref, 1e-3, 1e-4)
    close(f"linear/{name}/dw", wd.grad, dw_ref, 1e-3, 1e-4)
    close(f"linear/{name}/db", bd.grad, db_ref, 1e-3, 1e-4)


# ---- RMSNorm -----------------------------------------------------------------------------------------------------------------------
RN_ROWS = (1, 8, 31, 32, 33, 300)


def _rmsnorm_case(tag, x, w, g, form, bf16=False):
    """one forward + backward through RMSNormFn (form "plain") or RMSNormResFn ("res0": the residual unused, "res": with the residual's
    gradient, "tap": residual and tap gradients, "taponly": the tap's alone) against the fp64 formulas.  -> (y, image, dx, dw)"""
    import gaot_3d_amd
    from gaot_3d_amd import functional as GF
    rows, d = x.shape
    gres = gen(rows, d, seed=11) if form in ("res", "tap") else None
    gtap = gen(rows, d, seed=12) if form in ("tap", "taponly") else None
    xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    gaot_3d_amd.set_precision("bf16" if bf16 else "fp32")
    try:
        if form == "plain":
            y, yb = GF.RMSNormFn.apply(xd, wd, EPS)
            loss = (y * g.to(DEV)).sum()
        else:
            outs = GF.RMSNormResFn.apply(xd, wd, EPS, form in ("tap", "taponly"))
            y, xres, yb = outs[:3]
            assert torch.equal(xres, xd.detach())
            loss = (y * g.to(DEV)).sum()
            if gres is not None:
                loss = loss + (xres * gres.to(DEV)).sum()
            if gtap is not None:
                assert torch.equal(outs[3], xd.detach())
                loss = loss + (outs[3] * gtap.to(DEV)).sum()
        loss.backward()
    finally:
        gaot_3d_amd.set_precision("fp32")
    y_ref, _ = R.rmsnorm_fwd(x, w, EPS)
    dx_ref, dw_ref = R.rmsnorm_bwd(x, w, EPS, g, gres, gtap)
    close(f"rmsnorm/{tag}/y", y, y_ref, 1e-5, 1e-6)
    close(f"rmsnorm/{tag}/dx", xd.grad, dx_ref, 1e-4, 1e-5)
    close(f"rmsnorm/{tag}/dw", wd.grad, dw_ref, 1e-4, 1e-4)
    if bf16 and d % 8 == 0:
        assert yb.shape == y.shape and torch.equal(yb, y.detach().bfloat16()), tag
    else:
        assert yb.numel() == 0, tag
    return y.detach(), yb, xd.grad, wd.grad


@pytest.mark.parametrize("d", [4, 8, 252, 256, 260, 512, 1024])
def test_rmsnorm_widths_and_rows(d):
    """d = 256 takes k_rmsnorm_bwd_d256 (tail rows clamped, not stored), every other width the generic kernel (1, 2, 4 float4 per lane;
    252 and 260: a last float4 stride that is not full).  rows around the 32-row block.  Bars: the existing test's"""
    w = gen(d, seed=2) * 0.1 + 1
    for rows in RN_ROWS:
        x, g = gen(rows, d, seed=rows), gen(rows, d, seed=100 + rows)
        _rmsnorm_case(f"d{d}/r{rows}/plain", x, w, g, "plain")
        _rmsnorm_case(f"d{d}/r{rows}/plain/bf16", x, w, g, "plain", bf16=True)
        if d in (256, 512):
            for form in ("res0", "res", "tap", "taponly"):
                _rmsnorm_case(f"d{d}/r{rows}/{form}", x, w, g, form)
            _rmsnorm_case(f"d{d}/r{rows}/tap/bf16", x, w, g, "tap", bf16=True)


@pytest.mark.parametrize("d", [256, 260])
def test_rmsnorm_row_scales_and_a_zero_row(d):
    """rows scaled from 1e-3 to 1e3 and one all-zero row (1/rms = 1/sqrt(eps) there).  dx of a row scales with 1/rms and dw's terms with
    the upstream gradient, so the upstream gradient of a row carries the row's scale (dx is then unit-scale in every row, where the
    element-wise bar 1e-4 |ref| + 1e-5 is a statement about fp32), and its signs are sign(x): dw = sum over the rows of dy x r is then
    a sum of same-signed terms dominated by the large rows, which the relative part of its bar measures -- with free signs a column of
    dw is a cancelling sum of terms ~1e3 that no fp32 summation holds to 1e-4 of its own value"""
    rows = 33
    scale = 10.0 ** torch.linspace(-3, 3, rows)
    x = gen(rows, d, seed=1) * scale[:, None]
    x[7] = 0.0
    w = gen(d, seed=2) * 0.1 + 1
    sign = torch.where(x < 0, -torch.ones_like(x), torch.ones_like(x))
    g = gen(rows, d, seed=3).abs() * sign * scale[:, None]
    for form in ("plain", "tap"):
        _rmsnorm_case(f"scaled/d{d}/{form}", x, w, g, form)


@pytest.mark.parametrize("rows,d", [(300, 256), (33, 512)])
def test_rmsnorm_expanded_upstream_gradient_and_reproducibility(rows, d):
    from gaot_3d_amd import functional as GF
    x, w = gen(rows, d, seed=1), gen(d, seed=2) * 0.1 + 1
    grads = []
    for _ in range(2):
        xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
        y, _yb = GF.RMSNormFn.apply(xd, wd, EPS)
        y.sum().backward()                          # the upstream gradient arrives as a stride-0 expanded tensor
        grads.append((xd.grad, wd.grad))
    dx_ref, dw_ref = R.rmsnorm_bwd(x, w, EPS, torch.ones(rows, d))
    close(f"rmsnorm/expanded/d{d}/dx", grads[0][0], dx_ref, 1e-4, 1e-5)
    close(f"rmsnorm/expanded/d{d}/dw", grads[0][1], dw_ref, 1e-4, 1e-4)
    assert torch.equal(grads[0][1], grads[1][1]) and torch.equal(grads[0][0], grads[1][0])


def test_rmsnorm_edges():
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd._lib import GaotError
    for d in (256, 260):        # no rows: an empty y and a ZERO weight gradient
        xd, wd = torch.empty(0, d, device=DEV, requires_grad=True), (gen(d, seed=2) + 1).to(DEV).requires_grad_(True)
        y, _yb = GF.RMSNormFn.apply(xd, wd, EPS)
        assert y.shape == (0, d)
        y.sum().backward()
        assert wd.grad.shape == (d,) and torch.equal(wd.grad, torch.zeros_like(wd.grad)) and xd.grad.shape == (0, d)
    xd, wd = gen(5, 1028, seed=1).to(DEV).requires_grad_(True), torch.ones(1028, device=DEV, requires_grad=True)
    y, _yb = GF.RMSNormFn.apply(xd, wd, EPS)      # the forward has no width limit ...
    close("rmsnorm/d1028/y", y, R.rmsnorm_fwd(xd, wd, EPS)[0], 1e-5, 1e-6)
    with pytest.raises(GaotError):                # ... the backward keeps a row's weight-gradient terms in four float4 per lane
        y.sum().backward()
    with pytest.raises(GaotError):
        GF.RMSNormFn.apply(gen(5, 6, seed=1).to(DEV), torch.ones(6, device=DEV), EPS)


# ---- SwiGLU (fp32) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 77])
@pytest.mark.parametrize("f", [4, 12, 128, 1020])
def test_swiglu_fp32(rows, f):
    """u = silu(a) g and d(a | g) at the activation bar with |v| = |a|, times the factor the activation is multiplied by: |g| for u,
    |du g| for da, |du| for dg.  a carries 0, +-20, +-88 (exp at the end of the range) and +-100 (exp overflows: sigmoid is 0 or 1)"""
    from gaot_3d_amd import functional as GF
    ag, du = gen(rows, 2 * f, seed=4, scale=4.0), gen(rows, f, seed=5)
    planted = torch.tensor([0.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0])
    a_flat = ag[:, :f].reshape(-1).clone()
    k = min(planted.numel(), a_flat.numel())
    a_flat[torch.arange(k) * (a_flat.numel() // k)] = planted[:k]           # spread over the rows
    ag[:, :f] = a_flat.view(rows, f)
    a, g = ag[:, :f].double(), ag[:, f:].double()
    ad = ag.to(DEV).requires_grad_(True)
    u = GF.SwiGLUFn.apply(ad, f)
    (u * du.to(DEV)).sum().backward()
    u_ref, dag_ref = R.swiglu_fwd(ag, f), R.swiglu_bwd(ag, du, f)
    floor = 4e-7 * a.abs().clamp(min=1.0)
    within(f"swiglu/r{rows}/f{f}/u", u, u_ref, 4e-6 * u_ref.abs() + floor * g.abs())
    bar = torch.cat([4e-6 * dag_ref[:, :f].abs() + floor * (du.double() * g).abs(), 4e-6 * dag_ref[:, f:].abs() + floor * du.double().abs()], dim=1)
    within(f"swiglu/r{rows}/f{f}/dag", ad.grad, dag_ref, bar)


# ---- RoPE --------------------------------------------------------------------------------------------------------------------------
def _rope_case(tag, rows, s, nheads, hd, col0):
    """in place on a [rows, ld] buffer with ld larger than the rotated span.  Bar per pair: 2e-6 (|x0| + |x1|) -- two products and a sum
    in fp32 and sincosf at two ulps; the inverse call returns the input within twice that"""
    from gaot_3d_amd import ops
    ld = col0 + nheads * hd + 6
    x = gen(rows, ld, seed=6)
    fr = R.rope_freqs(hd)
    ref = R.rope(x, ld, col0, nheads, hd, s, fr)
    mass = R.rope_pair_mass(x, ld, col0, nheads, hd)
    xd = x.to(DEV).clone()
    ops.rope_(xd, rows, ld, col0, nheads, s, fr.to(DEV), False, head_dim=hd)
    within(f"rope/{tag}/fwd", xd, ref, 2e-6 * mass)
    out = xd.cpu()
    lo, hi = col0, col0 + nheads * hd
    assert torch.equal(bits(out[:, :lo]), bits(x[:, :lo])) and torch.equal(bits(out[:, hi:]), bits(x[:, hi:])), tag
    assert not torch.equal(out[1:, lo:hi], x[1:, lo:hi])
    ops.rope_(xd, rows, ld, col0, nheads, s, fr.to(DEV), True, head_dim=hd)
    within(f"rope/{tag}/roundtrip", xd, x.double(), 4e-6 * mass)


@pytest.mark.parametrize("hd", [2, 32, 64, 128])
@pytest.mark.parametrize("nheads", [1, 3])
@pytest.mark.parametrize("col0", [0, 32])
def test_rope_head_dims(hd, nheads, col0):
    _rope_case(f"hd{hd}/h{nheads}/c{col0}", 2 * 50, 50, nheads, hd, col0)         # B = 2, S = 50: position = row % S


def test_rope_long_sequence():
    _rope_case("s16384", 16384, 16384, 1, 32, 0)        # positions up to 16 383: the range reduction of sincosf


# ---- patchify ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,d,h,w,p,c", [(1, 1, 1, 1, 1, 4), (1, 2, 2, 2, 2, 8), (2, 4, 6, 2, 2, 32), (1, 6, 3, 9, 3, 4), (3, 4, 8, 12, 4, 36)])
def test_patchify(b, d, h, w, p, c):
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd import ops
    grid = gen(b, d * h * w, c, seed=7)
    tok_ref = R.patchify(grid, b, d, h, w, p, c)
    tok = ops.patchify(grid.to(DEV), b, d, h, w, p, c, True)
    same = torch.equal(tok.cpu().view(tok_ref.shape), tok_ref)
    back = torch.equal(ops.patchify(tok, b, d, h, w, p, c, False).cpu(), grid)
    print(f"[parity] patchify/{(b, d, h, w, p, c)}: to_tokens {'bit-identical' if same else 'DIFFERS'}, to_grid {'bit-identical' if back else 'DIFFERS'}")
    assert same and back
    # PatchifyFn's backward is the inverse move of the gradient, both ways
    gt = gen(*tok_ref.shape, seed=8)
    leaf = grid.to(DEV).requires_grad_(True)
    out = GF.PatchifyFn.apply(leaf, b, d, h, w, p, c, True)
    (out.view(tok_ref.shape) * gt.to(DEV)).sum().backward()
    assert torch.equal(leaf.grad.cpu(), R.unpatchify(gt, b, d, h, w, p, c))
    leaf2 = tok_ref.contiguous().to(DEV).requires_grad_(True)
    out2 = GF.PatchifyFn.apply(leaf2, b, d, h, w, p, c, False)
    (out2.view(grid.shape) * grid.to(DEV)).sum().backward()
    assert torch.equal(leaf2.grad.cpu().view(tok_ref.shape), tok_ref)


def test_patchify_rejects():
    from gaot_3d_amd import ops
    from gaot_3d_amd._lib import GaotError
    with pytest.raises(GaotError):
        ops.patchify(gen(1, 4 * 6 * 3, 8).to(DEV), 1, 4, 6, 3, 2, 8, True)       # 3 is not divisible by the patch size
    with pytest.raises(GaotError):
        ops.patchify(gen(1, 8, 6).to(DEV), 1, 2, 2, 2, 2, 6, True)               # channels: multiples of 4


# ---- MSE ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 255, 256, 257, 3702, 262144 + 77, 1000003])
def test_mse(n):
    """values near 1e3 whose differences are near 1e-3 (a float accumulation of the squares, or a subtraction after a rounding, loses
    them).  n > 1024 * 256: k_mse_part's grid-stride loop; more than 64 blocks: k_mse_final's stride-64 loop.  Loss: the accumulation is
    double and rounded once (2e-7 relative); gradient: (p - t) is exact, then coef and two products round (4e-7 relative)"""
    from gaot_3d_amd import functional as GF
    p = gen(n, seed=8) + 1e3
    t = p + gen(n, seed=9) * 1e-3
    up = float(torch.tensor(1.7, dtype=torch.float32))
    runs = []
    for _ in range(2):
        pd = p.to(DEV).requires_grad_(True)
        loss = GF.mse_loss(pd, t.to(DEV))
        (loss * 1.7).backward()
        runs.append((loss.detach(), pd.grad))
    l_ref, g_ref = R.mse_fwd(p, t), R.mse_bwd(p, t, up)
    within(f"mse/n{n}/loss", runs[0][0], l_ref, 2e-7 * l_ref.abs())
    within(f"mse/n{n}/grad", runs[0][1], g_ref, 4e-7 * g_ref.abs())
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ---- column sums -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,ld", [(1, 1, 1), (63, 5, 5), (33, 33, 35), (64, 4, 8), (65, 36, 36), (100, 132, 136), (7001, 72, 80), (16500, 8, 8)])
def test_colsum(m, n, ld):
    """the scalar kernel (N or ld no multiple of 4) and the float4 kernel, each with ld > N (the pad columns are NaN: a read past a
    row's N columns shows), a second column block, two chunks, and M > 16 384 where the 256-chunk cap leaves the trailing chunks empty.
    Bar per column: L 2^-24 sum|x| with L the longest addition chain of the two-stage order (rowops_ref.colsum_chain)"""
    from gaot_3d_amd import ops
    x = gen(m, ld, seed=10)
    if m == 7001:
        x[:, 3] = gen(m, seed=11) + 1e4 * (1.0 - 2.0 * (torch.arange(m) % 2))    # +-1e4 alternating, plus unit noise
    x[:, n:] = float("nan")
    ref, mass = R.colsum(x, n)
    xd = x.to(DEV)
    out = ops.colsum(xd, m, n, ld)
    within(f"colsum/{(m, n, ld)}", out, ref, R.colsum_chain(m) * U * mass)
    assert torch.equal(out, ops.colsum(xd, m, n, ld))


# ---- scale mix ---------------------------------------------------------------------------------------------------------------------
def _pm80(rows, ns):
    return torch.where(torch.rand(rows, ns, generator=torch.Generator().manual_seed(9)) < 0.5, -80.0, 80.0)


@pytest.mark.parametrize("ns", [1, 2, 3, 8])
def test_scale_mix(ns):
    """1 .. 8 scales (the unrolled backward's whole range); odd row counts leave the last wave half full (two rows per wave).  Logits:
    unit scale, all equal (weights exactly 1/ns), and a +-80 spread: every logit is -80 or +80, so the weights are equal shares among a
    row's +80s and exp(-160), which fp32 flushes to zero, elsewhere.  (Logits drawn from the whole interval put one weight within an
    ulp of 1; dlogits_s = w_s (<dout, x_s> - sum_t w_t <dout, x_t>) is then the difference of two numbers ~5 that agree to an ulp,
    4.8e-7, which an absolute bar of 1e-6 does not hold in fp32: torch's own fp32 autograd misses it by 1.4x on such rows.)
    Bars: the existing test's"""
    from gaot_3d_amd import functional as GF
    for rows in (1, 2, 3, 7, 500, 513):
        xs = [gen(rows, 32, seed=20 + s) for s in range(ns)]
        go = gen(rows, 32, seed=8)
        for kind, lg in (("unit", gen(rows, ns, seed=7)), ("equal", torch.full((rows, ns), 0.3)),
                         ("spread", _pm80(rows, ns))):
            tag = f"scalemix/s{ns}/r{rows}/{kind}"
            dx = [t.to(DEV).requires_grad_(True) for t in xs]
            dlg = lg.to(DEV).requires_grad_(True)
            out = GF.ScaleMixFn.apply(dlg, *dx)
            (out * go.to(DEV)).sum().backward()
            out_ref, _w = R.scale_mix_fwd(lg, xs)
            dlog_ref, dxs_ref = R.scale_mix_bwd(lg, xs, go)
            close(f"{tag}/out", out, out_ref, 1e-5, 1e-6)
            close(f"{tag}/dlogits", dlg.grad, dlog_ref, 1e-4, 1e-6)
            for s in range(ns):
                close(f"{tag}/dx{s}", dx[s].grad, dxs_ref[s], 1e-5, 1e-6)


def test_scale_mix_rejects():
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd._lib import GaotError
    with pytest.raises(GaotError):
        GF.ScaleMixFn.apply(gen(4, 9).to(DEV), *[gen(4, 32, seed=s).to(DEV) for s in range(9)])
    with pytest.raises(GaotError):
        GF.ScaleMixFn.apply(gen(4, 2).to(DEV), *[gen(4, 16, seed=s).to(DEV) for s in range(2)])


# ---- axpy --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_axpy_with_a_period(n):
    """out = a + alpha b[i % period]: a product and a sum, 2^-24 each (1.2e-7 (|a| + |alpha b|))"""
    from gaot_3d_amd import ops
    a = gen(n, seed=1)
    for period in (n, 1, 7, 32):
        b = gen(period, seed=2)
        for alpha in (1.0, -0.37):
            ref = R.axpy(a, b, alpha, period)
            al = float(torch.tensor(alpha, dtype=torch.float32))
            mass = a.double().abs() + (al * b.double()[torch.arange(n) % period]).abs()
            out = ops.axpy(a.to(DEV), b.to(DEV), alpha, None if period == n else period)
            within(f"axpy/n{n}/p{period}/a{alpha}", out, ref, 1.2e-7 * mass)
    out = ops.axpy(a.to(DEV), a.to(DEV), -0.37, n)      # the period given and equal to n
    within(f"axpy/n{n}/p=n", out, R.axpy(a, a, -0.37, n), 1.2e-7 * 1.37 * a.double().abs())


# ---- bf16 casts --------------------------------------------------------------------------------------------------------------------
def _special_floats():
    """halfway patterns of both parities (round to even: down, then up), their neighbours, +-0, +-inf, NaNs (one whose payload lives in
    the DROPPED bits only: a truncation would make it an infinity), subnormals (halfway ones too, and the largest, which rounds up into
    the normals), the largest finite float (rounds to infinity) and the largest that stays finite"""
    pats = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
            0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0x00000001, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x807FFFFF,
            0x80018000, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F7F8000]
    return torch.tensor([p - (1 << 32) if p >= (1 << 31) else p for p in pats], dtype=torch.int32).view(torch.float32)


def _cast_input(n, seed=0):
    sp = _special_floats()
    if n <= 2 * sp.numel():
        return sp.roll(n).repeat(-(-n // sp.numel()))[:n].clone()     # another stretch of the specials for every n
    x = gen(n, seed=seed)
    x[:sp.numel()] = sp
    x[-sp.numel():] = sp.flip(0)      # ... and in the tail elements the last thread walks one by one
    return x


def _same_bf16(tag, got, x):
    """bit-equal to the CPU's round-to-nearest-even cast of x, NaN where it is NaN (any payload)"""
    want = x.cpu().contiguous().bfloat16()
    got = got.cpu()
    assert got.dtype == torch.bfloat16 and got.shape == want.shape, (tag, got.shape, want.shape)
    nan = torch.isnan(want)
    ok = torch.equal(torch.isnan(got), nan) and torch.equal(bits(got)[~nan], bits(want)[~nan])
    nbad = int((bits(got)[~nan] != bits(want)[~nan]).sum()) if got.shape == want.shape else -1
    print(f"[parity] {tag}: {'bit-identical' if ok else f'DIFFERS in {nbad} elements'} ({want.numel()} elements, {int(nan.sum())} NaN)")
    assert ok, tag


@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 2049])
def test_cast_bf16_bits(n):
    from gaot_3d_amd import ops
    x = _cast_input(n)
    _same_bf16(f"cast_bf16/n{n}", ops.cast_bf16(x.to(DEV)), x)
    _same_bf16(f"cast_bf16_multi/n{n}", ops.cast_bf16_multi([x.to(DEV)])[0], x)


def test_cast_bf16_multi_many_tensors():
    """70 tensors: more than one 64-entry table; empty ones are skipped inside a table and their outputs stay empty"""
    from gaot_3d_amd import ops
    shapes = [(0,), (1,), (7,), (8,), (3, 3), (0, 5), (300,), (2049,), (24, 40), (9,)]
    xs = [_cast_input(int(torch.Size(shapes[i % len(shapes)]).numel()), seed=i).view(shapes[i % len(shapes)]) for i in range(70)]
    outs = ops.cast_bf16_multi([x.to(DEV) for x in xs])
    assert len(outs) == 70
    for i, (o, x) in enumerate(zip(outs, xs)):
        _same_bf16(f"cast_bf16_multi/70/{i}", o, x)
    assert ops.cast_bf16_multi([]) == []


def test_cast_bf16_multi_of_strided_views_casts_each_input():
    """three transposed views of equal size: the contiguous copy the wrapper makes of one must not be released -- and its block handed
    to the next one's copy -- before the launch (every output was the cast of the LAST input's data)"""
    from gaot_3d_amd import ops
    bases = [(gen(40, 24, seed=30 + i) + 10.0 * i).to(DEV) for i in range(3)]
    views = [b.t() for b in bases]
    assert not any(v.is_contiguous() for v in views)
    for i, o in enumerate(ops.cast_bf16_multi(views)):
        assert o.shape == (24, 40)
        _same_bf16(f"cast_bf16_multi/strided/{i}", o, views[i].contiguous())
    for i, o in enumerate(ops.cast_bf16_transpose_multi(views)):      # the transpose of a transposed view: the base matrix
        assert o.shape == (40, 24)
        _same_bf16(f"cast_bf16_transpose_multi/strided/{i}", o, bases[i])
    mixed = [bases[0], views[1], bases[2][:, :8], bases[1]]           # contiguous ones among them, and a column slice
    for i, o in enumerate(ops.cast_bf16_transpose_multi(mixed)):
        _same_bf16(f"cast_bf16_transpose_multi/mixed/{i}", o, mixed[i].t().contiguous())


def test_cast_bf16_of_a_strided_view_follows_the_shape():
    """the cast of a transposed view is the cast of what the view shows (or a refusal) -- never of the storage order"""
    from gaot_3d_amd import ops
    from gaot_3d_amd._lib import GaotError
    base = gen(40, 24, seed=40).to(DEV)
    try:
        out = ops.cast_bf16(base.t())
    except GaotError:
        return
    assert out.shape == (24, 40)
    _same_bf16("cast_bf16/strided", out, base.t().contiguous())


def test_cast_bf16_transpose_multi_rejects_what_is_no_matrix():
    from gaot_3d_amd import ops
    from gaot_3d_amd._lib import GaotError
    with pytest.raises(GaotError):
        ops.cast_bf16_transpose_multi([gen(4, 8).to(DEV), gen(2, 4, 8).to(DEV)])
    with pytest.raises(GaotError):
        ops.cast_bf16_multi([gen(4, 8).to(DEV), gen(4, 8).double().to(DEV)])
