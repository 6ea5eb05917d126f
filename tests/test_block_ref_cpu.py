"""CPU: the comparison helpers of tests/block_ref.py have teeth.  A kernel-like result (fp32 arithmetic, bf16 rounding where the kernels
round) of each stage passes against the fp64 restatement; tampered copies of it -- the faults the bf16 block kernels could make
without anything else noticing -- are rejected."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_ref as R  # noqa: E402

ROWS, F = 1000, 128        # 1000 rows: the last 64-row block holds 40


def _problem():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(ROWS, 256, generator=g)
    nw = 1.0 + 0.2 * torch.randn(256, generator=g)
    wqkv = torch.randn(768, 256, generator=g) / 16
    w13 = torch.randn(2 * F, 256, generator=g) / 16
    w2 = torch.randn(256, F, generator=g) / F ** 0.5
    dqkv = 0.05 * torch.randn(ROWS, 768, generator=g)
    dres = 0.1 * torch.randn(ROWS, 256, generator=g)
    dy = 0.1 * torch.randn(ROWS, 256, generator=g)
    return x, nw, wqkv, w13, w2, dqkv, dres, dy


def _fp32_qkv_bwd_norm(dqkv, wqkv, x, nw, rstd, dres):
    """the stage in fp32 as a kernel computes it: bf16 operands, fp32 products and sums"""
    dn = dqkv.bfloat16().float() @ wqkv.bfloat16().float()
    r = rstd[:, None]
    c = (x * nw * dn).sum(-1, keepdim=True) * r ** 3 / 256
    dx = r * nw * dn - x * c + dres
    return dx, (dn * x * r).sum(0)


def _ok(rep):
    assert not rep.failures, rep.failures


def _rejected(rep, name):
    assert rep.failures and name in rep.failures[-1], rep.failures


def test_norm_weight_gradient_and_input_gradient():
    x, nw, wqkv, _w13, _w2, dqkv, dres, _dy = _problem()
    rstd = torch.rsqrt(x.square().mean(-1) + 1e-6)
    ref = R.qkv_bwd_norm(dqkv, wqkv, x, nw, rstd, dres)
    dx, dnw = _fp32_qkv_bwd_norm(dqkv, wqkv, x, nw, rstd, dres)
    rep = R.Report("teeth")
    rep.fp32("dx", dx, ref["dx"])
    rep.colsum("dnw", dnw, ref["dnw"], ref["dnw_mass"])
    _ok(rep)
    rep.colsum("dnw scaled", dnw * (1 + 1e-3), ref["dnw"], ref["dnw_mass"])                        # norm-weight gradient x (1 + 1e-3)
    _rejected(rep, "dnw scaled")
    dx_nores, _ = _fp32_qkv_bwd_norm(dqkv, wqkv, x, nw, rstd, torch.zeros_like(dres))
    rep.fp32("dx without dres", dx_nores, ref["dx"])                                                # the dres addend dropped
    _rejected(rep, "dx without dres")
    ragged = dx.clone()
    ragged[ROWS // 64 * 64:] = 0.0
    rep.fp32("dx last block zeroed", ragged, ref["dx"])                                              # the ragged last block lost
    _rejected(rep, "dx last block zeroed")


def test_bf16_outputs():
    x, nw, _wqkv, w13, _w2, _dqkv, _dres, _dy = _problem()
    n, _r = R.norm(x, nw, 1e-6)
    a, g, _u = R.swiglu(n.bfloat16(), w13, F)
    u = torch.nn.functional.silu(a) * g
    got = u.float().bfloat16()                 # rounded from fp32: flips at rounding boundaries only
    rep = R.Report("teeth")
    rep.bf16("u", got, u)
    _ok(rep)
    moved = got.clone().view(-1)
    idx = torch.randperm(moved.numel(), generator=torch.Generator().manual_seed(1))[:moved.numel() // 100]
    bits = moved.view(torch.int16)
    bits[idx] += 2                             # 1 % of the elements two ulps away (away from zero: same sign)
    rep.bf16("u moved", moved.view_as(got), u)
    _rejected(rep, "u moved")
    ragged = got.clone()
    ragged[ROWS // 64 * 64:] = 0
    rep.bf16("u last block zeroed", ragged, u)
    _rejected(rep, "u last block zeroed")
    rep.failures.clear()
    rep.bf16("cast", u.bfloat16(), u, flips=0.0)          # a cast (bf16(dy)) is checked with no flips allowed
    _ok(rep)
    flipped = u.bfloat16().view(-1)
    flipped.view(torch.int16)[idx[:10]] += 1                # ten elements one ulp away: a cast that does not round to nearest
    rep.bf16("cast with flips", flipped.view_as(got), u, flips=0.0)
    _rejected(rep, "cast with flips")


def test_weight_gradient_split_k():
    x, nw, _wqkv, w13, w2, _dqkv, _dres, dy = _problem()
    n, _r = R.norm(x, nw, 1e-6)
    _a, _g, u = R.swiglu(n.bfloat16(), w13, F)
    dyb = dy.bfloat16()
    val, mass = R.dw(dyb, u)
    # a split-K product: fp32 partial sums over 4 parts of the rows, summed in order
    bounds = [0, 256, 512, 768, ROWS]
    parts = [dyb[lo:hi].float().t() @ u[lo:hi].float() for lo, hi in zip(bounds, bounds[1:])]
    rep = R.Report("teeth")
    rep.colsum("dW2", sum(parts), val, mass)
    _ok(rep)
    rep.colsum("dW2 one part missing", sum(parts[:2] + parts[3:]), val, mass)
    _rejected(rep, "dW2 one part missing")
    rep.colsum("dW2 last part missing", sum(parts[:3]), val, mass)      # the ragged tail part
    _rejected(rep, "dW2 last part missing")


def test_report_done_names_the_failing_tensor():
    rep = R.Report("case")
    rep.fp32("good", torch.ones(4), torch.ones(4, dtype=torch.float64))
    rep.done()
    rep.fp32("bad", torch.full((4,), 1.001), torch.ones(4, dtype=torch.float64))
    try:
        rep.done()
    except AssertionError as e:
        assert "case/bad" in str(e) and "case/good" not in str(e)
    else:
        raise AssertionError("a missed bound did not fail")
