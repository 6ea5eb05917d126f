"""The bf16 Transformer block's row-block kernels (csrc/ffn_fused.hip) and weight-gradient products against an fp64 restatement
(tests/block_ref.py), launch by launch, then a whole L = 2 / L = 3 Transformer in bf16 mode against the oracle in fp64.

Bounds (achieved values: the [parity] lines of the parity log):
  * fp32 outputs (h, y, xo, dh, dx, dxa / dxb, delta, rstd): max |err| <= 1e-5 x peak -- fp32 accumulation of bf16 products.
  * bf16 outputs (image, yb, dO image, dag, u, dyb): bf16(fp64 value) except rounding-boundary flips of one ulp (<= 1e-3 of the
    elements); more than one ulp only where the kernel re-rounds an intermediate the reference cannot take from it (named below).
    An element within 1e-5 x peak of the fp64 value counts as equal: a result that cancels to ~1e-5 of its terms carries the fp32
    accumulation's error in its leading bits (measured: up to a few hundred ulps on such elements of the image and of yb).
  * column sums (the two norm-weight gradients, the weight-gradient products): |err_j| <= 1e-5 x sum over the rows of |term_ij|,
    with the deferred completion (ops.defer_reductions) on and off -- and the two bit-identical."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import gaot_oracle as orc  # noqa: E402  (checker only)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_ref as R  # noqa: E402
import parity as PAR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-6
SCALE = 1.0 / (32 ** 0.5)

# Bounds per check, each <= 3 x the worst value measured on the MI355X over CASES (in the comment) and at least as tight as the module
# docstring's.  fp32 outputs: max |err| / peak; column sums: max |err_j| / sum_rows |term_ij|; bf16 outputs: (fraction of one-ulp flips,
# fraction beyond one ulp).  dag and u may move by more than one ulp: the backward kernel recomputes a | g from yb and rounds it to bf16
# without writing it, and du = dy W2 likewise; where the fp64 a | g or du rounds the other way -- a one-ulp flip of an INPUT of the
# SwiGLU or its derivative -- the result moves by up to two ulps.  Flip fractions are granular at 70 rows (one element = 5.6e-5 of yb).
FP32 = {"xo": 1.2e-6,           # 4.25e-7
        "rstd": 4.9e-7,         # 1.63e-7
        "h": 1.6e-6,            # 5.51e-7
        "y": 1.3e-6,            # 4.57e-7
        "dh": 3.2e-6,           # 1.08e-6
        "delta": 4.9e-7,        # 1.66e-7
        "dx": 1.3e-6,           # 4.58e-7
        "dxa": 9.6e-7,          # 3.21e-7
        "dxb": 7.3e-7}          # 2.44e-7
COLSUM = {"d(attn_norm.weight)": 4.2e-7,   # 1.42e-7
          "d(ffn_norm.weight)": 8.5e-7,    # 2.85e-7
          "dW2": 5.9e-7,                   # 2.00e-7
          "dW13": 6.8e-7,                  # 2.29e-7
          "dWo": 3.2e-7,                   # 1.09e-7
          "dWqkv": 4.1e-7,                 # 1.38e-7
          "dWskip": 3.4e-7}                # 1.16e-7
BF16 = {"yb": (1.6e-4, 0.0),             # 5.58e-5, 0
        "image": (8.4e-5, 0.0),          # 2.81e-5, 0
        "dO image": (1.6e-4, 0.0),       # 5.58e-5, 0
        "dyb": (0.0, 0.0),               # a cast: exact
        "u": (1.2e-4, 2.9e-5),           # 4.08e-5, 9.77e-6
        "dag": (1.2e-4, 6.2e-5)}         # 4.29e-5, 2.09e-5


def _fp32(rep, name, got, ref):
    rep.fp32(name, got, ref, FP32[name.rsplit("/", 1)[-1]])


def _bf16(rep, name, got, ref):
    flips, beyond = BF16[name.rsplit("/", 1)[-1]]
    rep.bf16(name, got, ref, flips=flips, beyond=beyond)


# (rows, batch, F, kv heads, rope, head kind, dres, dtap, same): every row count meets every kernel -- the encoder head (norm_qkv,
# qkv_bwd_norm), the decoder head (cat_norm_qkv, qkv_bwd_norm_cat) and, in each case, block_tail, ffn_bwd_norm, oproj_bwd and the
# weight-gradient products
CASES = [
    (16384, 1, 1024, 8, True, "enc", True, True, None),        # configs[1]
    (16384, 1, 1024, 8, True, "cat", True, False, True),
    (16384, 1, 128, 4, False, "enc", False, False, None),
    (8192, 2, 1024, 4, True, "enc", True, False, None),         # one rank's share at G = 2 (two sequences of 4096: RoPE position = row % S)
    (8192, 1, 128, 4, True, "cat", False, False, False),
    (4096, 1, 128, 8, False, "enc", False, True, None),
    (4096, 1, 1024, 8, False, "cat", True, False, True),
    (4096, 1, 1024, 4, True, "enc", False, True, None),
    (2048, 1, 128, 4, True, "enc", True, True, None),
    (2048, 1, 1024, 8, True, "cat", True, False, False),
    (1024, 1, 1024, 8, True, "enc", False, False, None),
    (1024, 1, 128, 4, False, "cat", False, False, True),
    (16384 - 37, 1, 1024, 4, True, "enc", True, True, None),   # ragged last 64-row block
    (16384 - 37, 1, 128, 8, True, "cat", True, False, False),
    (1000, 1, 1024, 8, False, "enc", True, False, None),
    (1000, 1, 1024, 4, True, "cat", True, False, True),
    (70, 1, 128, 4, True, "enc", True, True, None),
    (70, 1, 128, 8, False, "cat", False, False, False),
    (70, 1, 1024, 8, True, "enc", False, False, None),
    (2048, 1, 1024, 4, False, "cat", False, False, True),
]


def _ids(c):
    rows, b, f, kv, rope, kind, dres, dtap, same = c
    s = f"{kind}-r{rows}" + (f"x{b}" if b > 1 else "") + f"-F{f}-kv{kv}-{'rope' if rope else 'abs'}"
    s += ("-dres" if dres else "") + ("-dtap" if dtap else "")
    return s + ("" if same is None else f"-same{int(same)}")


def _lin(n, k, g):
    return (torch.randn(n, k, generator=g) / k ** 0.5).to(DEV)


@pytest.mark.parametrize("case", CASES, ids=[_ids(c) for c in CASES])
def test_block_kernels_vs_fp64(case):
    from gaot_3d_amd import ops
    rows, b, f, kv, rope, kind, with_dres, with_dtap, same = case
    s, nh = rows // b, 8
    n = (nh + 2 * kv) * 32
    g = torch.Generator().manual_seed(rows * 7 + f + kv)
    wqkv, wo, w13, w2 = _lin(n, 256, g), _lin(256, 256, g), _lin(2 * f, 256, g), _lin(256, f, g)
    nw1 = (1.0 + 0.2 * torch.randn(256, generator=g)).to(DEV)      # norm weights that are not all ones
    nw2 = (1.0 + 0.2 * torch.randn(256, generator=g)).to(DEV)
    x = torch.randn(rows, 256, generator=g).to(DEV)
    freqs = (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32))).to(DEV) if rope else None
    table = ops.rope_table(freqs, s) if rope else None
    qs = ops._qscale(SCALE)
    rep = R.Report(f"block {_ids(case)}")
    qkv_packed = ops.qkv_pack_multi([wqkv], True)[0]
    blk_packed = ops.block_pack_multi([(w13, w2, wo)], f)[0]

    # ---- head: attn_norm -> q | k | v -> RoPE -> image (encoder) / skip_proj in front (decoder) ----
    if kind == "enc":
        img, yb, rstd = ops.norm_qkv_image(x, nw1, EPS, qkv_packed, b, s, nh, kv, freqs, SCALE)
        xres = x
        ref = R.head(x, nw1, EPS, wqkv, yb, table, s, nh, kv, qs)
        name = "norm_qkv"
    else:
        xa = x
        xb = x if same else torch.randn(rows, 256, generator=g).to(DEV)
        wsk, bsk = _lin(256, 512, g), (0.1 * torch.randn(256, generator=g)).to(DEV)
        spk = ops.skip_pack_multi([wsk])[0]
        img, xo, yb, rstd = ops.cat_norm_qkv_image(xa, xb, spk, bsk, nw1, EPS, qkv_packed, b, s, nh, kv, freqs, SCALE)
        xres = xo
        ref = R.cat_head(xa, xb, wsk, bsk, nw1, EPS, wqkv, yb, table, s, nh, kv, qs)
        name = "cat_norm_qkv"
        _fp32(rep, f"{name}/xo", xo, ref["xo"])
    image = img[:rows * n * 2].view(torch.bfloat16).view(rows, n)
    _bf16(rep, f"{name}/yb", yb, ref["yb"])
    _fp32(rep, f"{name}/rstd", rstd, ref["rstd"])
    _bf16(rep, f"{name}/image", image, ref["image"])

    # ---- attention (pinned against fp64 in test_fullsize_oracle_gpu.py): its output feeds the block's tail ----
    o, _lse, _ = ops.attn_fwd_bf16(None, freqs, b, s, nh, kv, SCALE, image=img)

    # ---- tail: o_proj + residual -> ffn_norm -> FFN -> + the normalised rows ----
    y, h, ybt, rstd2 = ops.block_tail_fwd(o, xres, nw2, EPS, blk_packed, f)

    # ---- backward: ffn_bwd_norm, oproj_bwd_image, qkv_bwd_norm(_cat), with the deferred completion off and on ----
    dy = (0.1 * torch.randn(rows, 256, generator=g)).to(DEV)
    dqkv = (0.05 * torch.randn(rows, n, generator=g)).to(DEV)
    dres = (0.1 * torch.randn(rows, 256, generator=g)).to(DEV) if with_dres else None
    dtap = (0.1 * torch.randn(rows, 256, generator=g)).to(DEV) if with_dtap else None
    outs = {}
    prev = ops.defer_reductions(False)
    try:
        for defer in (False, True):
            ops.defer_reductions(defer)
            dh, dag, u, dyb, dnw2 = ops.ffn_bwd_norm(ybt, dy, blk_packed, f, h, nw2, rstd2, defer=defer)
            doimg, delta = ops.oproj_bwd_image(dh, o, blk_packed, f, b, s, nh, kv)
            doimg = doimg[:rows * 256 * 2].view(torch.bfloat16).view(rows, 256)    # the image heads the backward's scratch
            if kind == "enc":
                dx, dnw1 = ops.qkv_bwd_norm(dqkv, qkv_packed, x, nw1, rstd, dres, dtap, defer=defer)
                dxa = dxb = None
            else:
                dx, dxa, dxb, dnw1 = ops.qkv_bwd_norm_cat(dqkv, qkv_packed, xo, nw1, rstd, dres, spk, same, defer=defer)
            # the weight-gradient products as the block's backward issues them (BlockTailFn, NormQKVFn / CatNormQKVFn.backward)
            dws = {"dW2": ops.gemm_dw(dyb, u, 256, f, rows, 256, f, 1, defer=defer),
                   "dW13": ops.gemm_dw(dag, ybt, 2 * f, 256, rows, 2 * f, 256, 1, defer=defer),
                   "dWo": ops.gemm_dw(dh, o, 256, 256, rows, 256, 256, 1, defer=defer),
                   "dWqkv": ops.gemm_dw(dqkv, yb, n, 256, rows, n, 256, 1, defer=defer)}
            if kind == "cat":
                dwsk = torch.empty(256, 512, device=DEV)
                ops.gemm(dx, xa, 256, 256, rows, 256, 256, True, False, out=dwsk, ldc=512, precision=1)
                ops.gemm(dx, xb, 256, 256, rows, 256, 256, True, False, out=dwsk[:, 256:], ldc=512, precision=1)
                dws["dWskip"] = dwsk
            pending = ops.deferred_pending()
            ops.flush_deferred()
            torch.cuda.synchronize()
            outs[defer] = dict(dh=dh, dag=dag, u=u, dyb=dyb, dnw2=dnw2, doimg=doimg, delta=delta, dx=dx, dxa=dxa, dxb=dxb, dnw1=dnw1,
                               pending=pending, **dws)
    finally:
        ops.defer_reductions(prev)
    off, on = outs[False], outs[True]
    assert off["pending"] == 0 and on["pending"] > 0, (off["pending"], on["pending"])   # the deferral was exercised
    for k in off:
        if isinstance(off[k], torch.Tensor):
            rep.exact(f"defer on = off/{k}", on[k], off[k])

    # references, stage by stage, from what each kernel read
    rt = R.tail(o, xres, wo, nw2, EPS, w2, off["u"])
    _fp32(rep, "block_tail/h", h, rt["h"])
    _bf16(rep, "block_tail/yb", ybt, rt["yb"])
    _fp32(rep, "block_tail/rstd", rstd2, rt["rstd"])
    _fp32(rep, "block_tail/y", y, rt["y"])
    rf = R.ffn_bwd_norm(ybt, dy, w13, w2, f, h, nw2, rstd2, off["dag"])
    _bf16(rep, "ffn_bwd_norm/dyb", off["dyb"], rf["dyb"])
    _bf16(rep, "ffn_bwd_norm/u", off["u"], rf["u"])
    _bf16(rep, "ffn_bwd_norm/dag", off["dag"], rf["dag"])
    _fp32(rep, "ffn_bwd_norm/dh", off["dh"], rf["dh"])
    ro = R.oproj_bwd(off["dh"], o, wo, b, s, nh)
    _bf16(rep, "oproj_bwd/dO image", off["doimg"], ro["do"])
    _fp32(rep, "oproj_bwd/delta", off["delta"], ro["delta"])
    if kind == "enc":
        rq = R.qkv_bwd_norm(dqkv, wqkv, x, nw1, rstd, dres, dtap)
        _fp32(rep, "qkv_bwd_norm/dx", off["dx"], rq["dx"])
    else:
        rq = R.qkv_bwd_norm(dqkv, wqkv, xo, nw1, rstd, dres, None)
        _fp32(rep, "qkv_bwd_norm_cat/dx", off["dx"], rq["dx"])
        rs = R.skip_bwd(off["dx"], wsk, same)
        _fp32(rep, "qkv_bwd_norm_cat/dxa", off["dxa"], rs["dxa"])
        if not same:
            _fp32(rep, "qkv_bwd_norm_cat/dxb", off["dxb"], rs["dxb"])
    head_bwd = "qkv_bwd_norm" if kind == "enc" else "qkv_bwd_norm_cat"
    operands = {"dW2": (off["dyb"], off["u"]), "dW13": (off["dag"], ybt), "dWo": (off["dh"], o), "dWqkv": (dqkv, yb)}
    if kind == "cat":
        operands["dWskip"] = (off["dx"], torch.cat([xa, xb], dim=1))
    for defer, res in outs.items():
        sfx = "deferred" if defer else "in call"
        rep.colsum(f"ffn_bwd_norm/d(ffn_norm.weight) {sfx}", res["dnw2"], rf["dnw"], rf["dnw_mass"], COLSUM["d(ffn_norm.weight)"])
        rep.colsum(f"{head_bwd}/d(attn_norm.weight) {sfx}", res["dnw1"], rq["dnw"], rq["dnw_mass"], COLSUM["d(attn_norm.weight)"])
    for k, (a_, b_) in operands.items():
        val, mass = R.dw(a_, b_)
        for defer, res in outs.items():
            rep.colsum(f"{k} {'deferred' if defer else 'in call'}", res[k], val, mass, COLSUM[k])
    rep.done()


# ---- the whole block: a Transformer in bf16 mode against the oracle in fp64 ----
# bounds: WHOLE_BOUNDS below
WHOLE = [(2, 4096, 1024, 8, True), (3, 2000, 128, 4, False)]


@pytest.mark.parametrize("layers,s,f,kv,rope", WHOLE, ids=[f"L{c[0]}-S{c[1]}-F{c[2]}-kv{c[3]}-{'rope' if c[4] else 'abs'}" for c in WHOLE])
def test_transformer_bf16_vs_fp64_oracle(layers, s, f, kv, rope):
    """L = 2: one encoder and one decoder block -- the encoder block's output is the decoder's input AND its skip (the CAT head with
    same = True).  L = 3: encoder, middle, decoder -- the middle block's attention norm hands the skip on as its tap (dtap) and the
    decoder's two inputs differ (same = False).  Every parameter gradient, no energy filter."""
    import gaot_3d_amd
    from gaot_3d_amd.model.layers.attn import AttentionConfig, FFNConfig, Transformer, TransformerConfig
    torch.manual_seed(11 + layers)
    cfg = TransformerConfig(patch_size=2, hidden_size=256, num_layers=layers, positional_embedding="rope" if rope else "absolute",
                            attn_config=AttentionConfig(hidden_size=256, num_heads=8, num_kv_heads=kv, atten_dropout=0.0),
                            ffn_config=FFNConfig(hidden_size=f))
    model = Transformer(256, 256, cfg).to(DEV).train()
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("norm.weight"):
                p.add_(0.2 * torch.randn_like(p))
    x = torch.randn(1, s, 256, device=DEV)
    w = torch.randn(1, s, 256, device=DEV)
    # fp64 oracle on the device; the RoPE angles position x frequency formed in fp32, as the reference does on fp32 tensors
    sd = {k: (v.detach().clone() if k.endswith("rotary_emb.freqs") else v.detach().double()) for k, v in model.state_dict().items()}
    for v in sd.values():
        v.requires_grad_(v.dtype == torch.float64)
    xr = x.double().requires_grad_(True)
    with torch.device(DEV):      # (the oracle's position vectors are made with the default device)
        out_r = orc.transformer(sd, "", xr, cfg, rope)
    (out_r * w.double()).sum().backward()
    gaot_3d_amd.set_precision("bf16")
    try:
        xd = x.clone().requires_grad_(True)
        out = model(xd, relative_positions=True if rope else None)
        (out * w).sum().backward()
        torch.cuda.synchronize()
    finally:
        gaot_3d_amd.set_precision("fp32")
    tag = f"transformer_bf16 L={layers} S={s} F={f} kv={kv} {'rope' if rope else 'abs'}"
    got = {"out": out, "d input": xd.grad}
    want = {"out": out_r, "d input": xr.grad}
    for k, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None, k
            got[k], want[k] = p.grad, sd[k].grad
    fails = []
    for k in got:
        bound_l2, bound_peak = WHOLE_BOUNDS[re.sub(r"^(encoder_layers\.\d+|middle_layer|decoder_layers\.\d+)\.", "", k)]
        err, peak, l2 = PAR.stats(got[k], want[k])
        ok = err <= bound_peak * peak and l2 <= bound_l2 and bool(torch.isfinite(got[k]).all())
        print(f"[parity] {tag}/{k}: rel_l2={l2:.3e} (bound {bound_l2:.1e}) max|err|/peak={err / max(peak, 1e-300):.3e} "
              f"(bound {bound_peak:.1e})")
        if not ok:
            fails.append(k)
    assert not fails, f"{tag}: {fails}"


# tensor (name past the block prefix) -> (relative L2, max |err| / peak): 3 x the worst of the two cases and of the blocks measured on the
# MI355X (in the comment), rounded down.  Every tensor is some 5e-3 off in relative L2: bf16 operands through two blocks
WHOLE_BOUNDS = {"out": (7.6e-3, 7.5e-3),                   # 2.54e-3, 2.51e-3
                "d input": (8.1e-3, 8.3e-3),               # 2.72e-3, 2.78e-3
                "attn.q_proj.weight": (1.7e-2, 1.8e-2),    # 5.79e-3, 6.11e-3
                "attn.k_proj.weight": (1.6e-2, 1.7e-2),    # 5.66e-3, 6.00e-3
                "attn.v_proj.weight": (1.4e-2, 1.4e-2),    # 4.96e-3, 4.95e-3
                "attn.o_proj.weight": (1.5e-2, 1.3e-2),    # 5.25e-3, 4.45e-3
                "ffn.w1.weight": (1.8e-2, 1.8e-2),         # 6.08e-3, 6.22e-3
                "ffn.w2.weight": (1.7e-2, 1.9e-2),         # 5.91e-3, 6.43e-3
                "ffn.w3.weight": (1.7e-2, 2.0e-2),         # 5.93e-3, 6.69e-3
                "attn_norm.weight": (1.6e-2, 1.9e-2),      # 5.37e-3, 6.63e-3
                "ffn_norm.weight": (8.4e-3, 1.1e-2),       # 2.83e-3, 3.88e-3
                "skip_proj.weight": (7.7e-3, 7.5e-3),      # 2.59e-3, 2.52e-3
                "skip_proj.bias": (5.8e-3, 6.1e-3)}        # 1.96e-3, 2.04e-3
