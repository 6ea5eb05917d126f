"""Flash attention for every head size that is a multiple of 4 up to 128 in bf16 mode (csrc/attn_hd.hip: tile widths 32 / 64 / 96 /
128, padded instances for the sizes in between): against the fp64 oracle through GroupQueryFlashAttention, head by head against
one-head calls (nothing read from or written to a neighbouring head's columns), in O(S) memory, under graph replay, and inside the
whole model.
bf16 bars (tests/test_attn_headdim_gpu.py): output max|err| <= 2e-2 of the peak and relative L2 <= 1e-2; every
gradient cosine >= 0.999 and max|err| <= 2e-2 of its peak."""
import os
import sys

import pytest
import torch

import parity as PAR

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import gaot_oracle as orc  # noqa: E402  (checker only)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _seed_tensor(word):
    return torch.tensor([word - (1 << 64) if word >= (1 << 63) else word], dtype=torch.int64, device=DEV)


def _bars(tag, out, ref, grads):
    PAR.close_peak(f"{tag}/out", out, ref, 2e-2, rel_l2=1e-2)
    for nm, (a, r) in grads.items():
        PAR.cosine(f"{tag}/{nm}", a, r, 0.999)
        PAR.close_peak(f"{tag}/{nm}", a, r, 2e-2)


# head sizes 8 .. 120 x S {5, 33, 77, 130, 257} x batch {1, 2} x (H, HKV) {(2, 2), (4, 2), (4, 1)} x RoPE x p {0, 0.1}, pruned: two
# cases per head size, every head size at least once with dropout and at least once with grouped kv heads.  100 puts the width
# boundary between the two float4s of a lane's 8-column run, 36 is mostly padding, 68 lands in the 96 instance, 96 is the new
# exact instance; 8, 16, 20 run the 32 instance, 48 the 64 instance, 100 and 120 the 128 instance.
_ORACLE_CASES = [
    (8, 5, 1, 2, 2, True, 0.1), (8, 130, 2, 4, 1, False, 0.0),
    (16, 33, 2, 4, 2, False, 0.1), (16, 257, 1, 2, 2, True, 0.0),
    (20, 77, 1, 4, 1, True, 0.1), (20, 5, 2, 2, 2, False, 0.0),
    (36, 130, 2, 2, 2, False, 0.1), (36, 33, 1, 4, 2, True, 0.0),
    (48, 257, 1, 4, 2, True, 0.1), (48, 77, 2, 4, 1, False, 0.0),
    (68, 5, 2, 4, 1, False, 0.1), (68, 130, 1, 2, 2, True, 0.0),
    (96, 33, 1, 2, 2, True, 0.1), (96, 257, 2, 4, 2, False, 0.1),
    (100, 77, 2, 4, 2, False, 0.1), (100, 257, 1, 4, 1, True, 0.0),
    (120, 130, 1, 4, 1, True, 0.1), (120, 5, 2, 2, 2, False, 0.0)]


@pytest.mark.parametrize("d,s,b,h,hkv,rope,p", _ORACLE_CASES)
def test_attention_headsize_matches_fp64_oracle(d, s, b, h, hkv, rope, p):
    """GroupQueryFlashAttention in bf16 mode against the oracle's attention in fp64: forward, dx and the q / k / v / o projection
    weight gradients; the construction of test_attention_hd_matches_fp64_oracle (q / k weights x 3; with dropout the mask the
    kernels regenerate is rebuilt from the seed word, equals the oracle's draw bit for bit and goes into the oracle's SDPA)."""
    import gaot_3d_amd
    from gaot_3d_amd import functional as GF, ops
    from gaot_3d_amd.model.layers.attn import GroupQueryFlashAttention
    hidden = h * d
    torch.manual_seed(d + s)
    att = GroupQueryFlashAttention(hidden, hidden, hidden_size=hidden, num_heads=h, num_kv_heads=hkv, atten_dropout=p,
                                   positional_embedding="rope" if rope else "absolute")
    assert att.head_dim == d
    with torch.no_grad():      # scores of O(1) instead of O(0.1): a softmax with structure (the same weights go to the oracle)
        att.q_proj.weight.mul_(3.0)
        att.k_proj.weight.mul_(3.0)
    sd = {"a." + k: v.detach().clone() for k, v in att.state_dict().items()}
    x = torch.randn(b, s, hidden)
    w = torch.randn(b, s, hidden)
    seed0 = 0xC0FFEE + d + s
    calls = dict(GF.AttentionHdFn.calls)
    gaot_3d_amd.set_precision("bf16")
    try:
        att = att.to(DEV).train()
        xd = x.to(DEV).requires_grad_(True)
        GF.set_dropout_seed(seed0, DEV)
        out = att(xd, relative_positions=True if rope else None)
        (out * w.to(DEV)).sum().backward()
        torch.cuda.synchronize()
    finally:
        gaot_3d_amd.set_precision("fp32")
    assert GF.AttentionHdFn.calls["fwd"] == calls["fwd"] + 1 and GF.AttentionHdFn.calls["bwd"] == calls["bwd"] + 1
    keep, p_eff = None, 0.0
    if p > 0.0:
        p_eff = orc.dropout_threshold(p) / 65536.0
        word = GF.dropout_seed_sequence(seed0, 1)[0]
        keep = ops.attn_dropout_mask(_seed_tensor(word), p, b, h, s).cpu().bool()      # what the kernels regenerate
        assert torch.equal(keep, orc.dropout_keep_mask(word, b, h, s, p))               # bit-exact against the oracle's draw
    leaves = {k: v.double().requires_grad_(v.dtype.is_floating_point and "freqs" not in k) for k, v in sd.items()}
    xr = x.double().requires_grad_(True)
    ref = orc.attention(leaves, "a.", xr, h, hkv, rope, keep, p_eff)
    (ref * w.double()).sum().backward()
    grads = {"dx": (xd.grad, xr.grad)}
    for k, prm in att.named_parameters():
        if prm.requires_grad:
            grads[f"grad/{k}"] = (prm.grad, leaves["a." + k].grad)
    assert {"grad/q_proj.weight", "grad/k_proj.weight", "grad/v_proj.weight", "grad/o_proj.weight"} <= set(grads)
    _bars(f"attn_hs{d}_S{s}_b{b}_h{h}kv{hkv}_rope{int(rope)}_p{p}", out, ref.detach(), grads)


def _qkv(d, s, b, h, hkv, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(b * s, (h + 2 * hkv) * d, generator=g)
    qkv[:, :(h + hkv) * d] *= 1.5          # |score| of O(2): a softmax with structure
    return qkv, torch.randn(b * s, h * d, generator=g)


@pytest.mark.parametrize("d", [20, 100])
def test_attention_headsize_no_leakage_between_heads(d):
    """head j of a 3-head call against a ONE-head call on that head's contiguous q | k | v slice (head0 = j, heads_total = 3: the
    same dropout mask): outputs and dq / dk / dv equal bit for bit.  In the 3-head call the columns right of a head belong to its
    neighbour (to the next ROW for the last head); in the one-head call there is nothing there.  A padded load that sees those
    columns changes the scores; a store that touches them overwrites the neighbour's result."""
    from gaot_3d_amd import ops
    s, b, h, p = 77, 2, 3, 0.1
    qkv, w = _qkv(d, s, b, h, h, 11 + d)
    st = _seed_tensor(0x9E3779B97F4A7C15 ^ d)
    scale = d ** -0.5
    qd, wd = qkv.to(DEV), w.to(DEV)
    oh, lseh = ops.attn_hd_fwd(qd, b, s, h, h, d, scale, p, st)
    gh = ops.attn_hd_bwd(qd, oh, wd, lseh, b, s, h, h, d, scale, p, st)
    torch.cuda.synchronize()
    assert torch.isfinite(oh).all() and torch.isfinite(gh).all()
    for j in range(h):
        sl = torch.cat([qd[:, (i * h + j) * d:(i * h + j + 1) * d] for i in range(3)], dim=1).contiguous()     # q, k, v of head j
        ws = wd[:, j * d:(j + 1) * d].contiguous()
        o1, lse1 = ops.attn_hd_fwd(sl, b, s, 1, 1, d, scale, p, st, head0=j, heads_total=h)
        g1 = ops.attn_hd_bwd(sl, o1, ws, lse1, b, s, 1, 1, d, scale, p, st, head0=j, heads_total=h)
        torch.cuda.synchronize()
        assert torch.equal(o1, oh[:, j * d:(j + 1) * d]), (j, "o")
        assert torch.equal(lse1.reshape(b, s), lseh[:, j]), (j, "lse")
        for i, nm in enumerate(("dq", "dk", "dv")):
            assert torch.equal(g1[:, i * d:(i + 1) * d], gh[:, (i * h + j) * d:(i * h + j + 1) * d]), (j, nm)


def test_attention_headsize_never_holds_an_s_by_s_tensor():
    """S = 16 384, head size 48 (the padded 64 instance), 2 heads on 1 kv head, p = 0.1, forward + backward: one fp32 score matrix
    alone is 1 GiB; the peak above the inputs stays below 256 MiB.  Two runs with the same seed are bit-identical."""
    import gaot_3d_amd
    from gaot_3d_amd import functional as GF
    d, s, b, h, hkv, p = 48, 16384, 1, 2, 1, 0.1
    qkv, w = _qkv(d, s, b, h, hkv, 3)
    freqs = (1.0 / (10000 ** (torch.arange(0, d, 2).float() / d))).to(DEV)
    wd = w.to(DEV)
    x = qkv.to(DEV).requires_grad_(True)
    runs = []
    calls = dict(GF.AttentionHdFn.calls)
    gaot_3d_amd.set_precision("bf16")
    try:
        for i in range(2):
            GF.set_dropout_seed(777, DEV)
            x.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            o = GF.attention_general(x, freqs, b, s, h, hkv, d, p)
            (o * wd).sum().backward()
            torch.cuda.synchronize()
            extra = torch.cuda.max_memory_allocated() - before
            print(f"[memory] attn_hs48_S{s} run {i}: peak above the inputs {extra / 2 ** 20:.1f} MiB")
            assert extra <= 256 * 2 ** 20, f"{extra / 2 ** 20:.1f} MiB allocated above the inputs: an S x S tensor?"
            runs.append((o.detach().clone(), x.grad.clone()))
    finally:
        gaot_3d_amd.set_precision("fp32")
    assert GF.AttentionHdFn.calls["fwd"] == calls["fwd"] + 2 and GF.AttentionHdFn.calls["bwd"] == calls["bwd"] + 2
    assert torch.isfinite(runs[0][0]).all() and torch.isfinite(runs[0][1]).all()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_attention_headsize_graph_replay_equals_eager():
    """forward + backward of one GroupQueryFlashAttention (head size 48, S = 257) captured once and replayed on refilled static
    inputs: output, dx and every weight gradient equal the eager step's bit for bit (test_attention_hd_graph_replay_equals_eager)"""
    import gaot_3d_amd
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd.model.layers.attn import GroupQueryFlashAttention
    d, s, b, h, hkv = 48, 257, 2, 4, 2
    hidden = h * d
    torch.manual_seed(5)
    att = GroupQueryFlashAttention(hidden, hidden, hidden_size=hidden, num_heads=h, num_kv_heads=hkv, atten_dropout=0.0,
                                   positional_embedding="rope").to(DEV).train()
    params = [prm for prm in att.parameters() if prm.requires_grad]
    xs = torch.randn(b, s, hidden, device=DEV).requires_grad_(True)
    ws = torch.randn(b, s, hidden, device=DEV)

    def step():
        xs.grad = None
        for prm in params:
            prm.grad = None
        out = att(xs, relative_positions=True)
        (out * ws).sum().backward()
        return out

    gaot_3d_amd.set_precision("bf16")
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        calls = GF.AttentionHdFn.calls["fwd"]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out_g = step()
        assert GF.AttentionHdFn.calls["fwd"] == calls + 1
        grads_g = [xs.grad] + [prm.grad for prm in params]
        for i in range(2):
            xn, wn = torch.randn(b, s, hidden, device=DEV), torch.randn(b, s, hidden, device=DEV)
            with torch.no_grad():
                xs.copy_(xn)
                ws.copy_(wn)
            graph.replay()
            torch.cuda.synchronize()
            got = [out_g.detach().clone()] + [g.clone() for g in grads_g]
            out_e = step()                                   # eagerly on the same (static) inputs; fresh gradient tensors
            torch.cuda.synchronize()
            want = [out_e.detach()] + [xs.grad] + [prm.grad for prm in params]
            assert all(torch.isfinite(t).all() for t in got)
            for j, (a, r) in enumerate(zip(got, want)):
                assert torch.equal(a, r), (i, j, float((a - r).abs().max()))
            xs.grad, grads = grads_g[0], grads_g[1:]         # the graph's own gradient tensors back in place for the next replay
            for prm, g in zip(params, grads):
                prm.grad = g
    finally:
        gaot_3d_amd.set_precision("fp32")


def _model_step(model, batch, tokens):
    from gaot_3d_amd import functional as GF
    model.zero_grad(set_to_none=True)
    pred = model(batch=batch, tokens_pos=tokens)
    loss = GF.mse_loss(pred, batch.x)
    loss.backward()
    torch.cuda.synchronize()
    return pred.detach(), loss.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def test_model_with_head_dim_48_bf16_against_fp32():
    """a small GAOT3D with hidden 96 / 2 heads (head size 48, the padded 64 instance): one training step in bf16 mode (flash kernels)
    against the same model in fp32 mode (the general path, pinned to the oracle by test_attention_any_head_dim_matches_oracle):
    prediction 2e-2 of the peak and relative L2 1e-2, loss rtol 1e-2, gradient cosine >= 0.999 overall.  The per-tensor cosines are
    printed, with no bar fixed in advance.

    Measured: the lowest two are processor.decoder_layers.0.attn.q_proj.weight 0.999472 and k_proj.weight 0.999629 (the same two
    tensors as at head size 64, for the reason given in test_model_with_head_dim_64_bf16_against_fp32); every other tensor is
    >= 0.99994, the overall cosine 0.999999."""
    import gaot_3d_amd
    import test_model_gpu as T
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd.data import make_synthetic_sample
    from gaot_3d_amd.model import init_model
    gaot_3d_amd.set_precision("fp32")
    torch.manual_seed(0)
    cfg = T.small_config(False, heads=2, head_dim=48, layers=2)
    model = init_model(6, 1, "gaot_3d", cfg).to(DEV).train()
    assert all(blk.attn.head_dim == 48 for blk in model.processor.encoder_layers)
    batch, tokens = make_synthetic_sample(3001, (8, 8, 4), k=4, seed=1, device=str(DEV))
    tokens = tokens.to(DEV)
    with torch.no_grad():
        p0 = model(batch=batch, tokens_pos=tokens)
    last = model.decoder.projection.fcs[-1]
    PAR.unit_scale_last_layer(last.weight, last.bias, float(p0.std()))
    calls = dict(GF.AttentionHdFn.calls)
    pred_r, loss_r, grads_r = _model_step(model, batch, tokens)
    assert GF.AttentionHdFn.calls == calls                      # fp32 mode: the general path, not the flash kernels
    gaot_3d_amd.clear_graph_cache(batch)
    gaot_3d_amd.set_precision("bf16")
    try:
        pred, loss, grads = _model_step(model, batch, tokens)
    finally:
        gaot_3d_amd.set_precision("fp32")
    assert GF.AttentionHdFn.calls["fwd"] == calls["fwd"] + 2 and GF.AttentionHdFn.calls["bwd"] == calls["bwd"] + 2   # 2 layers
    per = []
    for k in grads_r:
        if k in grads:
            x, y = grads[k].double().flatten(), grads_r[k].double().flatten()
            per.append((float(x @ y / (x.norm() * y.norm() + 1e-300)), k))
    for c, k in sorted(per):
        print(f"[parity] model_hs48_bf16/grads/{k}: cosine={c:.6f}")
    PAR.close_peak("model_hs48_bf16/pred", pred, pred_r, 2e-2, rel_l2=1e-2)
    PAR.close("model_hs48_bf16/loss", loss, loss_r, 1e-2, 0.0)
    PAR.grads_cosine("model_hs48_bf16/grads", grads, grads_r, 0.999)


def test_model_head_dim_48_dropout_seed_words_reserved_in_one_launch():
    """bf16 mode, head size 48, attention dropout 0.1: the Transformer counts its two blocks by hd_flash_eligible and reserves their
    seed words with one launch; the step equals the one in which every block draws its own word bit for bit, exactly two words of
    the stream are consumed, and the step has one launch fewer
    (test_model_head_dim_64_dropout_seed_words_reserved_in_one_launch)"""
    import gaot_3d_amd
    import test_model_gpu as T
    from gaot_3d_amd import functional as GF, ops
    from gaot_3d_amd.data import make_synthetic_sample
    from gaot_3d_amd.model import init_model
    from gaot_3d_amd.model.layers import attn as A
    torch.manual_seed(0)
    model = init_model(6, 1, "gaot_3d", T.small_config(False, heads=2, head_dim=48, layers=2, dropout=0.1)).to(DEV).train()
    batch, tokens = make_synthetic_sample(3001, (8, 8, 4), k=4, seed=1, device=str(DEV))
    tokens = tokens.to(DEV)
    seed0, runs, nxt, launches = 424242, [], [], []
    _model_step(model, batch, tokens)          # the per-sample caches (neighbour lists, statistics) are built once, here
    prev = A.SEED_BLOCK["on"]
    gaot_3d_amd.set_precision("bf16")
    try:
        for on in (True, False):
            A.SEED_BLOCK["on"] = on
            GF.set_dropout_seed(seed0, DEV)
            calls = GF.AttentionHdFn.calls["fwd"]
            ops.launch_count_reset()
            runs.append(_model_step(model, batch, tokens))
            launches.append(ops.launch_count())
            assert GF.AttentionHdFn.calls["fwd"] == calls + 2
            nxt.append(int(GF.next_dropout_seed(DEV).item()) & 0xFFFFFFFFFFFFFFFF)
    finally:
        A.SEED_BLOCK["on"] = prev
        gaot_3d_amd.set_precision("fp32")
    assert nxt[0] == nxt[1] == GF.dropout_seed_sequence(seed0, 3)[2]
    assert launches[0] == launches[1] - 1, launches
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert runs[0][2].keys() == runs[1][2].keys() and all(torch.equal(runs[0][2][k], runs[1][2][k]) for k in runs[0][2])


@pytest.mark.parametrize("d", [6, 132])
def test_attention_headsize_refusals(d):
    """head sizes outside the rule are refused by ops.attn_hd_fwd before any launch"""
    from gaot_3d_amd import ops
    b, s, h = 1, 8, 2
    qkv = torch.zeros(b * s, 3 * h * d, device=DEV)
    torch.cuda.synchronize()
    ops.launch_count_reset()
    n0 = ops.launch_count()
    with pytest.raises(ops.GaotError, match="head_dim must be a multiple of 4 with 4 <= head_dim <= 128"):
        ops.attn_hd_fwd(qkv, b, s, h, h, d, d ** -0.5)
    assert ops.launch_count() == n0
