"""Flash attention for head sizes 64 and 128 in bf16 mode (csrc/attn_hd.hip; reference attn.py:110-127 accepts every
hidden_size % num_heads == 0): against the fp64 oracle through GroupQueryFlashAttention, against the unfused general path, in
O(S) memory, under graph replay, and inside the whole model.
bf16 bars (tests/test_fullsize_oracle_gpu.py): output max|err| <= 2e-2 of the peak and relative L2 <= 1e-2; every
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


# every S, batch, (H, HKV), RoPE setting and p with each D (a pruned cross product)
_ORACLE_CASES = [
    (64, 5, 1, 2, 2, True, 0.0), (64, 33, 2, 4, 2, False, 0.1), (64, 77, 1, 4, 1, True, 0.1), (64, 130, 2, 2, 2, False, 0.0),
    (64, 257, 1, 4, 2, True, 0.1), (64, 2048 + 77, 1, 4, 1, False, 0.0),
    (128, 5, 2, 4, 1, False, 0.1), (128, 33, 1, 2, 2, True, 0.0), (128, 77, 2, 4, 2, False, 0.0), (128, 130, 1, 4, 1, True, 0.1),
    (128, 257, 2, 2, 2, False, 0.1), (128, 2048 + 77, 1, 4, 2, True, 0.1)]


@pytest.mark.parametrize("d,s,b,h,hkv,rope,p", _ORACLE_CASES)
def test_attention_hd_matches_fp64_oracle(d, s, b, h, hkv, rope, p):
    """GroupQueryFlashAttention with head size 64 / 128 in bf16 mode against the oracle's attention in fp64: forward, dx and the
    q / k / v / o projection weight gradients.  S below one tile, one past a tile, ragged last tiles on the key and the query side,
    and 2 125 (several key tiles per workgroup, several workgroups per head).  With dropout the mask the kernels regenerate is
    rebuilt from the seed word, equals the oracle's draw bit for bit and goes into the oracle's SDPA."""
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
    _bars(f"attn_hd{d}_S{s}_b{b}_h{h}kv{hkv}_rope{int(rope)}_p{p}", out, ref.detach(), grads)


def _qkv(d, s, b, h, hkv, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(b * s, (h + 2 * hkv) * d, generator=g)
    qkv[:, :(h + hkv) * d] *= 1.5          # |score| of O(2): a softmax with structure
    return qkv, torch.randn(b * s, h * d, generator=g)


@pytest.mark.parametrize("d,s,b,h,hkv,rope", [(64, 257, 2, 4, 2, True), (128, 130, 1, 4, 1, False)])
def test_attention_hd_matches_unfused_path(d, s, b, h, hkv, rope):
    """the same q | k | v through the flash kernels (bf16 mode) and through the unfused general path (fp32 arithmetic), p = 0"""
    import gaot_3d_amd
    from gaot_3d_amd import functional as GF
    qkv, w = _qkv(d, s, b, h, hkv, 7 + d)
    freqs = (1.0 / (10000 ** (torch.arange(0, d, 2).float() / d))).to(DEV) if rope else None
    xa, xb, wd = qkv.to(DEV).requires_grad_(True), qkv.to(DEV).requires_grad_(True), w.to(DEV)
    ref = GF._attention_unfused(xa, freqs, b, s, h, hkv, d)
    (ref * wd).sum().backward()
    gaot_3d_amd.set_precision("bf16")
    try:
        out = GF.attention_general(xb, freqs, b, s, h, hkv, d)
        (out * wd).sum().backward()
        torch.cuda.synchronize()
    finally:
        gaot_3d_amd.set_precision("fp32")
    cols = (("dq", 0, h * d), ("dk", h * d, (h + hkv) * d), ("dv", (h + hkv) * d, (h + 2 * hkv) * d))
    _bars(f"attn_hd{d}_vs_unfused_S{s}", out, ref.detach(), {nm: (xb.grad[:, lo:hi], xa.grad[:, lo:hi]) for nm, lo, hi in cols})


@pytest.mark.parametrize("d", [64, 128])
def test_attention_hd_head_slice_draws_the_global_heads_mask(d):
    """heads 2..3 of 4 (head0 = 2, heads_total = 4: a rank's slice of a head- / sequence-parallel step) draw the masks heads 2 and
    3 draw in the 4-head launch: outputs and gradients of the slice equal the 4-head run's bit for bit, and the 4-head mask's slice
    in the oracle's SDPA reproduces them"""
    from gaot_3d_amd import ops
    s, b, h, p = 77, 2, 4, 0.1
    qkv, w = _qkv(d, s, b, h, h, 11 + d)
    word = 0x9E3779B97F4A7C15 ^ d
    st = _seed_tensor(word)
    scale = d ** -0.5
    qd, wd = qkv.to(DEV), w.to(DEV)
    o4, lse4 = ops.attn_hd_fwd(qd, b, s, h, h, d, scale, p, st)
    g4 = ops.attn_hd_bwd(qd, o4, wd, lse4, b, s, h, h, d, scale, p, st)
    sl = torch.cat([qd[:, (j * h + 2) * d:(j * h + 4) * d] for j in range(3)], dim=1).contiguous()     # q, k, v of heads 2..3
    ws = wd[:, 2 * d:4 * d].contiguous()
    o2, lse2 = ops.attn_hd_fwd(sl, b, s, 2, 2, d, scale, p, st, head0=2, heads_total=4)
    g2 = ops.attn_hd_bwd(sl, o2, ws, lse2, b, s, 2, 2, d, scale, p, st, head0=2, heads_total=4)
    o2_unkeyed, _ = ops.attn_hd_fwd(sl, b, s, 2, 2, d, scale, p, st)
    torch.cuda.synchronize()
    assert torch.equal(o2, o4[:, 2 * d:4 * d])
    assert not torch.equal(o2_unkeyed, o2)                                 # (keyed by the local head it draws heads 0..1's masks)
    for j in range(3):
        assert torch.equal(g2[:, 2 * j * d:2 * (j + 1) * d], g4[:, (j * h + 2) * d:(j * h + 4) * d]), j
    keep = ops.attn_dropout_mask(st, p, b, h, s).cpu().bool()
    assert torch.equal(keep, orc.dropout_keep_mask(word, b, h, s, p))
    x = sl.cpu().double().requires_grad_(True)
    q, k, v = (x[:, 2 * j * d:2 * (j + 1) * d].reshape(b, s, 2, d).transpose(1, 2) for j in range(3))
    ref = orc.sdpa(q, k, v, keep[:, 2:4], orc.dropout_threshold(p) / 65536.0).transpose(1, 2).reshape(b * s, 2 * d)
    (ref * ws.cpu().double()).sum().backward()
    _bars(f"attn_hd{d}_heads2to3of4_p{p}", o2, ref.detach(),
          {nm: (g2[:, 2 * j * d:2 * (j + 1) * d], x.grad[:, 2 * j * d:2 * (j + 1) * d]) for j, nm in enumerate(("dq", "dk", "dv"))})


def test_attention_hd_never_holds_an_s_by_s_tensor():
    """S = 16 384, head size 64, forward + backward: one fp32 score matrix alone is 1 GiB (the unfused path keeps one per head),
    the O(S * D) buffers of this call are below 100 MiB.  Two runs with the same seed are bit-identical (no float atomics)."""
    import gaot_3d_amd
    from gaot_3d_amd import functional as GF
    d, s, b, h, hkv, p = 64, 16384, 1, 2, 1, 0.1
    qkv, w = _qkv(d, s, b, h, hkv, 3)
    freqs = (1.0 / (10000 ** (torch.arange(0, d, 2).float() / d))).to(DEV)
    wd = w.to(DEV)
    x = qkv.to(DEV).requires_grad_(True)
    runs = []
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
            print(f"[memory] attn_hd64_S{s} run {i}: peak above the inputs {extra / 2 ** 20:.1f} MiB")
            assert extra <= 256 * 2 ** 20, f"{extra / 2 ** 20:.1f} MiB allocated above the inputs: an S x S tensor?"
            runs.append((o.detach().clone(), x.grad.clone()))
    finally:
        gaot_3d_amd.set_precision("fp32")
    assert torch.isfinite(runs[0][0]).all() and torch.isfinite(runs[0][1]).all()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_attention_hd_graph_replay_equals_eager():
    """forward + backward of one GroupQueryFlashAttention (head size 64, S = 257) captured once and replayed on refilled static
    inputs: output, dx and every weight gradient equal the eager step's bit for bit"""
    import gaot_3d_amd
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd.model.layers.attn import GroupQueryFlashAttention
    d, s, b, h, hkv = 64, 257, 2, 4, 2
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


def test_model_with_head_dim_64_bf16_against_fp32():
    """a small GAOT3D with hidden 128 / 2 heads (head size 64): one training step in bf16 mode (flash kernels) against the same
    model in fp32 mode (the general path, pinned to the oracle by test_attention_any_head_dim_matches_oracle); the bf16 bars of
    tests/test_model_gpu.py::test_cfg0_vs_oracle, unchanged: prediction 2e-2 of the peak and relative L2 1e-2, loss rtol 1e-2,
    gradient cosine >= 0.999 overall and >= 0.9994 for every tensor with no energy filter.

    The tensors nearest the per-tensor bar are processor.decoder_layers.0.attn.q_proj.weight / k_proj.weight (measured 0.999741 /
    0.999633; every other tensor >= 0.99995): in this untrained model the softmax is nearly uniform and keys and values share a
    large common component, which sum_k dS = 0 cancels.  It cancels in the kernels too because delta = rowsum(dO . O) is formed
    from the bf16-rounded dO the matrix cores see (with the unrounded dO these two tensors reach 0.9986 / 0.9982)."""
    import gaot_3d_amd
    import test_model_gpu as T
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd.data import make_synthetic_sample
    from gaot_3d_amd.model import init_model
    gaot_3d_amd.set_precision("fp32")
    torch.manual_seed(0)
    cfg = T.small_config(False, heads=2, head_dim=64, layers=2, latent=(8, 8, 4), dropout=0.0)
    model = init_model(6, 1, "gaot_3d", cfg).to(DEV).train()
    assert all(blk.attn.head_dim == 64 for blk in model.processor.encoder_layers)
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
    PAR.close_peak("model_hd64_bf16/pred", pred, pred_r, 2e-2, rel_l2=1e-2)
    PAR.close("model_hd64_bf16/loss", loss, loss_r, 1e-2, 0.0)
    PAR.grads_cosine("model_hd64_bf16/grads", grads, grads_r, 0.999, per_tensor=0.9994, energy=0.0)


def test_model_head_dim_64_dropout_seed_words_reserved_in_one_launch():
    """bf16 mode, head size 64, attention dropout 0.1: the Transformer reserves the seed words of its two blocks with one launch
    (they count in ``n_drop`` like head-size-32 blocks); the step equals the one in which every block draws its own word bit for
    bit, exactly two words of the stream are consumed, and the step has one launch fewer (one block of two words instead of two
    single words)"""
    import gaot_3d_amd
    import test_model_gpu as T
    from gaot_3d_amd import functional as GF, ops
    from gaot_3d_amd.data import make_synthetic_sample
    from gaot_3d_amd.model import init_model
    from gaot_3d_amd.model.layers import attn as A
    torch.manual_seed(0)
    model = init_model(6, 1, "gaot_3d", T.small_config(False, heads=2, head_dim=64, dropout=0.1)).to(DEV).train()
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


def test_point_shard_head_dim_64_bf16_one_gpu(tmp_path):
    """two ranks on one GPU, head-parallel, head size 64 in bf16 mode against the unsharded bf16 step: each rank runs the flash
    kernels on its head behind the existing exchanges; the assertions of test_point_shard_other_variants_one_gpu"""
    import gaot_3d_amd
    import test_model_gpu as T
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd.data import make_synthetic_sample
    from gaot_3d_amd.model import init_model
    gaot_3d_amd.set_precision("bf16")
    try:
        torch.manual_seed(0)
        model = init_model(6, 1, "gaot_3d", T.small_config(False, 2, head_dim=64)).to(DEV).train()
        batch, tokens = make_synthetic_sample(3001, (8, 8, 4), k=4, seed=1, device=str(DEV))
        calls = GF.AttentionHdFn.calls["fwd"]
        loss = GF.mse_loss(model(batch=batch, tokens_pos=tokens.to(DEV)), batch.x)
        loss.backward()
        torch.cuda.synchronize()
        assert GF.AttentionHdFn.calls["fwd"] == calls + 2
    finally:
        gaot_3d_amd.set_precision("fp32")
    got = T._run_shard_workers(tmp_path, 2, 29597, GAOT_TEST_PARALLEL="head", GAOT_TEST_HEADS=2, GAOT_TEST_HEADDIM=64,
                               GAOT_TEST_PREC="bf16", GAOT_TEST_EMBED="statistical", GAOT_TEST_DEC_GEO="0")
    print(f"[parity] shard2_head_hd64_bf16/loss: {got['loss']:.8f} vs {float(loss.detach()):.8f}")
    assert abs(got["loss"] - float(loss.detach())) <= 1e-5 * abs(float(loss.detach())) + 1e-8
    n = 0
    for k, p in model.named_parameters():
        if p.grad is None:
            continue
        ref = p.grad.detach().cpu().double()
        assert k in got["norms"], k
        assert abs(got["norms"][k] - float(ref.norm())) <= 1e-3 * float(ref.norm()) + 1e-6, (k, got["norms"][k], float(ref.norm()))
        head = torch.tensor(got["grads"][k], dtype=torch.float64)
        assert torch.allclose(head, ref.flatten()[:64], rtol=1e-3, atol=1e-5 * max(1.0, float(ref.abs().max()))), k
        n += 1
    assert n > 20
