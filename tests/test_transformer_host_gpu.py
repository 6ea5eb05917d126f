"""The host layer that drives the Transformer-block kernels (gaot_3d_amd/functional.py): the launches it issues, the life time of the
per-forward weight images, and what happens when a shape-only placeholder loses the image it carries.  bf16 mode; the smallest
Transformer that runs every fused Function: hidden 256, 8 heads / 4 kv heads of 32, FFN hidden 128, 128 tokens (two 64-row blocks),
three layers with the long-range skip -- an encoder block (NormQKVFn, its output tapped by the next block), a middle block (NormQKVFn
with the tap) and a decoder block (CatNormQKVFn) -- each ending in BlockTailFn, whose backward hands dO on as an image; dropout 0.1."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, S, D, HEADS, KV, F, P_DROP = 1, 128, 256, 8, 4, 128, 0.1

# kernel launches of the library (ops.launch_count) measured with this file's own _census() on the parent of the commit that
# introduced the image store -- dfa1dea "Flash attention kernels for head sizes 64 and 128 in bf16 mode" -- on an MI355X:
PARENT_STEP_LAUNCHES = 61       # one training step (forward, MSE, backward) of the three-layer Transformer, images prepared by Transformer.forward
PARENT_BLOCK_LAUNCHES = 31      # the same of its decoder block called on its own: every image is packed at its use


def _net():
    from gaot_3d_amd.model.layers.attn import AttentionConfig, FFNConfig, Transformer, TransformerConfig
    torch.manual_seed(7)
    cfg = TransformerConfig(patch_size=2, hidden_size=D, num_layers=3, positional_embedding="rope", use_long_range_skip=True,
                            attn_config=AttentionConfig(hidden_size=D, num_heads=HEADS, num_kv_heads=KV, atten_dropout=P_DROP),
                            ffn_config=FFNConfig(hidden_size=F))
    net = Transformer(D, D, cfg).to(DEV).train()
    g = torch.Generator(device="cpu").manual_seed(8)
    x, skip, tgt = (torch.randn(B, S, D, generator=g).to(DEV) for _ in range(3))
    return net, x, skip, tgt


@pytest.fixture(scope="module")
def setup():
    import gaot_3d_amd
    from gaot_3d_amd import ops
    prev = ops.defer_reductions(False)
    gaot_3d_amd.set_precision("bf16")
    try:
        yield _net()
    finally:
        gaot_3d_amd.set_precision("fp32")
        ops.defer_reductions(prev)


def _trainable(module):
    return [p for p in module.parameters() if p.requires_grad]


def _step(run, params, tgt, seed=1234):
    """one training step of ``run`` (input -> output) from dropout seed ``seed`` -> (loss, input gradient + parameter gradients, launches)"""
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd import ops
    GF.set_dropout_seed(seed, DEV)
    for p in params:
        p.grad = None
    ops.launch_count_reset()
    xin, out = run()
    loss = GF.mse_loss(out, tgt)
    loss.backward()
    n = ops.launch_count()
    torch.cuda.synchronize()
    return loss.detach().clone(), [xin.grad.clone()] + [p.grad.clone() for p in params], n


def _census(net, x, skip, tgt):
    """-> (launches of a Transformer step, launches of a step of its decoder block on its own); the second step of each is counted:
    the first also co-locates the weights and builds the RoPE tables"""
    def whole():
        xin = x.clone().requires_grad_(True)
        return xin, net(xin, relative_positions=True)

    def block():
        xin = x.clone().requires_grad_(True)
        return xin, net.decoder_layers[0](xin, relative_positions=True, skip=skip)

    counts = []
    for run, params in ((whole, _trainable(net)), (block, _trainable(net.decoder_layers[0]))):
        _step(run, params, tgt)
        counts.append(_step(run, params, tgt)[2])
    return tuple(counts)


def test_launch_census_and_image_life_time(setup):
    """the host layer issues the launches it issued before the image store replaced the six dicts, with the images prepared ahead
    (Transformer.forward) and on the miss path (a bare block); and no image outlives the forward that made it, raised or not"""
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd._lib import GaotError
    from gaot_3d_amd.model.layers.attn import FFNConfig, Transformer, TransformerConfig
    net, x, skip, tgt = setup
    step, block = _census(net, x, skip, tgt)
    print(f"[census] transformer step {step} launches (parent {PARENT_STEP_LAUNCHES}), bare decoder block {block} (parent {PARENT_BLOCK_LAUNCHES})")
    assert (step, block) == (PARENT_STEP_LAUNCHES, PARENT_BLOCK_LAUNCHES)
    net(x, relative_positions=True)
    assert len(GF._IMAGES) == 0
    # a forward that raises: the input projection's host-side width check refuses the input after the images were made
    cfg = TransformerConfig(patch_size=2, hidden_size=D, num_layers=1, ffn_config=FFNConfig(hidden_size=F))
    narrow = Transformer(64, D, cfg).to(DEV).train()
    with pytest.raises(GaotError):
        narrow(x[..., :32])
    assert len(GF._IMAGES) == 0
    torch.cuda.synchronize()


def _head(net, x):
    """the encoder block's head on x -> (q | k | v placeholder, residual alias, RoPE frequencies)"""
    from gaot_3d_amd import functional as GF
    blk = net.encoder_layers[0]
    a = blk.attn
    wts = (a.q_proj.weight, a.k_proj.weight, a.v_proj.weight)
    GF.colocate(wts)
    spec = (a.rotary_emb.freqs, B, S, HEADS, KV, 1.0 / (32 ** 0.5))
    assert GF.NormQKVFn.eligible(x, blk.attn_norm.weight, wts, spec)
    qkv, xres = GF.NormQKVFn.apply(x, blk.attn_norm.weight, blk.attn_norm.eps, False, spec, *wts)
    assert GF._payload(qkv, "_gaot_qkv_image") is not None
    return qkv, xres, a.rotary_emb.freqs


def test_lost_qkv_image_is_an_error_before_any_launch(setup):
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd import ops
    from gaot_3d_amd._lib import GaotError
    net, x, _skip, _tgt = setup
    qkv, _xres, freqs = _head(net, x.clone().requires_grad_(True))
    before = ops.launch_count()
    with pytest.raises(GaotError):
        GF.AttentionFn.apply(qkv.view_as(qkv), freqs, B, S, HEADS, KV, P_DROP, None)    # same one-element storage, no image
    assert ops.launch_count() == before
    torch.cuda.synchronize()


def test_lost_do_image_is_an_error_in_the_attention_backward(setup):
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd._lib import GaotError
    net, x, _skip, tgt = setup
    blk = net.encoder_layers[0]
    f = blk.ffn
    GF.colocate([f.w1.weight, f.w3.weight])
    qkv, xres, freqs = _head(net, x.clone().requires_grad_(True))
    o = GF.AttentionFn.apply(qkv, freqs, B, S, HEADS, KV, P_DROP, None)
    o.register_hook(lambda g: g.view_as(g))      # the engine now delivers another tensor object: the attribute is gone
    assert GF.BlockTailFn.eligible(xres.reshape(B * S, D), blk.attn.o_proj.weight, blk.ffn_norm.weight, f.w1.weight, f.w3.weight, f.w2.weight)
    y = GF.BlockTailFn.apply(o, xres.reshape(B * S, D), blk.attn.o_proj.weight, blk.ffn_norm.weight, blk.ffn_norm.eps, f.w1.weight,
                             f.w3.weight, f.w2.weight, (B, S, HEADS, KV))
    with pytest.raises(GaotError):
        GF.mse_loss(y, tgt.reshape(B * S, D)).backward()
    torch.cuda.synchronize()
    for p in net.parameters():
        p.grad = None


def test_step_is_deterministic(setup):
    """the same seed twice: the loss and every gradient bit for bit (what a comparison of two builds of this layer rests on)"""
    net, x, _skip, tgt = setup

    def whole():
        xin = x.clone().requires_grad_(True)
        return xin, net(xin, relative_positions=True)

    params = _trainable(net)
    loss_a, grads_a, _ = _step(whole, params, tgt)
    loss_b, grads_b, _ = _step(whole, params, tgt)
    assert torch.equal(loss_a, loss_b)
    assert len(grads_a) == len(grads_b) == 1 + len(params)
    for ga, gb in zip(grads_a, grads_b):
        assert torch.equal(ga, gb)
