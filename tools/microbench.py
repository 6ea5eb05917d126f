#!/usr/bin/env python3
"""Kernel microbenchmarks at the configs[1] shapes (for rocprofv3 / quick A-B): attention fwd+bwd, GEMM shapes, GNO, PointNet GeoEmbed,
the attention-weighted GNO, the forward-only decoder (decoder_sample), the sampled field's Jacobian (decoder_jacobian), the projection MLP's tangent alone (projection_jvp), the sampled field's Hessian and Laplacian (decoder_hessian), its derivatives along per-query directions (decoder_directional), its adjoint with respect to the latent (decoder_adjoint), the adjoint of its Jacobian (decoder_jacobian_adjoint), the adjoint of its Laplacian (decoder_laplacian_adjoint), the adjoints of its directional derivatives and of its Hessian (decoder_directional_adjoint, decoder_hessian_adjoint), the projection MLP's exact-fp32 backward alone (projection_bwd_f32), the streamed gradients of the latent and the decoder's parameters (decoder_param_adjoint)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.environ.get("MB_TREE"):      # measure another checkout's package (gno_weighted: the parent commit's) with this script
    sys.path.insert(0, os.environ["MB_TREE"])
import torch
import gaot_3d_amd
from gaot_3d_amd import ops, functional as GF

what = sys.argv[1] if len(sys.argv) > 1 else "attn"
reps = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else 5
dev = "cuda:0"
gaot_3d_amd.set_precision(os.environ.get("GAOT_PRECISION", "bf16"))
torch.manual_seed(0)


def timeit(fn, name, flops=None):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps): fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    print(f"{name}: {dt*1e3:.3f} ms" + (f"  {flops/dt/1e12:.1f} TF/s" if flops else ""))


if what == "attn":
    b, s, h = 1, int(os.environ.get('MB_S', 16384)), int(os.environ.get('MB_H', 8))
    qkv = torch.randn(b * s, 3 * h * 32, device=dev)
    freqs = (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32))).to(dev)
    d_o = torch.randn(b * s, h * 32, device=dev)
    att = 2 * s * s * 32 * h
    pd = float(os.environ.get("MB_DROP", 0.0))     # attention dropout probability
    sd = torch.tensor([12345], dtype=torch.int64, device=dev) if pd > 0 else None
    fused = {"0": False, "1": True}.get(os.environ.get("MB_FUSED"))     # None: the library's choice
    if ops.get_precision() == "bf16":
        o, lse, img = ops.attn_fwd_bf16(qkv, freqs, b, s, h, h, 32 ** -0.5, pd, sd)
        timeit(lambda: ops.attn_fwd_bf16(qkv, freqs, b, s, h, h, 32 ** -0.5, pd, sd), "attn_fwd_bf16(+prep)", 2 * att)
        timeit(lambda: ops.attn_bwd_bf16(img, o, d_o, lse, b, s, h, h, 32 ** -0.5, pd, sd, fused=fused), "attn_bwd_bf16(all)", 4 * att)
        ops.timing_reset(True)
        for _ in range(reps):
            ops.attn_fwd_bf16(qkv, freqs, b, s, h, h, 32 ** -0.5, pd, sd)
            ops.attn_bwd_bf16(img, o, d_o, lse, b, s, h, h, 32 ** -0.5, pd, sd, fused=fused)
        torch.cuda.synchronize()
        for name, (calls, tot) in ops.timing_summary().items():
            print(f"  {name}: {tot / calls:.4f} ms")
        ops.timing_reset(False)
    else:
        o, lse = ops.attn_fwd(qkv, b, s, h, h, 32 ** -0.5)
        timeit(lambda: ops.attn_fwd(qkv, b, s, h, h, 32 ** -0.5), "attn_fwd_f32", 2 * att)
        timeit(lambda: ops.attn_bwd(qkv, o, d_o, lse, b, s, h, h, 32 ** -0.5), "attn_bwd_f32", 4 * att)
elif what == "gemm":
    m = 16384
    for (n, k) in ((768, 256), (256, 256), (2048, 256), (256, 1024), (256, 512)):
        x = torch.randn(m, k, device=dev); w = torch.randn(n, k, device=dev); dy = torch.randn(m, n, device=dev)
        fl = 2 * m * n * k
        timeit(lambda: ops.gemm(x, w, m, n, k, k, k, False, True), f"fwd  x[{m},{k}] W[{n},{k}]^T", fl)
        timeit(lambda: ops.gemm(dy, w, m, k, n, n, k, False, False), f"dx   dy[{m},{n}] W[{n},{k}]", fl)
        timeit(lambda: ops.gemm(dy, x, n, k, m, n, k, True, False), f"dW   dy^T[{n},{m}] x[{m},{k}]", fl)
        wb = w.bfloat16()
        timeit(lambda: ops.gemm(x, wb, m, n, k, k, k, False, True), f"fwd  (bf16 W)", fl)
        timeit(lambda: ops.gemm(dy, wb, m, k, n, n, k, False, False), f"dx   (bf16 W)", fl)
        timeit(lambda: ops.gemm(x, wb, m, n, k, k, k, False, True, out_dtype=torch.bfloat16), f"fwd  (bf16 W, bf16 C)", fl)
        xb = x.bfloat16()
        timeit(lambda: ops.gemm(xb, wb, m, n, k, k, k, False, True), f"fwd  (bf16 x, bf16 W)", fl)
        mb = (m * k + m * n + n * k) * 4 / 1e6
        print(f"     (operand + result bytes {mb:.0f} MB -> {mb / 5e3 * 1e3:.1f} us at 5 TB/s)")
elif what == "gemm16":
    # the bf16-in-memory GEMMs of one block at configs[1] (A and B bf16): dx of w1|w3, w2 forward
    m = 16384
    for (n, k, bt, name) in ((256, 2048, False, "dx_w13  dag[16384,2048] W13[2048,256]"), (256, 1024, True, "w2 fwd  u[16384,1024] W2[256,1024]^T")):
        a = torch.randn(m, k, device=dev).bfloat16()
        w = (torch.randn(n, k, device=dev) if bt else torch.randn(k, n, device=dev)).bfloat16()
        fl = 2 * m * n * k
        timeit(lambda: ops.gemm(a, w, m, n, k, k, w.shape[1], False, bt), name, fl)
elif what == "wgrad":
    # weight gradients of one block at configs[1]: dW = dy^T x over 16384 tokens, both operands bf16 in memory.  MB_SETS > 1
    # rotates through that many operand sets (6 x 75 MB do not fit the 256-MB Infinity Cache: operands come from HBM, as in the step)
    rows = 16384
    nsets = int(os.environ.get("MB_SETS", 1))
    for (m, n, name) in ((2048, 256, "w1|w3"), (256, 1024, "w2"), (768, 256, "q|k|v"), (256, 256, "o_proj"), (256, 512, "skip_proj")):
        sets = [((torch.randn(rows, m, device=dev) * 0.5).bfloat16(), (torch.randn(rows, n, device=dev) * 0.5).bfloat16()) for _ in range(nsets)]
        a, b = sets[0]
        c = ops.gemm(a, b, m, n, rows, m, n, True, False)
        ref = a.float().t() @ b.float()
        err = (c - ref).abs().max().item() / ref.abs().max().item()
        it = [0]
        def run():
            x, y = sets[it[0] % nsets]
            it[0] += 1
            return ops.gemm(x, y, m, n, rows, m, n, True, False)
        timeit(run, f"dW {name:9s} [{m} x {n}] rel err {err:.1e}", 2 * rows * m * n)
elif what == "graph":
    # device graph construction at configs[1]: 500 000 surface points against the 64x64x32 token grid
    from gaot_3d_amd import graph
    from gaot_3d_amd.data import make_synthetic_sample
    batch, tokens = make_synthetic_sample(500000, (64, 64, 32), k=8, seed=0, device=dev)
    tokens = tokens.to(dev)
    pos = batch.pos
    g = graph.as_latent_grid(tokens, (64, 64, 32))
    timeit(lambda: graph.knn_to_grid(pos, g, 8), "knn_to_grid k=8 (E = 4.0 M)")
    timeit(lambda: graph.knn_to_grid(pos, g, 1), "knn_to_grid k=1")
    for r in (0.033, 0.05):
        e = graph._decoder_edges("radius", pos, g, r, 1)
        timeit(lambda: graph._decoder_edges("radius", pos, g, r, 1), f"radius r={r} centres=phys (E = {e.shape[1]})")
        e = graph._encoder_edges("radius", pos, g, r, 1)
        timeit(lambda: graph._encoder_edges("radius", pos, g, r, 1), f"radius r={r} centres=latent, cap 32 per token (E = {e.shape[1]})")
        e = graph._encoder_edges("bidirectional", pos, g, r, 1)
        timeit(lambda: graph._encoder_edges("bidirectional", pos, g, r, 1), f"bidirectional k=1 r={r} encoder (E = {e.shape[1]})")
elif what == "gno":
    from gaot_3d_amd.data import make_synthetic_sample
    batch, tokens = make_synthetic_sample(500000, (64, 64, 32), k=8, seed=0, device=dev)
    n, m = 500000, tokens.shape[0]
    tokens = tokens.to(dev)
    for nh, ei, ns, nd, yp, xp in ((3, batch.encoder_edge_index_s0, n, m, batch.pos, tokens),
                                   (2, batch.decoder_edge_index_s0, m, n, tokens, batch.pos),
                                   (4, batch.encoder_edge_index_s0, n, m, batch.pos, tokens)):
        ws = [torch.randn(64, 6, device=dev) * 0.3] + [torch.randn(64, 64, device=dev) * 0.1 for _ in range(nh - 1)] + [torch.randn(32, 64, device=dev) * 0.1]
        bs = [torch.zeros(w.shape[0], device=dev) for w in ws]
        timeit(lambda: ops.build_graph(ei, ns, nd), f"csr x2 (E={ei.shape[1]})")
        g = ops.build_graph(ei, ns, nd)
        f = torch.randn(ns, 32, device=dev); go = torch.randn(nd, 32, device=dev)
        e = ei.shape[1]
        fl = e * {2: 13088, 3: 21280, 4: 29472}[nh]
        timeit(lambda: ops.gno_forward(ws, bs, yp, xp, f, g), f"gno_fwd nh={nh}", fl)
        timeit(lambda: ops.gno_backward(ws, bs, yp, xp, f, go, g), f"gno_bwd nh={nh}", 3 * fl)
elif what == "coordgrad":
    # cost of the gradients with respect to the coordinates at configs[1] (500K points, 64x64x32 tokens, knn k=8): the GNO
    # backward with / without them (both precisions), the statistical GeoEmbed forward + backward, and a whole training step
    # (forward + MSE + backward) with / without batch.pos.requires_grad_()
    from gaot_3d_amd.data import make_synthetic_sample
    from gaot_3d_amd.model.layers.geoembed import GeoStatFn
    batch, tokens = make_synthetic_sample(500000, (64, 64, 32), k=8, seed=0, device=dev)
    n, m = 500000, tokens.shape[0]
    tokens = tokens.to(dev)
    for prec in ("fp32", "bf16"):
        gaot_3d_amd.set_precision(prec)
        for nh, ei, ns, nd, yp, xp in ((3, batch.encoder_edge_index_s0, n, m, batch.pos, tokens),
                                       (2, batch.decoder_edge_index_s0, m, n, tokens, batch.pos)):
            ws = [torch.randn(64, 6, device=dev) * 0.3] + [torch.randn(64, 64, device=dev) * 0.1 for _ in range(nh - 1)] + [torch.randn(32, 64, device=dev) * 0.1]
            bs = [torch.zeros(w.shape[0], device=dev) for w in ws]
            g = ops.build_graph(ei, ns, nd)
            f = torch.randn(ns, 32, device=dev); go = torch.randn(nd, 32, device=dev)
            timeit(lambda: ops.gno_backward(ws, bs, yp, xp, f, go, g), f"{prec} gno_bwd nh={nh} (E={ei.shape[1]})")
            timeit(lambda: ops.gno_backward(ws, bs, yp, xp, f, go, g, coords=True), f"{prec} gno_bwd nh={nh} + coordinate grads (kernel + 2 segment sums)")
            ops.timing_reset(True)
            for _ in range(reps):
                ops.gno_backward(ws, bs, yp, xp, f, go, g)
                ops.gno_backward(ws, bs, yp, xp, f, go, g, coords=True)
            torch.cuda.synchronize()
            for name, (calls, tot) in ops.timing_summary().items():
                print(f"  {name}: {tot / calls:.4f} ms")
            ops.timing_reset(False)
    gaot_3d_amd.set_precision("fp32")
    g = ops.build_graph(batch.encoder_edge_index_s0, n, m)
    timeit(lambda: ops.geoembed_moments(batch.pos, tokens, g), "geoembed moments sweep (forward)")
    timeit(lambda: ops.geoembed_from_moments(ops.geoembed_moments(batch.pos, tokens, g)), "geoembed forward (moments + finish)")
    mom = ops.geoembed_moments(batch.pos, tokens, g)
    gf = torch.randn(m, 9, device=dev)
    timeit(lambda: ops.geoembed_from_moments_bwd(mom, gf), "geoembed from_moments_bwd")
    adj = ops.geoembed_from_moments_bwd(mom, gf)
    timeit(lambda: ops.geoembed_moments_bwd(batch.pos, tokens, g, adj), "geoembed moments_bwd sweep")
    sp = batch.pos.clone().requires_grad_()
    timeit(lambda: torch.autograd.grad((GeoStatFn.apply(sp, tokens, g) * gf).sum(), [sp]),
           "geoembed forward + backward (autograd, incl. the source-side segment sum)")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from gaot_3d_amd.model import init_model
    for prec in ("bf16", "fp32"):
        gaot_3d_amd.set_precision(prec)
        model = init_model(6, 1, "gaot_3d", bench.model_config((64, 64, 32), 10, 8, 0.0)).to(dev).train()
        pos0 = batch.pos.detach()
        for want in (False, True):
            # the same tensor on every step (the per-sample caches see one sample): pos0 itself, or one leaf that requires grad
            batch.pos = pos0.clone().requires_grad_() if want else pos0

            def step():
                model.zero_grad(set_to_none=True)
                GF.mse_loss(model(batch=batch, tokens_pos=tokens), batch.x).backward()
            timeit(step, f"{prec} train step fwd+bwd, batch.pos.requires_grad={want}")
        batch.pos = pos0
        del model
elif what == "gno_nonlinear":
    # transform_type 'nonlinear' / 'nonlinear_kernelonly' at the configs[1] graph (500K points, 64x64x32 tokens, knn k=8: E = 4 M; encoder
    # direction with NH = 3, decoder direction with NH = 2), both precision modes: forward and backward of the module on (1) the fused
    # linear transform, (2) the fused kernels of the type, per-node products (t = W_0f f_y, dW_0f, dt W_0f) included, (3) the general
    # per-edge path of the type (MB_GENERAL=0 leaves it out).  HIP events around the forward and around the backward, median of `reps`
    # after one warm-up; the module's own kernels per call follow.  Output kept in profiles/gno_nonlinear_microbench.txt.
    from gaot_3d_amd.data import make_synthetic_sample
    from gaot_3d_amd.model.layers.integral_transform import IntegralTransform
    batch, tokens = make_synthetic_sample(500000, (64, 64, 32), k=8, seed=0, device=dev)
    n, m = 500000, tokens.shape[0]
    tokens = tokens.to(dev)
    general = os.environ.get("MB_GENERAL", "1") != "0"

    def fwd_bwd_ms(it, yp, xp, f, g, go):
        def once():
            for p in it.parameters():
                p.grad = None
            f.grad = None
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record(); out = it(yp, xp, None, f_y=f, graph=g); e1.record(); out.backward(go); e2.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), e1.elapsed_time(e2)
        once()
        ts = sorted(once() for _ in range(reps))
        fw = sorted(t[0] for t in ts)[len(ts) // 2]
        bw = sorted(t[1] for t in ts)[len(ts) // 2]
        return fw, bw

    for prec in ("fp32", "bf16"):
        gaot_3d_amd.set_precision(prec)
        for nh, ei, ns, nd, yp, xp in ((3, batch.encoder_edge_index_s0, n, m, batch.pos, tokens),
                                       (2, batch.decoder_edge_index_s0, m, n, tokens, batch.pos)):
            g = ops.build_graph(ei, ns, nd)
            f = torch.randn(ns, 32, device=dev).requires_grad_(); go = torch.randn(nd, 32, device=dev)
            torch.manual_seed(1)
            lin = IntegralTransform(channel_mlp_layers=[6] + [64] * nh + [32], transform_type="linear").to(dev)
            lf, lb = fwd_bwd_ms(lin, yp, xp, f, g, go)
            print(f"{prec} nh={nh} E={ei.shape[1]} linear (fused): fwd {lf:.3f} ms  bwd {lb:.3f} ms  fwd+bwd {lf + lb:.3f} ms")
            for tt in ("nonlinear", "nonlinear_kernelonly"):
                it = IntegralTransform(channel_mlp_layers=[6 + 32] + [64] * nh + [32], transform_type=tt).to(dev)
                ff, fb = fwd_bwd_ms(it, yp, xp, f, g, go)
                line = (f"{prec} nh={nh} {tt} (fused + per-node products): fwd {ff:.3f} ms  bwd {fb:.3f} ms  fwd+bwd {ff + fb:.3f} ms"
                        f"  = {(ff + fb) / (lf + lb):.2f} x linear (fwd {ff / lf:.2f} x, bwd {fb / lb:.2f} x)")
                if general:
                    plan = it._fused_plan
                    it._fused_plan = lambda *a, **k: None
                    gf_, gb_ = fwd_bwd_ms(it, yp, xp, f, g, go)
                    it._fused_plan = plan
                    line += f";  general path: fwd {gf_:.3f} ms  bwd {gb_:.3f} ms  fwd+bwd {gf_ + gb_:.3f} ms  = {(gf_ + gb_) / (lf + lb):.1f} x linear"
                print(line)
                ops.timing_reset(True)
                for _ in range(reps):
                    f.grad = None
                    it(yp, xp, None, f_y=f, graph=g).backward(go)
                torch.cuda.synchronize()
                for name, (calls, tot) in ops.timing_summary().items():
                    print(f"    {name}: {tot / calls:.4f} ms")
                ops.timing_reset(False)
                del it
elif what == "pointnet":
    # GeometricEmbedding(3, 32, "pointnet") on the two configs[1] graphs (500K points, 64x64x32 tokens, knn k=8): encoder side
    # (Q = 131 072 tokens) and decoder side (Q = 500 000 points, E = 4 M), max and mean pooling, no coordinate gradients: forward, and
    # forward + backward, HIP events, median (min, max) of `reps` after one warm-up; peak memory = the growth of
    # torch.cuda.max_memory_allocated over one forward + backward; then the library's own timed calls of a forward + backward.  Output kept in profiles/pointnet_microbench.txt.
    from gaot_3d_amd.data import make_synthetic_sample
    from gaot_3d_amd.model.layers.geoembed import GeometricEmbedding
    batch, tokens = make_synthetic_sample(500000, (64, 64, 32), k=8, seed=0, device=dev)
    n, m = 500000, tokens.shape[0]
    tokens = tokens.to(dev)

    def median_ms(fn):
        fn(); torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        return f"{ts[len(ts) // 2]:.3f} ms (min {ts[0]:.3f}, max {ts[-1]:.3f})"

    for side, ei, ns, nd, sp, qp in (("encoder", batch.encoder_edge_index_s0, n, m, batch.pos, tokens),
                                     ("decoder", batch.decoder_edge_index_s0, m, n, tokens, batch.pos)):
        g = ops.build_graph(ei, ns, nd)
        go = torch.randn(nd, 32, device=dev)
        for pooling in ("max", "mean"):
            torch.manual_seed(1)
            ge = GeometricEmbedding(3, 32, method="pointnet", pooling=pooling).to(dev)

            def fwd():
                with torch.no_grad():
                    return ge(sp, qp, ei, graph=g)

            def fwd_bwd():
                for p in ge.parameters():
                    p.grad = None
                ge(sp, qp, ei, graph=g).backward(go)
            tf, tb = median_ms(fwd), median_ms(fwd_bwd)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fwd_bwd()
            torch.cuda.synchronize()
            peak = (torch.cuda.max_memory_allocated() - base) / 1e6
            print(f"pointnet {side} Q={nd} E={ei.shape[1]} {pooling}: fwd {tf}  fwd+bwd {tb}  peak memory of fwd+bwd {peak:.1f} MB")
            ops.timing_reset(True)
            for _ in range(reps):
                fwd_bwd()
            torch.cuda.synchronize()
            print("    " + "  ".join(f"{name}: {tot / calls:.4f} ms" for name, (calls, tot) in sorted(ops.timing_summary().items())))
            ops.timing_reset(False)
elif what == "attn_headdim":
    # head sizes 64 and 128 in bf16 mode at hidden 256, S = 16 384, b = 1, RoPE on, p = 0.1: forward + backward of (1) the unfused
    # general path (functional._attention_unfused: the path every head size other than 32 took before the flash kernels), (2) the
    # flash kernels of csrc/attn_hd.hip (functional.attention_general), and, FOR ORIENTATION ONLY -- hand-scheduled kernels, not a
    # target -- (3) the head-size-32 kernels at the same hidden size (hidden / 32 heads, equal FLOPs).  HIP events around each call, median
    # of `reps` after one warm-up, the three alternating in one process.
    # MB_DIMS (comma-separated head sizes, default 64,128) and MB_HIDDEN (default 256; a multiple of every head size and of 32):
    # any head size hd_flash_eligible accepts, e.g. MB_DIMS=16 MB_HIDDEN=256, MB_DIMS=48,96 MB_HIDDEN=384.
    gaot_3d_amd.set_precision("bf16")
    s, hidden, pd = int(os.environ.get("MB_S", 16384)), int(os.environ.get("MB_HIDDEN", 256)), 0.1
    dims = tuple(int(t) for t in os.environ.get("MB_DIMS", "64,128").split(","))
    eligible = getattr(GF, "hd_flash_eligible", lambda d: d in GF.HD_FLASH_HEAD_DIMS)     # (MB_TREE: a checkout from before the predicate)
    assert hidden % 32 == 0 and all(hidden % d == 0 and eligible(d) for d in dims), (hidden, dims)
    h32 = hidden // 32
    GF.set_dropout_seed(2026, dev)

    def fwd_bwd(path, qkv, freqs, h, d, w):
        qkv.grad = None
        if path == "unfused":
            o = GF._attention_unfused(qkv, freqs, 1, s, h, h, d, pd)
        elif path == "flash":
            o = GF.attention_general(qkv, freqs, 1, s, h, h, d, pd)
        else:
            o = GF.AttentionFn.apply(qkv, freqs, 1, s, h, h, pd)
        (o * w).sum().backward()

    def median_ms(fn):
        fn(); torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        return ts[len(ts) // 2], ts[0], ts[-1]

    w = torch.randn(s, hidden, device=dev)
    x32 = torch.randn(s, 3 * hidden, device=dev).requires_grad_(True)
    f32_ = (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32))).to(dev)
    for d in dims:
        h = hidden // d
        qkv = torch.randn(s, 3 * hidden, device=dev).requires_grad_(True)
        freqs = (1.0 / (10000 ** (torch.arange(0, d, 2).float() / d))).to(dev)
        flops = 18 * s * s * d * h          # forward 4, dK/dV 8, dQ 6 S^2 D per head
        res = {}
        for name, fn in (("unfused", lambda: fwd_bwd("unfused", qkv, freqs, h, d, w)),
                         ("flash", lambda: fwd_bwd("flash", qkv, freqs, h, d, w)),
                         ("hd32", lambda: fwd_bwd("hd32", x32, f32_, h32, 32, w))):
            res[name] = median_ms(fn)
        print(f"D={d} h={h} S={s} p={pd} rope: (1) _attention_unfused fwd+bwd: {res['unfused'][0]:.3f} ms (min {res['unfused'][1]:.3f}, max {res['unfused'][2]:.3f})")
        print(f"D={d} h={h} S={s} p={pd} rope: (2) flash kernels (attn_hd) fwd+bwd: {res['flash'][0]:.3f} ms (min {res['flash'][1]:.3f}, max {res['flash'][2]:.3f})"
              f"  = {res['flash'][0] / res['unfused'][0]:.3f} x (1);  {flops / res['flash'][0] / 1e9:.1f} TF/s of 18 S^2 D h, "
              f"{100 * flops / res['flash'][0] / 1e9 / 2500:.1f} % of the 2.5 PF/s bf16 roof (whole call incl. RoPE and the loss product)")
        print(f"D={d}: (3) orientation only, head size 32 x {h32} heads (hand-scheduled kernels): {res['hd32'][0]:.3f} ms (min {res['hd32'][1]:.3f}, max {res['hd32'][2]:.3f})")
    ops.timing_reset(True)
    for d in dims:
        h = hidden // d
        qkv = torch.randn(s, 3 * hidden, device=dev).requires_grad_(True)
        freqs = (1.0 / (10000 ** (torch.arange(0, d, 2).float() / d))).to(dev)
        ops.TIMING["events"] = {}
        for _ in range(reps):
            fwd_bwd("flash", qkv, freqs, h, d, w)
        torch.cuda.synchronize()
        for name, (calls, tot) in ops.timing_summary().items():
            if name.startswith("attn_hd"):
                print(f"  D={d} {name}: {tot / calls:.4f} ms")
    ops.timing_reset(False)
elif what == "gno_weighted":
    # IntegralTransform with use_attn=True on the two configs[1] graphs (500K points, 64x64x32 tokens, knn k=8: E = 4 M; encoder
    # direction NH = 3, decoder direction NH = 2): forward + backward of the module, {cosine, dot_product} x three transform types x
    # {fp32, bf16}, graph and maps built before timing, HIP events, one warm-up, median of `reps`.  Legs: (a) this tree (the weighted
    # fused kernels), (b) the checkout named by MB_PARENT -- its use_attn module (the general per-edge path) and its UNWEIGHTED fused
    # transform of the same type.  MB_ROUNDS (default 5) rounds alternate one fresh child process per leg; a row is the median over
    # the rounds, the spread (max - min) / median over the rounds.  Output kept in profiles/gno_weighted_microbench.txt.
    import json
    import subprocess
    if os.environ.get("MB_CHILD") != "1":
        rounds = int(os.environ.get("MB_ROUNDS", 5))
        trees = [("new", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))]
        if os.environ.get("MB_PARENT"):
            trees.insert(0, ("parent", os.path.abspath(os.environ["MB_PARENT"])))
        runs = {name: [] for name, _ in trees}
        for r in range(rounds):
            for name, tree in trees:
                env = dict(os.environ, MB_CHILD="1", MB_TREE=tree)
                env.pop("GAOT_LIB", None)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "gno_weighted", str(reps)], env=env, check=True,
                                     capture_output=True, text=True, timeout=600).stdout
                runs[name].append(json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1]))
                print(f"# round {r} {name}: done", flush=True)
        med = lambda v: sorted(v)[len(v) // 2]
        def row(name, key):
            tot = [d[key][0] + d[key][1] for d in runs[name] if key in d]
            if not tot:
                return None
            return med(tot), (max(tot) - min(tot)) / med(tot), med([d[key][0] for d in runs[name]]), med([d[key][1] for d in runs[name]]), \
                max(d[key][2] for d in runs[name])
        print(f"# fwd+bwd of IntegralTransform, ms: median over {rounds} alternated rounds of per-process medians of {reps}; spread = (max - min) / median over rounds")
        for key in sorted(runs["new"][0]):
            if not key.endswith("/attn"):
                continue
            n_ = row("new", key)
            line = f"{key[:-5]:58s} fused weighted {n_[0]:8.3f} (fwd {n_[2]:.3f} bwd {n_[3]:.3f}, spread {100 * n_[1]:.1f} %, peak {n_[4] / 2**20:.0f} MiB)"
            if "parent" in runs:
                g_, u_ = row("parent", key), row("parent", "/".join(key.split("/")[:-2]) + "/plain")
                line += (f" | parent general {g_[0]:8.3f} (spread {100 * g_[1]:.1f} %, peak {g_[4] / 2**20:.0f} MiB) = {g_[0] / n_[0]:.1f} x"
                         f" | parent unweighted fused {u_[0]:8.3f} (spread {100 * u_[1]:.1f} %): weighted = {n_[0] / u_[0]:.2f} x")
            print(line)
        sys.exit(0)
    from gaot_3d_amd.data import make_synthetic_sample
    from gaot_3d_amd.model.layers.integral_transform import IntegralTransform
    from gaot_3d_amd import edgeops as EO
    batch, tokens = make_synthetic_sample(500000, (64, 64, 32), k=8, seed=0, device=dev)
    n, m = 500000, tokens.shape[0]
    tokens = tokens.to(dev)
    res = {}

    def measure(it, yp, xp, f, g, go):
        def once():
            for p in it.parameters():
                p.grad = None
            f.grad = None
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record(); out = it(yp, xp, None, f_y=f, graph=g); e1.record(); out.backward(go); e2.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), e1.elapsed_time(e2)
        once()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ts = [once() for _ in range(reps)]
        peak = torch.cuda.max_memory_allocated() - base
        return sorted(t[0] for t in ts)[len(ts) // 2], sorted(t[1] for t in ts)[len(ts) // 2], peak

    for side, nh, ei, ns, nd, yp, xp in (("enc", 3, batch.encoder_edge_index_s0, n, m, batch.pos, tokens),
                                         ("dec", 2, batch.decoder_edge_index_s0, m, n, tokens, batch.pos)):
        g = ops.build_graph(ei, ns, nd)
        EO.src_to_dst_map(g); EO.dst_to_src_map(g)
        f = torch.randn(ns, 32, device=dev).requires_grad_(); go = torch.randn(nd, 32, device=dev)
        for prec in ("fp32", "bf16"):
            gaot_3d_amd.set_precision(prec)
            for tt in ("linear", "nonlinear", "nonlinear_kernelonly"):
                layers = [6 + (0 if tt == "linear" else 32)] + [64] * nh + [32]
                torch.manual_seed(1)
                res[f"{side}_nh{nh}_E{ei.shape[1]}/{prec}/{tt}/plain"] = measure(
                    IntegralTransform(channel_mlp_layers=layers, transform_type=tt).to(dev), yp, xp, f, g, go)
                for at in ("cosine", "dot_product"):
                    it = IntegralTransform(channel_mlp_layers=layers, transform_type=tt, use_attn=True, coord_dim=3, attention_type=at).to(dev)
                    res[f"{side}_nh{nh}_E{ei.shape[1]}/{prec}/{tt}/{at}/attn"] = measure(it, yp, xp, f, g, go)
                    del it
    print(json.dumps(res))
elif what == "decoder_sample":
    # From query coordinates to predictions under no_grad on the configs[1] decoder (latent 64x64x32 tokens, C = 32, knn k = 8, kernel
    # MLP hidden [64, 64], projection 32 -> 256 -> 1) at 500 K and 8 M random query points, both precisions:
    #   (a) the existing route: neighbour strategy (knn_to_grid + edge_index) -> build_graph (two radix sorts) -> decoder;
    #   (b) MAGNODecoder.sample: per chunk knn_to_grid -> gaot_gno_fwd_knn -> projection, no edge list (MB_CHUNK points, default
    #       the method's own default).
    # (a) and (b) alternate in this one process after a warm-up of each; device events around synchronised work; `reps` rounds; a row
    # is the median with min / max, the peak is the rise of allocated memory over the inputs.  Kept in
    # profiles/decoder_sample_microbench.txt.
    # `--strategy radius|bidirectional`: the reference YAML's decoder instead (config/examples/drivaernet/pressure.yaml: r = 0.033,
    # k_neighbors at its default 1, neighbor_strategy 'bidirectional'; 'radius' = the same decoder on the radius graph alone) with
    #   (a) the route sample fell back to for these strategies: per chunk get_neighbor_strategy (knn_to_grid, radius_pairs, cat,
    #       coalesce) -> build_graph -> decoder, into one preallocated result;
    #   (b) MAGNODecoder.sample: per chunk graph.query_lists (rows written in place, no sort) -> gaot_gno_fwd -> projection.
    # Kept in profiles/decoder_sample_radius_microbench.txt.
    from gaot_3d_amd.data import latent_grid
    from gaot_3d_amd.model.layers.magno import MAGNOConfig, MAGNODecoder
    latent = (64, 64, 32)
    strategy = sys.argv[sys.argv.index("--strategy") + 1] if "--strategy" in sys.argv else "knn"
    if strategy not in ("knn", "radius", "bidirectional"):
        sys.exit(f"--strategy must be radius or bidirectional, got {strategy}")
    rows = strategy != "knn"
    cfg = MAGNOConfig(gno_coord_dim=3, lifting_channels=32, mlp_type="linear", use_geoembed=[True, False],
                      neighbor_strategy=["knn", strategy] if rows else "knn", k_neighbors=1 if rows else 8, gno_radius=0.033,
                      out_gno_channel_mlp_hidden_layers=[64, 64], precompute_edges=False)
    dec = MAGNODecoder(in_channels=32, out_channels=1, gno_config=cfg).to(dev).eval()
    dec.latent_dims = latent
    tokens = latent_grid(latent).to(dev)
    m = tokens.shape[0]
    rn = torch.randn(m, 32, device=dev)
    lat_bidx = torch.zeros(m, dtype=torch.long, device=dev)
    chunk = int(os.environ["MB_CHUNK"]) if os.environ.get("MB_CHUNK") else None

    def timed(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        return e0.elapsed_time(e1), peak, out

    for nq in (500000, 8000000):
        q = torch.rand(nq, 3, device=dev) * 2 - 1
        q_bidx = torch.zeros(nq, dtype=torch.long, device=dev)
        for prec in ("fp32", "bf16"):
            gaot_3d_amd.set_precision(prec)
            with torch.no_grad():
                def route_a():
                    if not rows:
                        return dec._decode(rn, q, q_bidx, tokens, lat_bidx, None, False)
                    out, step = torch.empty(nq, 1, device=dev), chunk or dec.SAMPLE_CHUNK      # sample's fall-back loop
                    for i in range(0, nq, step):
                        out[i:i + step] = dec._decode(rn, q[i:i + step], q_bidx[i:i + step], tokens, lat_bidx, None, False)
                    return out
                route_b = lambda: dec.sample(rn, q, tokens, chunk_points=chunk)
                ra, rb = timed(route_a)[2], timed(route_b)[2]          # warm-up, and the two routes agree
                diff = (ra - rb).abs().max().item()
                del ra, rb
                ta, tb, pa, pb = [], [], 0, 0
                for _ in range(reps):
                    t, p, _o = timed(route_a); ta.append(t); pa = max(pa, p); del _o
                    t, p, _o = timed(route_b); tb.append(t); pb = max(pb, p); del _o
            ta.sort(); tb.sort()
            ma, mb = ta[len(ta) // 2], tb[len(tb) // 2]
            if rows:
                print(f"Nq={nq} {prec} {strategy}: max - min of the rounds (a) {ta[-1] - ta[0]:.3f} ms, (b) {tb[-1] - tb[0]:.3f} ms; (b) - (a) "
                      f"medians {mb - ma:+.3f} ms; (b) peak < (a) peak: {pb < pa}")
            print(f"Nq={nq} {prec}: (a) strategy + build_graph + decoder {ma:9.3f} ms (min {ta[0]:.3f}, max {ta[-1]:.3f}, spread "
                  f"{100 * (ta[-1] - ta[0]) / ma:.1f} %), peak {pa / 2**20:9.1f} MiB")
            print(f"Nq={nq} {prec}: (b) sample (chunk {chunk or dec.SAMPLE_CHUNK})      {mb:9.3f} ms (min {tb[0]:.3f}, max {tb[-1]:.3f}, spread "
                  f"{100 * (tb[-1] - tb[0]) / mb:.1f} %), peak {pb / 2**20:9.1f} MiB  = {mb / ma:.3f} x (a) in time, {pb / max(pa, 1):.3f} x in "
                  f"peak memory; max|a - b| = {diff:.1e}", flush=True)
        del q, q_bidx
elif what == "decoder_jacobian":
    # From query coordinates to predictions AND their spatial Jacobian on the configs[1] decoder (latent 64x64x32 tokens, C = 32, knn
    # k = 8, kernel MLP hidden [64, 64], projection 32 -> 256 -> 1) at 500 K and 8 M random query points, fp32 mode:
    #   (a) the autograd route: neighbour strategy (knn_to_grid + edge_index) -> build_graph (two radix sorts) -> decoder on queries
    #       that require grad -> one backward per output channel, in one piece (MAGNODecoder.sample_jacobian's fall-back route);
    #   (b) MAGNODecoder.sample_jacobian's streaming route: per chunk knn_to_grid -> gaot_gno_fwd_knn_jac -> scale mix -> projection
    #       tangent (MB_CHUNK points, default the method's own default).
    # (a) and (b) alternate in this one process after a warm-up of each; device events around synchronised work; `reps` rounds; a row
    # is the median with min / max, the peak is the rise of allocated memory over the inputs.  Then the split of (b) -- each stage
    # timed over all chunks on its own -- and the tangent kernel against gaot_gno_fwd_knn (precision 0) on the same list.  Kept in
    # profiles/decoder_jacobian_microbench.txt.
    # `--strategy radius|bidirectional`: the reference YAML's decoder instead (config/examples/drivaernet/pressure.yaml: r = 0.033,
    # k_neighbors at its default 1, neighbor_strategy 'bidirectional'; 'radius' = the same decoder on the radius graph alone) with
    #   (a) sample_jacobian's default route for these strategies: per chunk get_neighbor_strategy -> build_graph -> decoder on queries
    #       that require grad -> one backward per output channel;
    #   (b) sample_jacobian(row_lists=True): per chunk graph.query_lists -> gaot_gno_fwd_jac (tangent kernel + fix-up) -> scale mix
    #       -> projection tangent;
    # both with the same chunk (MB_CHUNK points, default the method's own default), then the split of (b) into lists, tangent kernel
    # + fix-up, and mix + projection tangent.  Kept in profiles/decoder_jacobian_rows_microbench.txt.
    from gaot_3d_amd import graph as device_graph
    from gaot_3d_amd.data import latent_grid
    from gaot_3d_amd.model.layers.magno import MAGNOConfig, MAGNODecoder
    gaot_3d_amd.set_precision("fp32")
    latent = (64, 64, 32)
    strategy = sys.argv[sys.argv.index("--strategy") + 1] if "--strategy" in sys.argv else "knn"
    if strategy not in ("knn", "radius", "bidirectional"):
        sys.exit(f"--strategy must be radius or bidirectional, got {strategy}")
    rows = strategy != "knn"
    cfg = MAGNOConfig(gno_coord_dim=3, lifting_channels=32, mlp_type="linear", use_geoembed=[True, False],
                      neighbor_strategy=["knn", strategy] if rows else "knn", k_neighbors=1 if rows else 8, gno_radius=0.033,
                      out_gno_channel_mlp_hidden_layers=[64, 64], precompute_edges=False)
    dec = MAGNODecoder(in_channels=32, out_channels=1, gno_config=cfg).to(dev).eval()
    dec.latent_dims = latent
    tokens = latent_grid(latent).to(dev)
    rn = torch.randn(tokens.shape[0], 32, device=dev)
    chunk = int(os.environ["MB_CHUNK"]) if os.environ.get("MB_CHUNK") else None
    step = chunk or dec.SAMPLE_CHUNK

    def timed(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        return e0.elapsed_time(e1), peak, out

    def median(ts):
        ts = sorted(ts)
        return ts[len(ts) // 2], ts[0], ts[-1]

    for nq in (500000, 8000000):
        q = torch.rand(nq, 3, device=dev) * 2 - 1

        def route_a():
            if rows:
                return dec.sample_jacobian(rn, q, tokens, chunk_points=chunk)       # the default route of these strategies
            dec._stream_grid = lambda *a: None          # the autograd route, the queries in one piece
            try:
                return dec.sample_jacobian(rn, q, tokens, chunk_points=nq)
            finally:
                del dec._stream_grid
        route_b = lambda: dec.sample_jacobian(rn, q, tokens, chunk_points=chunk, row_lists=rows)
        ra, rb = timed(route_a)[2], timed(route_b)[2]          # warm-up, and the two routes agree
        dp = (ra[0] - rb[0]).abs().max().item()
        dj = (ra[1] - rb[1]).abs().max().item() / ra[1].abs().max().item()
        del ra, rb
        ta, tb, pa, pb = [], [], 0, 0
        for _ in range(reps):
            t, p, _o = timed(route_a); ta.append(t); pa = max(pa, p); del _o
            t, p, _o = timed(route_b); tb.append(t); pb = max(pb, p); del _o
        (ma, lo_a, hi_a), (mb, lo_b, hi_b) = median(ta), median(tb)
        if rows:
            print(f"Nq={nq} fp32 {strategy}: max - min of the rounds (a) {hi_a - lo_a:.3f} ms, (b) {hi_b - lo_b:.3f} ms; (b) - (a) medians "
                  f"{mb - ma:+.3f} ms; (b) not slower beyond the spread: {mb - ma <= max(hi_a - lo_a, hi_b - lo_b)}; (b) peak < (a) peak: "
                  f"{pb < pa}")
        print(f"Nq={nq} fp32: (a) autograd route, {f'chunk {step}' if rows else 'one piece'}       {ma:9.3f} ms (min {lo_a:.3f}, max {hi_a:.3f}, spread "
              f"{100 * (hi_a - lo_a) / ma:.1f} %), peak {pa / 2**20:9.1f} MiB")
        print(f"Nq={nq} fp32: (b) sample_jacobian (chunk {step}) {mb:9.3f} ms (min {lo_b:.3f}, max {hi_b:.3f}, spread "
              f"{100 * (hi_b - lo_b) / mb:.1f} %), peak {pb / 2**20:9.1f} MiB  = {mb / ma:.3f} x (a) in time, {pb / max(pa, 1):.3f} x in "
              f"peak memory; (a) - (b) = {ma - mb:.3f} ms against a spread of {max(hi_a - lo_a, hi_b - lo_b):.3f} ms; "
              f"max|pred_a - pred_b| = {dp:.1e}, max|jac_a - jac_b| / peak = {dj:.1e}", flush=True)
        # the split of (b): every stage over all chunks on its own (the stages' inputs kept from the stage before)
        grid = dec._stream_grid(rn, q, tokens)
        if rows:
            with torch.no_grad():
                chunks = [q[i:i + step] for i in range(0, nq, step)]
                t_nbr, t_jac, t_proj = [], [], []
                for _ in range(reps + 1):                                  # the first round warms up and is dropped
                    t, _p, lists = timed(lambda: [device_graph.query_lists(strategy, c, grid, dec.gno_radius, 1) for c in chunks])
                    t_nbr.append(t)
                    edges = sum(g.by_dst.num_edges for g in lists)
                    t, _p, outs = timed(lambda: [dec.gno.jacobian_rows(tokens, c, rn, g) for c, g in zip(chunks, lists)]); t_jac.append(t)
                    t, _p, prj = timed(lambda: [dec.projection.jvp_rows(o, list(j.unbind(0))) for o, j in outs]); t_proj.append(t)
                    del lists, outs, prj
                (mn, _, _), (mj, lo_j, hi_j), (mp, _, _) = (median(t[1:]) for t in (t_nbr, t_jac, t_proj))
                tot = mn + mj + mp
                print(f"Nq={nq} fp32: split of (b): query_lists {mn:.3f} ms ({100 * mn / tot:.0f} %), GNO tangent kernel + fix-up {mj:.3f} ms "
                      f"({100 * mj / tot:.0f} %; min {lo_j:.3f}, max {hi_j:.3f}; {edges} edges), mix + projection tangent {mp:.3f} ms "
                      f"({100 * mp / tot:.0f} %); stages sum to {tot:.3f} ms", flush=True)
            del q, chunks
            continue
        with torch.no_grad():
            chunks = [q[i:i + step] for i in range(0, nq, step)]
            t_nbr, t_jac, t_fwd, t_proj = [], [], [], []
            for _ in range(reps + 1):                                      # the first round warms up and is dropped
                t, _p, nbrs = timed(lambda: [device_graph.knn_to_grid(c, grid, 8) for c in chunks]); t_nbr.append(t)
                t, _p, outs = timed(lambda: [dec.gno.jacobian_knn(tokens, c, n, 8, rn) for c, n in zip(chunks, nbrs)]); t_jac.append(t)
                t, _p, vals = timed(lambda: [dec.gno.forward_knn(tokens, c, n, 8, rn) for c, n in zip(chunks, nbrs)]); t_fwd.append(t)
                del vals
                t, _p, prj = timed(lambda: [dec.projection.jvp_rows(o, list(j.unbind(0))) for o, j in outs]); t_proj.append(t)
                del nbrs, outs, prj
            (mn, _, _), (mj, lo_j, hi_j), (mf, lo_f, hi_f), (mp, _, _) = (median(t[1:]) for t in (t_nbr, t_jac, t_fwd, t_proj))
            tot = mn + mj + mp
            print(f"Nq={nq} fp32: split of (b): neighbour search {mn:.3f} ms ({100 * mn / tot:.0f} %), GNO tangent kernel {mj:.3f} ms "
                  f"({100 * mj / tot:.0f} %), mix + projection tangent {mp:.3f} ms ({100 * mp / tot:.0f} %); stages sum to {tot:.3f} ms")
            print(f"Nq={nq} fp32: gaot_gno_fwd_knn_jac {mj:.3f} ms (min {lo_j:.3f}, max {hi_j:.3f}) against gaot_gno_fwd_knn at precision 0 "
                  f"{mf:.3f} ms (min {lo_f:.3f}, max {hi_f:.3f}) on the same lists: {mj / mf:.2f} x", flush=True)
        del q, chunks
elif what == "decoder_hessian":
    # Second spatial derivatives of the sampled field on the configs[1] decoder (latent 64x64x32 tokens, C = 32, knn k = 8, kernel MLP
    # hidden [64, 64], projection 32 -> 256 -> 1) at 500 K and 8 M random query points, fp32 mode: MAGNODecoder.sample_jacobian (the
    # yardstick: value + three tangent planes), sample_laplacian (three directional 2-jets) and sample_hessian (six), alternated in
    # this one process after a warm-up of each; device events around synchronised work; `reps` rounds (7 for the kept output); a row
    # is the median with max - min, the peak is the rise of allocated memory over the inputs.  Then the split of each -- neighbour
    # search, GNO jet kernel, scale mix + projection, every stage timed over all chunks on its own.  Kept in
    # profiles/decoder_hessian_microbench.txt.
    # `--strategy radius|bidirectional`: the reference YAML's decoder instead (config/examples/drivaernet/pressure.yaml: r = 0.033,
    # k_neighbors at its default 1, neighbor_strategy 'bidirectional'; 'radius' = the same decoder on the radius graph alone) on ROW
    # lists: sample_jacobian(row_lists=True) (the yardstick), sample_laplacian_rows and sample_hessian_rows, alternated in the same
    # way; the split is graph.query_lists, the GNO kernel + its fix-up, and scale mix + projection.  Kept in
    # profiles/decoder_hessian_rows_microbench.txt.
    from gaot_3d_amd import graph as device_graph
    from gaot_3d_amd.data import latent_grid
    from gaot_3d_amd.model.layers.magno import MAGNOConfig, MAGNODecoder, _mix_scales_jet2
    gaot_3d_amd.set_precision("fp32")
    latent = (64, 64, 32)
    strategy = sys.argv[sys.argv.index("--strategy") + 1] if "--strategy" in sys.argv else "knn"
    if strategy not in ("knn", "radius", "bidirectional"):
        sys.exit(f"--strategy must be radius or bidirectional, got {strategy}")
    rows = strategy != "knn"
    cfg = MAGNOConfig(gno_coord_dim=3, lifting_channels=32, mlp_type="linear", use_geoembed=[True, False],
                      neighbor_strategy=["knn", strategy] if rows else "knn", k_neighbors=1 if rows else 8, gno_radius=0.033,
                      out_gno_channel_mlp_hidden_layers=[64, 64], precompute_edges=False)
    dec = MAGNODecoder(in_channels=32, out_channels=1, gno_config=cfg).to(dev).eval()
    dec.latent_dims = latent
    tokens = latent_grid(latent).to(dev)
    rn = torch.randn(tokens.shape[0], 32, device=dev)
    chunk = int(os.environ["MB_CHUNK"]) if os.environ.get("MB_CHUNK") else None
    step = chunk or dec.SAMPLE_CHUNK
    DIRS = dec.HESSIAN_DIRS

    def timed(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        return e0.elapsed_time(e1), peak, out

    def median(ts):
        ts = sorted(ts)
        return ts[len(ts) // 2], ts[0], ts[-1]

    for nq in (500000, 8000000):
        q = torch.rand(nq, 3, device=dev) * 2 - 1
        routes = {"sample_jacobian": lambda: dec.sample_jacobian(rn, q, tokens, chunk_points=chunk, row_lists=rows),
                  "sample_laplacian": lambda: (dec.sample_laplacian_rows if rows else dec.sample_laplacian)(rn, q, tokens, chunk_points=chunk),
                  "sample_hessian": lambda: (dec.sample_hessian_rows if rows else dec.sample_hessian)(rn, q, tokens, chunk_points=chunk)}
        warm = {n: timed(f)[2] for n, f in routes.items()}            # warm-up, and the three agree where they must
        same = (torch.equal(warm["sample_hessian"][0], warm["sample_jacobian"][0]) and torch.equal(warm["sample_hessian"][1], warm["sample_jacobian"][1])
                and torch.equal(warm["sample_laplacian"][0], warm["sample_jacobian"][0]))
        h = warm["sample_hessian"][2]
        trace = torch.equal(warm["sample_laplacian"][1], h[..., 0, 0] + h[..., 1, 1] + h[..., 2, 2])
        del warm, h
        ts, pk = {n: [] for n in routes}, {n: 0 for n in routes}
        for _ in range(reps):
            for n, f in routes.items():
                t, p, _o = timed(f); ts[n].append(t); pk[n] = max(pk[n], p); del _o
        mj, lo_j, hi_j = median(ts["sample_jacobian"])
        for n in routes:
            m, lo, hi = median(ts[n])
            print(f"Nq={nq} fp32{' ' + strategy if rows else ''}: {n + ('_rows' if rows and n != 'sample_jacobian' else ''):21s} (chunk {step}) {m:9.3f} ms (max - min {hi - lo:.3f} ms = {100 * (hi - lo) / m:.1f} %), peak "
                  f"{pk[n] / 2**20:9.1f} MiB  = {m / mj:.2f} x sample_jacobian in time, {pk[n] / max(pk['sample_jacobian'], 1):.2f} x in peak memory")
        print(f"Nq={nq} fp32: pred / jac of sample_hessian and pred of sample_laplacian == sample_jacobian's bit for bit: {same}; "
              f"lap == ordered trace of hess bit for bit: {trace}", flush=True)
        # the split: every stage over all chunks on its own (the stages' inputs kept from the stage before)
        grid = dec._stream_grid(rn, q, tokens)
        if rows:
            with torch.no_grad():
                chunks = [q[i:i + step] for i in range(0, nq, step)]
                t_nbr, t_gno, t_prj = [], {"jac": [], "lap": [], "hess": []}, {"jac": [], "lap": [], "hess": []}
                for _ in range(reps + 1):                                  # the first round warms up and is dropped
                    t, _p, lists = timed(lambda: [device_graph.query_lists(strategy, c, grid, dec.gno_radius, 1) for c in chunks])
                    t_nbr.append(t)
                    edges = sum(g.by_dst.num_edges for g in lists)
                    t, _p, outs = timed(lambda: [dec.gno.jacobian_rows(tokens, c, rn, g) for c, g in zip(chunks, lists)]); t_gno["jac"].append(t)
                    def mix_jvp(c, o, j):
                        p = _mix_scales_jet2(dec, [o], [j], None, c, DIRS[:3])
                        return dec.projection.jvp_rows(p[0], p[1:])
                    t, _p, prj = timed(lambda: [mix_jvp(c, o, j) for c, (o, j) in zip(chunks, outs)]); t_prj["jac"].append(t)
                    del outs, prj
                    for name, nd in (("lap", 3), ("hess", 6)):
                        t, _p, outs = timed(lambda: [dec.gno.jet2_rows(tokens, c, rn, g, DIRS[:nd]) for c, g in zip(chunks, lists)])
                        t_gno[name].append(t)
                        def mix_jet(c, o, a, b, nd=nd):
                            p = _mix_scales_jet2(dec, [o], [a], [b], c, DIRS[:nd])
                            return dec.projection.jet2_rows(p[0], p[1:1 + nd], p[1 + nd:])
                        t, _p, prj = timed(lambda: [mix_jet(c, *oab) for c, oab in zip(chunks, outs)])
                        t_prj[name].append(t)
                        del outs, prj
                    del lists
                mn = median(t_nbr[1:])[0]
                gj = median(t_gno["jac"][1:])
                for name, label, chains in (("jac", "sample_jacobian(row_lists=True)", 4), ("lap", "sample_laplacian_rows", 7),
                                            ("hess", "sample_hessian_rows", 13)):
                    mg, lo_g, hi_g = median(t_gno[name][1:])
                    mp = median(t_prj[name][1:])[0]
                    tot = mn + mg + mp
                    print(f"Nq={nq} fp32 {strategy}: split of {label}: query_lists {mn:.3f} ms ({100 * mn / tot:.0f} %), GNO kernel + fix-up "
                          f"{mg:.3f} ms ({100 * mg / tot:.0f} %; max - min {hi_g - lo_g:.3f}; {edges} edges), mix + projection {mp:.3f} ms "
                          f"({100 * mp / tot:.0f} %); stages sum to {tot:.3f} ms; GNO kernel = {mg / gj[0]:.2f} x the Jacobian kernel's "
                          f"({chains} plane-chains against 4 by count: {chains / 4:.2f} x; yardstick's max - min {gj[2] - gj[1]:.3f} ms)",
                          flush=True)
            del q, chunks
            continue
        with torch.no_grad():
            chunks = [q[i:i + step] for i in range(0, nq, step)]
            t_nbr, t_gno, t_prj = [], {"jac": [], "lap": [], "hess": []}, {"jac": [], "lap": [], "hess": []}
            for _ in range(reps + 1):                                      # the first round warms up and is dropped
                t, _p, nbrs = timed(lambda: [device_graph.knn_to_grid(c, grid, 8) for c in chunks]); t_nbr.append(t)
                t, _p, outs = timed(lambda: [dec.gno.jacobian_knn(tokens, c, n, 8, rn) for c, n in zip(chunks, nbrs)]); t_gno["jac"].append(t)
                def mix_jvp(c, o, j):
                    p = dec._mix_equal_scales([o, *j.unbind(0)], c)
                    return dec.projection.jvp_rows(p[0], p[1:])
                t, _p, prj = timed(lambda: [mix_jvp(c, o, j) for c, (o, j) in zip(chunks, outs)]); t_prj["jac"].append(t)
                del outs, prj
                for name, nd in (("lap", 3), ("hess", 6)):
                    t, _p, outs = timed(lambda: [dec.gno.jet2_knn(tokens, c, n, 8, rn, DIRS[:nd]) for c, n in zip(chunks, nbrs)])
                    t_gno[name].append(t)
                    def mix_jet(c, o, a, b, nd=nd):
                        p = dec._mix_equal_scales([o, *a.unbind(0), *b.unbind(0)], c)
                        return dec.projection.jet2_rows(p[0], p[1:1 + nd], p[1 + nd:])
                    t, _p, prj = timed(lambda: [mix_jet(c, *oab) for c, oab in zip(chunks, outs)])
                    t_prj[name].append(t)
                    del outs, prj
                del nbrs
            mn = median(t_nbr[1:])[0]
            gj = median(t_gno["jac"][1:])
            for name, label, chains in (("jac", "sample_jacobian", 4), ("lap", "sample_laplacian", 7), ("hess", "sample_hessian", 13)):
                mg, lo_g, hi_g = median(t_gno[name][1:])
                mp = median(t_prj[name][1:])[0]
                tot = mn + mg + mp
                print(f"Nq={nq} fp32: split of {label}: neighbour search {mn:.3f} ms ({100 * mn / tot:.0f} %), GNO kernel {mg:.3f} ms "
                      f"({100 * mg / tot:.0f} %; max - min {hi_g - lo_g:.3f}), mix + projection {mp:.3f} ms ({100 * mp / tot:.0f} %); stages sum to "
                      f"{tot:.3f} ms; GNO kernel = {mg / gj[0]:.2f} x the Jacobian kernel's ({chains} plane-chains against 4 by count: "
                      f"{chains / 4:.2f} x; yardstick's max - min {gj[2] - gj[1]:.3f} ms)", flush=True)
        del q, chunks
elif what == "decoder_directional":
    # Derivatives of the sampled field along PER-QUERY directions (MAGNODecoder.sample_directional) on decoder_hessian's decoders --
    # configs[1] (knn, k = 8), or with `--strategy radius|bidirectional` the reference YAML's decoder on row lists -- at 500 K and 8 M
    # random query points with random unit directions, fp32 mode.  In this one process, alternated round by round after a warm-up of
    # each: sample_jacobian (row_lists=True on rows; the yardstick), sample_directional at nd = 1 (d/dn and d^2/dn^2: 3 plane-chains
    # through the per-edge MLP) and at nd = 3 (a local frame: 7), sample_laplacian(_rows) (7, host directions: the same work as
    # nd = 3, so the difference is the cost of per-query directions) and sample_hessian(_rows) (13).  Device events around
    # synchronised work; `reps` rounds (7 for the kept output); a row is the median with max - min, the peak is the rise of allocated
    # memory over the inputs.  Kept in profiles/decoder_directional_microbench.txt / decoder_directional_rows_microbench.txt.
    from gaot_3d_amd.data import latent_grid
    from gaot_3d_amd.model.layers.magno import MAGNOConfig, MAGNODecoder
    gaot_3d_amd.set_precision("fp32")
    latent = (64, 64, 32)
    strategy = sys.argv[sys.argv.index("--strategy") + 1] if "--strategy" in sys.argv else "knn"
    if strategy not in ("knn", "radius", "bidirectional"):
        sys.exit(f"--strategy must be knn, radius or bidirectional, got {strategy}")
    rows = strategy != "knn"
    cfg = MAGNOConfig(gno_coord_dim=3, lifting_channels=32, mlp_type="linear", use_geoembed=[True, False],
                      neighbor_strategy=["knn", strategy] if rows else "knn", k_neighbors=1 if rows else 8, gno_radius=0.033,
                      out_gno_channel_mlp_hidden_layers=[64, 64], precompute_edges=False)
    dec = MAGNODecoder(in_channels=32, out_channels=1, gno_config=cfg).to(dev).eval()
    dec.latent_dims = latent
    tokens = latent_grid(latent).to(dev)
    rn = torch.randn(tokens.shape[0], 32, device=dev)
    chunk = int(os.environ["MB_CHUNK"]) if os.environ.get("MB_CHUNK") else None
    step = chunk or dec.SAMPLE_CHUNK
    sfx = "_rows" if rows else ""

    def timed(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        return e0.elapsed_time(e1), peak, out

    def median(ts):
        ts = sorted(ts)
        return ts[len(ts) // 2], ts[0], ts[-1]

    for nq in (500000, 8000000):
        q = torch.rand(nq, 3, device=dev) * 2 - 1
        n_ = torch.nn.functional.normalize(torch.randn(nq, 3, device=dev), dim=1)       # an orthonormal frame (n, t1, t2) per query
        t1 = torch.randn(nq, 3, device=dev)
        t1 = torch.nn.functional.normalize(t1 - (t1 * n_).sum(1, keepdim=True) * n_, dim=1)
        frames = torch.stack([n_, t1, torch.linalg.cross(n_, t1)], dim=1).contiguous()
        normal = frames[:, :1].contiguous()
        del n_, t1
        routes = {"sample_jacobian": lambda: dec.sample_jacobian(rn, q, tokens, chunk_points=chunk, row_lists=rows),
                  "sample_directional nd=1": lambda: dec.sample_directional(rn, q, normal, tokens, chunk_points=chunk),
                  "sample_directional nd=3": lambda: dec.sample_directional(rn, q, frames, tokens, chunk_points=chunk),
                  "sample_laplacian" + sfx: lambda: (dec.sample_laplacian_rows if rows else dec.sample_laplacian)(rn, q, tokens, chunk_points=chunk),
                  "sample_hessian" + sfx: lambda: (dec.sample_hessian_rows if rows else dec.sample_hessian)(rn, q, tokens, chunk_points=chunk)}
        warm = {n: timed(f)[2] for n, f in routes.items()}            # warm-up, and the results agree where they must
        d3, lap = warm["sample_directional nd=3"], warm["sample_laplacian" + sfx][1]
        same = torch.equal(d3[0], warm["sample_jacobian"][0]) and torch.equal(warm["sample_directional nd=1"][1][..., 0], d3[1][..., 0])
        err = ((d3[2].sum(-1) - lap).abs().max() / lap.abs().max()).item()
        del warm, d3, lap
        ts, pk = {n: [] for n in routes}, {n: 0 for n in routes}
        for _ in range(reps):
            for n, f in routes.items():
                t, p, _o = timed(f); ts[n].append(t); pk[n] = max(pk[n], p); del _o
        med = {n: median(ts[n]) for n in routes}
        mj = med["sample_jacobian"][0]
        for n in routes:
            m, lo, hi = med[n]
            print(f"Nq={nq} fp32{' ' + strategy if rows else ''}: {n:25s} (chunk {step}) {m:9.3f} ms (max - min {hi - lo:.3f} ms = {100 * (hi - lo) / m:.1f} %), "
                  f"peak {pk[n] / 2**20:9.1f} MiB  = {m / mj:.2f} x sample_jacobian in time, {pk[n] / max(pk['sample_jacobian'], 1):.2f} x in peak memory")
        m1, m3 = med["sample_directional nd=1"][0], med["sample_directional nd=3"][0]
        ml, lo_l, hi_l = med["sample_laplacian" + sfx]
        mh = med["sample_hessian" + sfx][0]
        print(f"Nq={nq} fp32{' ' + strategy if rows else ''}: nd=1 : Jacobian = {m1 / mj:.2f} (3 plane-chains against 4 BY COUNT: 0.75), nd=1 : Hessian = {m1 / mh:.2f} "
              f"(3 against 13 by count: 0.23); nd=3 - Laplacian = {m3 - ml:+.3f} ms = {100 * (m3 - ml) / ml:+.1f} % (both 7 plane-chains: the cost of "
              f"per-query directions; the Laplacian's max - min is {hi_l - lo_l:.3f} ms = {100 * (hi_l - lo_l) / ml:.1f} %)")
        print(f"Nq={nq} fp32: pred == sample_jacobian's and slot 0 of nd=3 == nd=1 bit for bit: {same}; max |sum of d2 over the frame - lap| / "
              f"max |lap| = {err:.2e}", flush=True)
        del q, frames, normal
elif what == "decoder_adjoint":
    # The adjoint of the sampled field (MAGNODecoder.sample_vjp) on decoder_hessian's decoders -- configs[1] (knn, k = 8), or with
    # `--strategy radius|bidirectional` the reference YAML's decoder on row lists -- at 500 K and 8 M random query points with a random
    # cotangent, fp32 mode.  In this one process, alternated round by round after a warm-up of each:
    #   (a) sample_vjp, streamed in chunks;
    #   (b) the route it replaces: the general decoder on an edge list for ALL queries under autograd (what forward(query_coord_pos=..)
    #       runs), then torch.autograd.grad of <cotangent, pred> with respect to the latent;
    #   (c) kernels alone on one chunk's lists: gaot_gno_adj against gaot_gno_bwd (precision 0) on the same by-source list and against
    #       the forward (gaot_gno_fwd_knn / gaot_gno_fwd, precision 0) on the same by-query list;
    #   (d) the split of (a) into its stages, one chunk at a time with device events around every stage.
    # Device events around synchronised work; `reps` rounds (7 for the kept output); a row is the median with max - min, the peak is
    # the rise of allocated memory over the inputs.  (a) is also run at 2^20 queries (one chunk) for the peak's independence of Nq.
    # Kept in profiles/decoder_adjoint_microbench.txt / decoder_adjoint_rows_microbench.txt.
    from gaot_3d_amd import graph as device_graph
    from gaot_3d_amd.data import latent_grid
    from gaot_3d_amd.model.layers.magno import MAGNOConfig, MAGNODecoder
    gaot_3d_amd.set_precision("fp32")
    latent = (64, 64, 32)
    strategy = sys.argv[sys.argv.index("--strategy") + 1] if "--strategy" in sys.argv else "knn"
    if strategy not in ("knn", "radius", "bidirectional"):
        sys.exit(f"--strategy must be knn, radius or bidirectional, got {strategy}")
    rows = strategy != "knn"
    cfg = MAGNOConfig(gno_coord_dim=3, lifting_channels=32, mlp_type="linear", use_geoembed=[True, False],
                      neighbor_strategy=["knn", strategy] if rows else "knn", k_neighbors=1 if rows else 8, gno_radius=0.033,
                      out_gno_channel_mlp_hidden_layers=[64, 64], precompute_edges=False)
    dec = MAGNODecoder(in_channels=32, out_channels=1, gno_config=cfg).to(dev).eval()
    dec.latent_dims = latent
    for p_ in dec.parameters():
        p_.requires_grad_(True)              # (b) computes every decoder gradient: gno_bwd has no entry that skips them
    tokens = latent_grid(latent).to(dev)
    m_tok = tokens.shape[0]
    rn = torch.randn(m_tok, 32, device=dev)
    chunk = int(os.environ["MB_CHUNK"]) if os.environ.get("MB_CHUNK") else None
    step = chunk or dec.SAMPLE_CHUNK
    tag = f"fp32{' ' + strategy if rows else ''}"
    fcs = list(dec.gno.channel_mlp.fcs)
    kw_, kb_ = [fc.weight.detach() for fc in fcs], [fc.bias.detach() for fc in fcs]

    def timed(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        return e0.elapsed_time(e1), peak, out

    def median(ts):
        ts = sorted(ts)
        return ts[len(ts) // 2], ts[0], ts[-1]

    def replaced(q, g):
        leaf = rn.detach().clone().requires_grad_(True)
        zq = torch.zeros(q.shape[0], dtype=torch.long, device=dev)
        zl = torch.zeros(m_tok, dtype=torch.long, device=dev)
        pred = dec._decode(leaf, q, zq, tokens, zl, None, False)
        return torch.autograd.grad((pred * g).sum(), leaf)[0]

    def staged(q, g):
        """sample_vjp's chunk loop with device events between its stages (one scale) -> ({stage: ms}, grad)"""
        ev = lambda: torch.cuda.Event(enable_timing=True)
        marks, grad = [], torch.zeros_like(rn)
        with torch.no_grad():
            grid = dec._stream_grid(rn, q, tokens)
            for i in range(0, q.shape[0], step):
                qc, gc = q[i:i + step], g[i:i + step]
                es = [ev() for _ in range(7)]
                es[0].record()
                lists = (device_graph.knn_to_grid(qc, grid, 8), 8) if not rows else \
                    device_graph.query_lists(strategy, qc, grid, dec.gno_radius, int(dec.k_neighbors))
                es[1].record()
                x = dec.gno.forward_knn(tokens, qc, *lists, rn) if not rows else dec.gno(y_pos=tokens, x_pos=qc, edge_index=None, f_y=rn, graph=lists)
                es[2].record()
                dx = dec._project_vjp(x, gc)
                es[3].record()
                gs = device_graph.by_source(lists, m_tok)
                es[4].record()
                part = ops.gno_adjoint(kw_, kb_, tokens, qc, dx, gs, None if rows else 8)
                es[5].record()
                grad.add_(part)
                es[6].record()
                marks.append(es)
                del lists, x, dx, gs, part
        torch.cuda.synchronize()
        names = ("neighbour search", "recomputed forward", "projection + mix cotangent", "by_source", "adjoint kernel + fix-up", "accumulation")
        return {n: sum(es[j].elapsed_time(es[j + 1]) for es in marks) for j, n in enumerate(names)}, grad

    for nq in (500000, 8000000):
        q = torch.rand(nq, 3, device=dev) * 2 - 1
        g = torch.randn(nq, 1, device=dev)
        routes = {"(a) sample_vjp": lambda: dec.sample_vjp(rn, q, g, tokens, chunk_points=chunk),
                  "(b) decoder on an edge list + autograd.grad": lambda: replaced(q, g)}
        warm = {n: timed(f)[2] for n, f in routes.items()}
        a_, b_ = warm["(a) sample_vjp"], warm["(b) decoder on an edge list + autograd.grad"]
        err = ((a_ - b_).abs().max() / b_.abs().max()).item()
        same = torch.equal(a_, staged(q, g)[1])
        del warm, a_, b_
        ts, pk = {n: [] for n in routes}, {n: 0 for n in routes}
        split = []
        for _ in range(reps):
            for n, f in routes.items():
                t, p, _o = timed(f); ts[n].append(t); pk[n] = max(pk[n], p); del _o
            split.append(staged(q, g)[0])
        med = {n: median(ts[n]) for n in routes}
        ma, mb = med["(a) sample_vjp"][0], med["(b) decoder on an edge list + autograd.grad"][0]
        for n in routes:
            m, lo, hi = med[n]
            print(f"Nq={nq} {tag}: {n:45s} (chunk {step if n.startswith('(a)') else nq}) {m:9.3f} ms (max - min {hi - lo:.3f} ms = "
                  f"{100 * (hi - lo) / m:.1f} %), peak {pk[n] / 2**20:9.1f} MiB")
        pa, pb = pk["(a) sample_vjp"], pk["(b) decoder on an edge list + autograd.grad"]
        print(f"Nq={nq} {tag}: (a) : (b) = {ma / mb:.2f} in time, {pa / max(pb, 1):.3f} in peak memory; max |(a) - (b)| / max |(b)| = {err:.2e}; "
              f"the staged loop of (d) returns (a)'s bits: {same}")
        tot = sum(median([s[n] for s in split])[0] for n in split[0])
        for n in split[0]:
            m, lo, hi = median([s[n] for s in split])
            print(f"Nq={nq} {tag}: (d) {n:28s} {m:9.3f} ms (max - min {hi - lo:.3f} ms) = {100 * m / tot:5.1f} % of the stages' sum {tot:.3f} ms")
        # (c) the kernels alone, on the lists of the first chunk
        with torch.no_grad():
            qc = q[:step].contiguous()
            gc = torch.randn(qc.shape[0], 32, device=dev)
            grid = dec._stream_grid(rn, qc, tokens)
            if rows:
                lists = device_graph.query_lists(strategy, qc, grid, dec.gno_radius, int(dec.k_neighbors))
                gboth = device_graph.by_source(lists, m_tok)
                kk, ne = None, lists.by_dst.num_edges
                fwd = ("gaot_gno_fwd", lambda: ops.gno_forward(kw_, kb_, tokens, qc, rn, lists, precision=0))
            else:
                nbr = device_graph.knn_to_grid(qc, grid, 8)
                gsrc = device_graph.by_source((nbr, 8), m_tok)
                ei = torch.stack([nbr.reshape(-1), torch.arange(qc.shape[0], dtype=torch.int32, device=dev).repeat_interleave(8)])
                gboth = ops.BipartiteGraph(ops.csr_build(ei, 1, qc.shape[0]), gsrc.by_src, m_tok, qc.shape[0])
                kk, ne = 8, nbr.numel()
                fwd = ("gaot_gno_fwd_knn", lambda: ops.gno_forward_knn("linear", kw_, kb_, tokens, qc, rn, None, nbr, 8, precision=0))
            kern = {"gaot_gno_adj": lambda: ops.gno_adjoint(kw_, kb_, tokens, qc, gc, gboth, kk),
                    "gaot_gno_bwd (precision 0)": lambda: ops.gno_backward(kw_, kb_, tokens, qc, rn, gc, gboth, precision=0),
                    fwd[0] + " (precision 0)": fwd[1]}
            for f in kern.values():
                f()
            kt = {n: [] for n in kern}
            for _ in range(reps):
                for n, f in kern.items():
                    t, _p, _o = timed(f); kt[n].append(t); del _o
            deg = gboth.by_src.rowptr[1:] - gboth.by_src.rowptr[:-1]
            print(f"Nq={nq} {tag}: (c) one chunk of {qc.shape[0]} queries, {ne} edges; token rows: mean {deg.float().mean().item():.1f}, "
                  f"max {int(deg.max())} edges, {int((deg == 0).sum())} of {m_tok} empty")
            ka = median(kt["gaot_gno_adj"])
            for n in kern:
                m, lo, hi = median(kt[n])
                print(f"Nq={nq} {tag}: (c) {n:32s} {m:9.3f} ms (max - min {hi - lo:.3f} ms); gaot_gno_adj : this = {ka[0] / m:.2f}")
            kbm, kblo, kbhi = median(kt["gaot_gno_bwd (precision 0)"])
            print(f"Nq={nq} {tag}: (c) gaot_gno_bwd - gaot_gno_adj = {kbm - ka[0]:+.3f} ms against max - min {max(kbhi - kblo, ka[2] - ka[1]):.3f} ms of the rounds", flush=True)
        del q, g, qc, gc, gboth
    # (a)'s peak does not grow with the number of queries: 2^20 queries (one chunk) against 8 M
    peaks = {}
    for nq in (1 << 20, 8000000):
        q = torch.rand(nq, 3, device=dev) * 2 - 1
        g = torch.randn(nq, 1, device=dev)
        timed(lambda: dec.sample_vjp(rn, q, g, tokens, chunk_points=chunk))
        peaks[nq] = timed(lambda: dec.sample_vjp(rn, q, g, tokens, chunk_points=chunk))[1] + q.numel() * 4 + g.numel() * 4
        del q, g
    grow, allow = peaks[8000000] - peaks[1 << 20], 8000000 * 16
    print(f"{tag}: (a) peak with its two inputs: 2^20 queries {peaks[1 << 20] / 2**20:.1f} MiB, 8 M queries {peaks[8000000] / 2**20:.1f} MiB: "
          f"+{grow / 2**20:.1f} MiB against {allow / 2**20:.1f} MiB of query_pos and cotangent at 8 M: {'within' if grow <= allow else 'ABOVE'}")
elif what == "decoder_jacobian_adjoint":
    # The adjoint of the field's Jacobian (MAGNODecoder.sample_jacobian_vjp) on decoder_adjoint's decoders -- configs[1] (knn, k = 8), or
    # with `--strategy radius|bidirectional` the reference YAML's decoder on row lists -- at 500 K and 8 M random query points with random
    # cotangents, fp32 mode.  There is no older route to beat; the yardsticks are the two existing calls, alternated with the new one
    # round by round in this one process after a warm-up of each:
    #   (a) sample_jacobian_vjp;   (b) sample_jacobian (row_lists=True);   (c) sample_vjp;
    #   (d) the split of (a) into its stages, one chunk at a time with device events around every stage (one scale);
    #   (e) the kernel alone on one chunk's lists: gaot_gno_adj_jac against gaot_gno_adj on the same by-source list and against
    #       gaot_gno_fwd_knn_jac / gaot_gno_fwd_jac on the same by-query list.
    # Device events around synchronised work; `reps` rounds (7 for the kept output); a row is the median with max - min, the peak is
    # the rise of allocated memory over the inputs.  Kept in profiles/decoder_jacobian_adjoint_microbench.txt / ..._rows_microbench.txt.
    from gaot_3d_amd import graph as device_graph
    from gaot_3d_amd.data import latent_grid
    from gaot_3d_amd.model.layers.magno import MAGNOConfig, MAGNODecoder
    gaot_3d_amd.set_precision("fp32")
    latent = (64, 64, 32)
    strategy = sys.argv[sys.argv.index("--strategy") + 1] if "--strategy" in sys.argv else "knn"
    if strategy not in ("knn", "radius", "bidirectional"):
        sys.exit(f"--strategy must be knn, radius or bidirectional, got {strategy}")
    rows = strategy != "knn"
    cfg = MAGNOConfig(gno_coord_dim=3, lifting_channels=32, mlp_type="linear", use_geoembed=[True, False],
                      neighbor_strategy=["knn", strategy] if rows else "knn", k_neighbors=1 if rows else 8, gno_radius=0.033,
                      out_gno_channel_mlp_hidden_layers=[64, 64], precompute_edges=False)
    dec = MAGNODecoder(in_channels=32, out_channels=1, gno_config=cfg).to(dev).eval()
    dec.latent_dims = latent
    tokens = latent_grid(latent).to(dev)
    m_tok = tokens.shape[0]
    rn = torch.randn(m_tok, 32, device=dev)
    chunk = int(os.environ["MB_CHUNK"]) if os.environ.get("MB_CHUNK") else None
    step = chunk or dec.SAMPLE_CHUNK
    tag = f"fp32{' ' + strategy if rows else ''}"
    fcs = list(dec.gno.channel_mlp.fcs)
    kw_, kb_ = [fc.weight.detach() for fc in fcs], [fc.bias.detach() for fc in fcs]

    def timed(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        return e0.elapsed_time(e1), peak, out

    def median(ts):
        ts = sorted(ts)
        return ts[len(ts) // 2], ts[0], ts[-1]

    def staged(q, gy, gj):
        """sample_jacobian_vjp's chunk loop with device events between its stages (one scale) -> ({stage: ms}, grad)"""
        ev = lambda: torch.cuda.Event(enable_timing=True)
        marks, grad = [], torch.zeros_like(rn)
        with torch.no_grad():
            grid = dec._stream_grid(rn, q, tokens)
            for i in range(0, q.shape[0], step):
                qc = q[i:i + step]
                es = [ev() for _ in range(7)]
                es[0].record()
                lists = (device_graph.knn_to_grid(qc, grid, 8), 8) if not rows else \
                    [device_graph.query_lists(strategy, qc, grid, dec.gno_radius, int(dec.k_neighbors))]
                es[1].record()
                planes = dec._jet_planes(rn, qc, tokens, lists)
                es[2].record()
                d = dec._project_jac_vjp(planes, gy[i:i + step], gj[i:i + step])
                dj = torch.stack(d[1:])
                es[3].record()
                gs = device_graph.by_source(lists if not rows else lists[0], m_tok)
                es[4].record()
                part = ops.gno_adjoint_jac(kw_, kb_, tokens, qc, d[0], dj, gs, None if rows else 8)
                es[5].record()
                grad.add_(part)
                es[6].record()
                marks.append(es)
                del lists, planes, d, dj, gs, part
        torch.cuda.synchronize()
        names = ("neighbour search", "recomputed planes (value + 3 tangents)", "projection cotangent", "by_source",
                 "adjoint kernel + fix-up", "accumulation")
        return {n: sum(es[j].elapsed_time(es[j + 1]) for es in marks) for j, n in enumerate(names)}, grad

    for nq in (500000, 8000000):
        q = torch.rand(nq, 3, device=dev) * 2 - 1
        gy, gj = torch.randn(nq, 1, device=dev), torch.randn(nq, 1, 3, device=dev)
        routes = {"(a) sample_jacobian_vjp": lambda: dec.sample_jacobian_vjp(rn, q, gy, gj, tokens, chunk_points=chunk),
                  "(b) sample_jacobian": lambda: dec.sample_jacobian(rn, q, tokens, chunk_points=chunk, row_lists=True),
                  "(c) sample_vjp": lambda: dec.sample_vjp(rn, q, gy, tokens, chunk_points=chunk)}
        warm = {n: timed(f)[2] for n, f in routes.items()}
        same = torch.equal(warm["(a) sample_jacobian_vjp"], staged(q, gy, gj)[1])
        del warm
        ts, pk = {n: [] for n in routes}, {n: 0 for n in routes}
        split = []
        for _ in range(reps):
            for n, f in routes.items():
                t, p, _o = timed(f); ts[n].append(t); pk[n] = max(pk[n], p); del _o
            split.append(staged(q, gy, gj)[0])
        med = {n: median(ts[n]) for n in routes}
        for n in routes:
            m, lo, hi = med[n]
            print(f"Nq={nq} {tag}: {n:26s} (chunk {step}) {m:9.3f} ms (max - min {hi - lo:.3f} ms = {100 * (hi - lo) / m:.1f} %), "
                  f"peak {pk[n] / 2**20:9.1f} MiB")
        ma, mb, mc = (med[n][0] for n in routes)
        print(f"Nq={nq} {tag}: (a) : (b) = {ma / mb:.2f}, (a) : (c) = {ma / mc:.2f} in time (by count of plane-chains (4 + 4) : (1 + 1) = 4 "
              f"against (c)); the staged loop of (d) returns (a)'s bits: {same}")
        tot = sum(median([s[n] for s in split])[0] for n in split[0])
        for n in split[0]:
            m, lo, hi = median([s[n] for s in split])
            print(f"Nq={nq} {tag}: (d) {n:38s} {m:9.3f} ms (max - min {hi - lo:.3f} ms) = {100 * m / tot:5.1f} % of the stages' sum {tot:.3f} ms")
        # (e) the kernels alone, on the lists of the first chunk
        with torch.no_grad():
            qc = q[:step].contiguous()
            gc, gjc = torch.randn(qc.shape[0], 32, device=dev), torch.randn(3, qc.shape[0], 32, device=dev)
            grid = dec._stream_grid(rn, qc, tokens)
            if rows:
                lists = device_graph.query_lists(strategy, qc, grid, dec.gno_radius, int(dec.k_neighbors))
                gboth = device_graph.by_source(lists, m_tok)
                kk, ne = None, lists.by_dst.num_edges
                fwd = ("gaot_gno_fwd_jac", lambda: ops.gno_forward_jac("linear", kw_, kb_, tokens, qc, rn, None, lists))
            else:
                nbr = device_graph.knn_to_grid(qc, grid, 8)
                gboth = device_graph.by_source((nbr, 8), m_tok)
                kk, ne = 8, nbr.numel()
                fwd = ("gaot_gno_fwd_knn_jac", lambda: ops.gno_forward_knn_jac("linear", kw_, kb_, tokens, qc, rn, None, nbr, 8))
            kern = {"gaot_gno_adj_jac": lambda: ops.gno_adjoint_jac(kw_, kb_, tokens, qc, gc, gjc, gboth, kk),
                    "gaot_gno_adj": lambda: ops.gno_adjoint(kw_, kb_, tokens, qc, gc, gboth, kk),
                    fwd[0]: fwd[1]}
            for f in kern.values():
                f()
            kt = {n: [] for n in kern}
            for _ in range(reps):
                for n, f in kern.items():
                    t, _p, _o = timed(f); kt[n].append(t); del _o
            print(f"Nq={nq} {tag}: (e) one chunk of {qc.shape[0]} queries, {ne} edges, {len(fcs) - 1} hidden layers")
            ka = median(kt["gaot_gno_adj_jac"])
            for n in kern:
                m, lo, hi = median(kt[n])
                print(f"Nq={nq} {tag}: (e) {n:24s} {m:9.3f} ms (max - min {hi - lo:.3f} ms); gaot_gno_adj_jac : this = {ka[0] / m:.2f}", flush=True)
        del q, gy, gj, qc, gc, gjc, gboth
elif what == "decoder_laplacian_adjoint":
    # The adjoint of the field's Laplacian (MAGNODecoder.sample_laplacian_vjp) on decoder_jacobian_adjoint's decoders -- configs[1] (knn,
    # k = 8), or with `--strategy radius|bidirectional` the reference YAML's decoder on row lists -- at 500 K and 8 M random query points
    # with random cotangents, fp32 mode.  There is no older route to beat; the yardsticks are the existing calls, alternated with the new
    # one round by round in this one process after a warm-up of each:
    #   (a) sample_laplacian_vjp;   (b) sample_laplacian / sample_laplacian_rows;   (c) sample_jacobian_vjp;
    #   (d) the split of (a) into its stages, one chunk at a time with device events around every stage (one scale);
    #   (e) the kernel alone on one chunk's lists: gaot_gno_adj_jet2 (three axes, one second-order plane) against gaot_gno_adj_jac on
    #       the same by-source list and against gaot_gno_fwd_knn_jet2 / gaot_gno_fwd_jet2 (three axes) on the same by-query list;
    #   (f) the projection cotangent's elementwise middle on one chunk's rows: gaot_mlp2_lap_cot_mid against the same expression as
    #       fp32 tensor operations.
    # Device events around synchronised work; `reps` rounds (7 for the kept output); a row is the median with max - min, the peak is
    # the rise of allocated memory over the inputs.  Kept in profiles/decoder_laplacian_adjoint_microbench.txt / ..._rows_microbench.txt.
    from gaot_3d_amd import graph as device_graph
    from gaot_3d_amd.data import latent_grid
    from gaot_3d_amd.model.layers.magno import MAGNOConfig, MAGNODecoder
    gaot_3d_amd.set_precision("fp32")
    latent = (64, 64, 32)
    strategy = sys.argv[sys.argv.index("--strategy") + 1] if "--strategy" in sys.argv else "knn"
    if strategy not in ("knn", "radius", "bidirectional"):
        sys.exit(f"--strategy must be knn, radius or bidirectional, got {strategy}")
    rows = strategy != "knn"
    cfg = MAGNOConfig(gno_coord_dim=3, lifting_channels=32, mlp_type="linear", use_geoembed=[True, False],
                      neighbor_strategy=["knn", strategy] if rows else "knn", k_neighbors=1 if rows else 8, gno_radius=0.033,
                      out_gno_channel_mlp_hidden_layers=[64, 64], precompute_edges=False)
    dec = MAGNODecoder(in_channels=32, out_channels=1, gno_config=cfg).to(dev).eval()
    dec.latent_dims = latent
    tokens = latent_grid(latent).to(dev)
    m_tok = tokens.shape[0]
    rn = torch.randn(m_tok, 32, device=dev)
    chunk = int(os.environ["MB_CHUNK"]) if os.environ.get("MB_CHUNK") else None
    step = chunk or dec.SAMPLE_CHUNK
    tag = f"fp32{' ' + strategy if rows else ''}"
    fcs = list(dec.gno.channel_mlp.fcs)
    kw_, kb_ = [fc.weight.detach() for fc in fcs], [fc.bias.detach() for fc in fcs]
    axes = dec.LAP_VJP_DIRS
    hid = dec.projection.fcs[0].weight.shape[0]

    def timed(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        return e0.elapsed_time(e1), peak, out

    def median(ts):
        ts = sorted(ts)
        return ts[len(ts) // 2], ts[0], ts[-1]

    def staged(q, gy, gj, gl):
        """sample_laplacian_vjp's chunk loop with device events between its stages (one scale) -> ({stage: ms}, grad)"""
        ev = lambda: torch.cuda.Event(enable_timing=True)
        marks, grad = [], torch.zeros_like(rn)
        with torch.no_grad():
            grid = dec._stream_grid(rn, q, tokens)
            for i in range(0, q.shape[0], step):
                qc = q[i:i + step]
                es = [ev() for _ in range(7)]
                es[0].record()
                lists = (device_graph.knn_to_grid(qc, grid, 8), 8) if not rows else \
                    [device_graph.query_lists(strategy, qc, grid, dec.gno_radius, int(dec.k_neighbors))]
                es[1].record()
                planes = dec._jet_planes(rn, qc, tokens, lists, axes)
                es[2].record()
                d = dec._project_lap_vjp(planes, gy[i:i + step], gj[i:i + step], gl[i:i + step])
                d1, d2 = torch.stack(d[1:4]), d[4].unsqueeze(0)
                es[3].record()
                gs = device_graph.by_source(lists if not rows else lists[0], m_tok)
                es[4].record()
                part = ops.gno_adjoint_jet2(kw_, kb_, tokens, qc, axes, d[0], d1, d2, gs, None if rows else 8)
                es[5].record()
                grad.add_(part)
                es[6].record()
                marks.append(es)
                del lists, planes, d, d1, d2, gs, part
        torch.cuda.synchronize()
        names = ("neighbour search", "recomputed planes (value + 3 x 2 jets)", "projection cotangent", "by_source",
                 "adjoint kernel + fix-up", "accumulation")
        return {n: sum(es[j].elapsed_time(es[j + 1]) for es in marks) for j, n in enumerate(names)}, grad

    def mid_as_tensor_ops(zus, a, ad, al, b1):
        """gaot_mlp2_lap_cot_mid's expression as fp32 tensor operations -> [5, rows, hidden]"""
        z = zus[0] + b1
        phi = torch.exp(-0.5 * z * z) * 0.3989422804014327
        a1 = 0.5 * (1.0 + torch.erf(z * 0.7071067811865476)) + z * phi
        a2, a3 = phi * (2.0 - z * z), phi * z * (z * z - 4.0)
        u = zus[1:4]
        dz = a1 * a + a2 * (u * ad).sum(0) + (a3 * (u * u).sum(0) + a2 * zus[4]) * al
        return torch.cat([dz[None], a1 * ad + (2.0 * a2 * al) * u, (a1 * al)[None]])

    lap_fwd = dec.sample_laplacian_rows if rows else dec.sample_laplacian
    for nq in (500000, 8000000):
        q = torch.rand(nq, 3, device=dev) * 2 - 1
        gy, gj, gl = torch.randn(nq, 1, device=dev), torch.randn(nq, 1, 3, device=dev), torch.randn(nq, 1, device=dev)
        routes = {"(a) sample_laplacian_vjp": lambda: dec.sample_laplacian_vjp(rn, q, gy, gj, gl, tokens, chunk_points=chunk),
                  "(b) sample_laplacian": lambda: lap_fwd(rn, q, tokens, chunk_points=chunk),
                  "(c) sample_jacobian_vjp": lambda: dec.sample_jacobian_vjp(rn, q, gy, gj, tokens, chunk_points=chunk)}
        warm = {n: timed(f)[2] for n, f in routes.items()}
        same = torch.equal(warm["(a) sample_laplacian_vjp"], staged(q, gy, gj, gl)[1])
        del warm
        ts, pk = {n: [] for n in routes}, {n: 0 for n in routes}
        split = []
        for _ in range(reps):
            for n, f in routes.items():
                t, p, _o = timed(f); ts[n].append(t); pk[n] = max(pk[n], p); del _o
            split.append(staged(q, gy, gj, gl)[0])
        med = {n: median(ts[n]) for n in routes}
        for n in routes:
            m, lo, hi = med[n]
            print(f"Nq={nq} {tag}: {n:26s} (chunk {step}) {m:9.3f} ms (max - min {hi - lo:.3f} ms = {100 * (hi - lo) / m:.1f} %), "
                  f"peak {pk[n] / 2**20:9.1f} MiB")
        ma, mb, mc = (med[n][0] for n in routes)
        print(f"Nq={nq} {tag}: (a) : (b) = {ma / mb:.2f}, (a) : (c) = {ma / mc:.2f} in time (by count of plane-chains (7 + 7) : 7 = 2 "
              f"against (b), (7 + 7) : (4 + 4) = 1.75 against (c)); the staged loop of (d) returns (a)'s bits: {same}")
        tot = sum(median([s[n] for s in split])[0] for n in split[0])
        for n in split[0]:
            m, lo, hi = median([s[n] for s in split])
            print(f"Nq={nq} {tag}: (d) {n:38s} {m:9.3f} ms (max - min {hi - lo:.3f} ms) = {100 * m / tot:5.1f} % of the stages' sum {tot:.3f} ms")
        # (e) the kernels alone, on the lists of the first chunk
        with torch.no_grad():
            qc = q[:step].contiguous()
            nc = qc.shape[0]
            gc, gjc = torch.randn(nc, 32, device=dev), torch.randn(3, nc, 32, device=dev)
            glc = torch.randn(1, nc, 32, device=dev)
            grid = dec._stream_grid(rn, qc, tokens)
            if rows:
                lists = device_graph.query_lists(strategy, qc, grid, dec.gno_radius, int(dec.k_neighbors))
                gboth = device_graph.by_source(lists, m_tok)
                kk, ne = None, lists.by_dst.num_edges
                fwd = ("gaot_gno_fwd_jet2", lambda: ops.gno_forward_jet2("linear", kw_, kb_, tokens, qc, rn, None, lists, axes))
            else:
                nbr = device_graph.knn_to_grid(qc, grid, 8)
                gboth = device_graph.by_source((nbr, 8), m_tok)
                kk, ne = 8, nbr.numel()
                fwd = ("gaot_gno_fwd_knn_jet2", lambda: ops.gno_forward_knn_jet2("linear", kw_, kb_, tokens, qc, rn, None, nbr, 8, axes))
            kern = {"gaot_gno_adj_jet2": lambda: ops.gno_adjoint_jet2(kw_, kb_, tokens, qc, axes, gc, gjc, glc, gboth, kk),
                    "gaot_gno_adj_jac": lambda: ops.gno_adjoint_jac(kw_, kb_, tokens, qc, gc, gjc, gboth, kk),
                    fwd[0]: fwd[1]}
            for f in kern.values():
                f()
            kt = {n: [] for n in kern}
            for _ in range(reps):
                for n, f in kern.items():
                    t, _p, _o = timed(f); kt[n].append(t); del _o
            print(f"Nq={nq} {tag}: (e) one chunk of {nc} queries, {ne} edges, {len(fcs) - 1} hidden layers")
            ka = median(kt["gaot_gno_adj_jet2"])
            for n in kern:
                m, lo, hi = median(kt[n])
                print(f"Nq={nq} {tag}: (e) {n:24s} {m:9.3f} ms (max - min {hi - lo:.3f} ms); gaot_gno_adj_jet2 : this = {ka[0] / m:.2f}", flush=True)
            del gc, gjc, glc, gboth
            # (f) the projection cotangent's middle alone, on the rows of one of _project_lap_vjp's blocks
            mr = nc if hid <= 32 else max(1024, nc * 32 // hid)
            zus, a5 = torch.randn(5, mr, hid, device=dev), torch.randn(5, mr, hid, device=dev)
            b1 = dec.projection.fcs[0].bias.detach()
            mids = {"gaot_mlp2_lap_cot_mid": lambda: ops.mlp2_lap_cot_mid(zus, a5[0], a5[1:4], a5[4], b1),
                    "tensor operations": lambda: mid_as_tensor_ops(zus, a5[0], a5[1:4], a5[4], b1)}
            close = (mids["gaot_mlp2_lap_cot_mid"]() - mids["tensor operations"]()).abs().max().item()
            mt, mp = {n: [] for n in mids}, {n: 0 for n in mids}
            for _ in range(reps):
                for n, f in mids.items():
                    t, p, _o = timed(f); mt[n].append(t); mp[n] = max(mp[n], p); del _o
            km = median(mt["gaot_mlp2_lap_cot_mid"])
            print(f"Nq={nq} {tag}: (f) the middle on [{mr}, {hid}] planes ({15 * mr * hid * 4 / 2**20:.0f} MiB read and written); "
                  f"max |kernel - tensor operations| = {close:.2e}")
            for n in mids:
                m, lo, hi = median(mt[n])
                print(f"Nq={nq} {tag}: (f) {n:24s} {m:9.3f} ms (max - min {hi - lo:.3f} ms), peak {mp[n] / 2**20:8.1f} MiB; "
                      f"this : gaot_mlp2_lap_cot_mid = {m / km[0]:.2f}", flush=True)
            del zus, a5
        del q, gy, gj, gl, qc
elif what in ("decoder_directional_adjoint", "decoder_hessian_adjoint"):
    # The adjoints of the field's directional derivatives (MAGNODecoder.sample_directional_vjp, per-query directions) and of its
    # Hessian (sample_hessian_vjp) on decoder_laplacian_adjoint's decoders -- configs[1] (knn, k = 8), or with
    # `--strategy radius|bidirectional` the reference YAML's decoder on row lists -- at 500 K and 8 M random query points with random
    # unit directions and random cotangents, fp32 mode.  There is no older route to beat; the yardsticks are the existing calls,
    # alternated with the new ones round by round in this one process after a warm-up of each:
    #   directional: (a1) sample_directional_vjp nd = 1;  (a3) nd = 3;  (b) sample_directional nd = 3;  (c) sample_laplacian_vjp;
    #                (j) sample_jacobian_vjp
    #   hessian:     (a) sample_hessian_vjp;  (b) sample_hessian / sample_hessian_rows;  (c) sample_laplacian_vjp;  (j) sample_jacobian_vjp
    #   (d) the split of the new call (nd = 3 / the six directions) into its stages, one chunk at a time with device events (one scale);
    #   (e) the kernel alone on one chunk's lists: gaot_gno_adj_jet2_qd against gaot_gno_adj_jet2 on the same by-source list, the same
    #       directions on every query (the results are compared bit for bit), nd = 1, 3, 6, a second-order plane per direction;
    #   (f) the projection cotangent's elementwise middle on one block's rows: gaot_mlp2_jet2_cot_mid against the same expression as
    #       fp32 tensor operations.
    # Device events around synchronised work; `reps` rounds (7 for the kept output); a row is the median with max - min, the peak is
    # the rise of allocated memory over the inputs.  Kept in profiles/decoder_{directional,hessian}_adjoint[_rows]_microbench.txt.
    from gaot_3d_amd import graph as device_graph
    from gaot_3d_amd.data import latent_grid
    from gaot_3d_amd.model.layers.magno import MAGNOConfig, MAGNODecoder
    gaot_3d_amd.set_precision("fp32")
    latent = (64, 64, 32)
    strategy = sys.argv[sys.argv.index("--strategy") + 1] if "--strategy" in sys.argv else "knn"
    if strategy not in ("knn", "radius", "bidirectional"):
        sys.exit(f"--strategy must be knn, radius or bidirectional, got {strategy}")
    rows = strategy != "knn"
    hessian = what == "decoder_hessian_adjoint"
    cfg = MAGNOConfig(gno_coord_dim=3, lifting_channels=32, mlp_type="linear", use_geoembed=[True, False],
                      neighbor_strategy=["knn", strategy] if rows else "knn", k_neighbors=1 if rows else 8, gno_radius=0.033,
                      out_gno_channel_mlp_hidden_layers=[64, 64], precompute_edges=False)
    dec = MAGNODecoder(in_channels=32, out_channels=1, gno_config=cfg).to(dev).eval()
    dec.latent_dims = latent
    tokens = latent_grid(latent).to(dev)
    m_tok = tokens.shape[0]
    rn = torch.randn(m_tok, 32, device=dev)
    chunk = int(os.environ["MB_CHUNK"]) if os.environ.get("MB_CHUNK") else None
    step = chunk or dec.SAMPLE_CHUNK
    tag = f"fp32{' ' + strategy if rows else ''}"
    fcs = list(dec.gno.channel_mlp.fcs)
    kw_, kb_ = [fc.weight.detach() for fc in fcs], [fc.bias.detach() for fc in fcs]
    hid = dec.projection.fcs[0].weight.shape[0]
    sizes = [int(a) for a in os.environ["MB_NQ"].split(",")] if os.environ.get("MB_NQ") else [500000, 8000000]

    def timed(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        return e0.elapsed_time(e1), peak, out

    def median(ts):
        ts = sorted(ts)
        return ts[len(ts) // 2], ts[0], ts[-1]

    def staged(q, dirs, gy, g1, g2):
        """the new call's chunk loop with device events between its stages (one scale) -> ({stage: ms}, grad); ``dirs``: the
        per-query directions [Nq, nd, 3] or the six host directions"""
        ev = lambda: torch.cuda.Event(enable_timing=True)
        marks, grad = [], torch.zeros_like(rn)
        qd = isinstance(dirs, torch.Tensor)
        with torch.no_grad():
            grid = dec._stream_grid(rn, q, tokens)
            for i in range(0, q.shape[0], step):
                qc, dc = q[i:i + step], dirs[i:i + step] if qd else dirs
                es = [ev() for _ in range(7)]
                es[0].record()
                lists = (device_graph.knn_to_grid(qc, grid, 8), 8) if not rows else \
                    [device_graph.query_lists(strategy, qc, grid, dec.gno_radius, int(dec.k_neighbors))]
                es[1].record()
                planes = dec._jet_planes(rn, qc, tokens, lists, dc)
                es[2].record()
                d = dec._project_cot(3, planes, gy[i:i + step], g1[i:i + step], g2[i:i + step])
                per = dec._mix_cot(d, qc, not rows, None, None, dc)[0]
                es[3].record()
                gs = device_graph.by_source(lists if not rows else lists[0], m_tok)
                es[4].record()
                part = dec.gno._adjoint(tokens, qc, per, gs, lists if not rows else None, dc, qd=qd)
                es[5].record()
                grad.add_(part)
                es[6].record()
                marks.append(es)
                del lists, planes, d, per, gs, part
        torch.cuda.synchronize()
        nd = dirs.shape[1] if qd else len(dirs)
        names = ("neighbour search", f"recomputed planes (value + {nd} x 2 jets)", "projection cotangent", "by_source",
                 "adjoint kernel + fix-up", "accumulation")
        return {n: sum(es[j].elapsed_time(es[j + 1]) for es in marks) for j, n in enumerate(names)}, grad

    def mid_as_tensor_ops(zus, a, ab, b1):
        """gaot_mlp2_jet2_cot_mid's expression as fp32 tensor operations -> [1 + 2 nd, rows, hidden]"""
        nd = ab.shape[0] // 2
        z = zus[0] + b1
        phi = torch.exp(-0.5 * z * z) * 0.3989422804014327
        a1 = 0.5 * (1.0 + torch.erf(z * 0.7071067811865476)) + z * phi
        a2, a3 = phi * (2.0 - z * z), phi * z * (z * z - 4.0)
        u, sv, ad, bd = zus[1:1 + nd], zus[1 + nd:], ab[:nd], ab[nd:]
        dz = a1 * a + a2 * (u * ad).sum(0) + ((a3 * u * u + a2 * sv) * bd).sum(0)
        return torch.cat([dz[None], a1 * ad + (2.0 * a2) * u * bd, a1 * bd])

    for nq in sizes:
        q = torch.rand(nq, 3, device=dev) * 2 - 1
        v = torch.nn.functional.normalize(torch.randn(nq, 3, 3, device=dev), dim=2)
        v1 = v[:, :1].contiguous()
        gy, gj, gl = torch.randn(nq, 1, device=dev), torch.randn(nq, 1, 3, device=dev), torch.randn(nq, 1, device=dev)
        g1, g2 = torch.randn(nq, 1, 3, device=dev), torch.randn(nq, 1, 3, device=dev)
        g11, g21 = g1[:, :, :1].contiguous(), g2[:, :, :1].contiguous()
        gh = torch.randn(nq, 1, 3, 3, device=dev)
        if hessian:
            hess_fwd = dec.sample_hessian_rows if rows else dec.sample_hessian
            new = "(a) sample_hessian_vjp"
            routes = {new: lambda: dec.sample_hessian_vjp(rn, q, gy, gj, gh, tokens, chunk_points=chunk),
                      "(b) sample_hessian": lambda: hess_fwd(rn, q, tokens, chunk_points=chunk)}
            p6, s6 = dec._polarise_cot(gj, gh)
            split_args = (dec.HESSIAN_DIRS, gy, p6, s6)
            counts = "13 + 13 plane-chains against the Laplacian adjoint's 7 + 7"
        else:
            new = "(a3) sample_directional_vjp nd=3"
            routes = {"(a1) sample_directional_vjp nd=1": lambda: dec.sample_directional_vjp(rn, q, v1, gy, g11, g21, tokens, chunk_points=chunk),
                      new: lambda: dec.sample_directional_vjp(rn, q, v, gy, g1, g2, tokens, chunk_points=chunk),
                      "(b) sample_directional nd=3": lambda: dec.sample_directional(rn, q, v, tokens, chunk_points=chunk)}
            split_args = (v, gy, g1, g2)
            counts = "nd = 1: 3 + 3 plane-chains, nd = 3: 7 + 7, against the Laplacian adjoint's 7 + 7"
        routes["(c) sample_laplacian_vjp"] = lambda: dec.sample_laplacian_vjp(rn, q, gy, gj, gl, tokens, chunk_points=chunk)
        routes["(j) sample_jacobian_vjp"] = lambda: dec.sample_jacobian_vjp(rn, q, gy, gj, tokens, chunk_points=chunk)
        warm = {n: timed(f)[2] for n, f in routes.items()}
        same = torch.equal(warm[new], staged(q, *split_args)[1])
        del warm
        ts, pk = {n: [] for n in routes}, {n: 0 for n in routes}
        split = []
        for _ in range(reps):
            for n, f in routes.items():
                t, p, _o = timed(f); ts[n].append(t); pk[n] = max(pk[n], p); del _o
            split.append(staged(q, *split_args)[0])
        med = {n: median(ts[n]) for n in routes}
        for n in routes:
            m, lo, hi = med[n]
            print(f"Nq={nq} {tag}: {n:34s} (chunk {step}) {m:9.3f} ms (max - min {hi - lo:.3f} ms = {100 * (hi - lo) / m:.1f} %), "
                  f"peak {pk[n] / 2**20:9.1f} MiB")
        mc = med["(c) sample_laplacian_vjp"][0]
        print(f"Nq={nq} {tag}: " + ", ".join(f"{n.split()[0]} : (c) = {med[n][0] / mc:.2f}" for n in routes if n[1] == "a")
              + f" in time (by count: {counts}); the staged loop of (d) returns {new.split()[0]}'s bits: {same}")
        tot = sum(median([s_[n] for s_ in split])[0] for n in split[0])
        for n in split[0]:
            m, lo, hi = median([s_[n] for s_ in split])
            print(f"Nq={nq} {tag}: (d) {n:38s} {m:9.3f} ms (max - min {hi - lo:.3f} ms) = {100 * m / tot:5.1f} % of the stages' sum {tot:.3f} ms")
        with torch.no_grad():
            # (e) the kernels alone, on the lists of the first chunk
            qc = q[:step].contiguous()
            nc = qc.shape[0]
            grid = dec._stream_grid(rn, qc, tokens)
            if rows:
                lists = device_graph.query_lists(strategy, qc, grid, dec.gno_radius, int(dec.k_neighbors))
                gboth, kk, ne = device_graph.by_source(lists, m_tok), None, lists.by_dst.num_edges
            else:
                nbr = device_graph.knn_to_grid(qc, grid, 8)
                gboth, kk, ne = device_graph.by_source((nbr, 8), m_tok), 8, nbr.numel()
            print(f"Nq={nq} {tag}: (e) one chunk of {nc} queries, {ne} edges, {len(fcs) - 1} hidden layers")
            for nd in (1, 3, 6):
                hd = dec.HESSIAN_DIRS[:nd]
                vd = torch.tensor(hd, device=dev)[None].expand(nc, nd, 3).contiguous()
                gc, pc, sc = torch.randn(nc, 32, device=dev), torch.randn(nd, nc, 32, device=dev), torch.randn(nd, nc, 32, device=dev)
                kern = {"gaot_gno_adj_jet2_qd": lambda: ops.gno_adjoint_jet2_qd(kw_, kb_, tokens, qc, vd, gc, pc, sc, gboth, kk),
                        "gaot_gno_adj_jet2": lambda: ops.gno_adjoint_jet2(kw_, kb_, tokens, qc, hd, gc, pc, sc, gboth, kk)}
                bits = torch.equal(*(f() for f in kern.values()))
                kt = {n: [] for n in kern}
                for _ in range(reps):
                    for n, f in kern.items():
                        t, _p, _o = timed(f); kt[n].append(t); del _o
                kh = median(kt["gaot_gno_adj_jet2"])
                for n in kern:
                    m, lo, hi = median(kt[n])
                    print(f"Nq={nq} {tag}: (e) nd={nd} {n:22s} {m:9.3f} ms (max - min {hi - lo:.3f} ms); this : gaot_gno_adj_jet2 = "
                          f"{m / kh[0]:.3f}; the same bits: {bits}", flush=True)
                del vd, gc, pc, sc
            del gboth
            # (f) the projection cotangent's middle alone, on the rows of one of _project_cot's blocks
            b1 = dec.projection.fcs[0].bias.detach()
            for nd in (1, 3, 6):
                npl = 1 + 2 * nd
                mr = nc if hid <= 32 else max(1024, nc * 32 // hid)
                if npl > 5:
                    mr = max(1024, mr * 5 // npl)
                zus, acot = torch.randn(npl, mr, hid, device=dev), torch.randn(npl, mr, hid, device=dev)
                mids = {"gaot_mlp2_jet2_cot_mid": lambda: ops.mlp2_jet2_cot_mid(zus, acot[0], acot[1:], b1),
                        "tensor operations": lambda: mid_as_tensor_ops(zus, acot[0], acot[1:], b1)}
                close = (mids["gaot_mlp2_jet2_cot_mid"]() - mids["tensor operations"]()).abs().max().item()
                mt, mp = {n: [] for n in mids}, {n: 0 for n in mids}
                for _ in range(reps):
                    for n, f in mids.items():
                        t, p, _o = timed(f); mt[n].append(t); mp[n] = max(mp[n], p); del _o
                km = median(mt["gaot_mlp2_jet2_cot_mid"])
                print(f"Nq={nq} {tag}: (f) nd={nd}: the middle on [{mr}, {hid}] planes ({3 * npl * mr * hid * 4 / 2**20:.0f} MiB read and "
                      f"written); max |kernel - tensor operations| = {close:.2e}")
                for n in mids:
                    m, lo, hi = median(mt[n])
                    print(f"Nq={nq} {tag}: (f) nd={nd} {n:24s} {m:9.3f} ms (max - min {hi - lo:.3f} ms), peak {mp[n] / 2**20:8.1f} MiB; "
                          f"this : gaot_mlp2_jet2_cot_mid = {m / km[0]:.2f}", flush=True)
                del zus, acot
        del q, v, v1, gy, gj, gl, g1, g2, g11, g21, gh, qc
elif what == "projection_jvp":
    # The projection MLP's forward-mode tangent on its own (LinearChannelMLP 32 -> 256 -> out, out in {1, 4}, three tangent planes, fp32
    # mode, random rows), as MAGNODecoder.sample_jacobian calls it: SAMPLE_CHUNK rows at a time into preallocated pred [N, out] and
    # jac [N, out, 3] through ``out=``.
    #   (a) jvp_rows(fused=False): the chain of gaot_gemm / gaot_act_bwd launches with the hidden tensors in memory;
    #   (b) jvp_rows(fused=True): one gaot_mlp2_jvp launch per chunk, the hidden layer in registers.
    # (a) and (b) alternate in this one process after a warm-up of each; device events around synchronised work; a window is `inner`
    # passes over all rows (10 at 500 K rows, 1 at 8 M) and the figures are per pass; `reps` windows; a row is the median with min / max,
    # the peak is the rise of allocated memory over the operands and the results.  Kept in profiles/projection_jvp_microbench.txt.
    from gaot_3d_amd.model.layers.magno import MAGNODecoder
    from gaot_3d_amd.model.layers.mlp import LinearChannelMLP
    gaot_3d_amd.set_precision("fp32")
    step = MAGNODecoder.SAMPLE_CHUNK

    def timed(fn, inner):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner, torch.cuda.max_memory_allocated() - base

    def median(ts):
        ts = sorted(ts)
        return ts[len(ts) // 2], ts[0], ts[-1]

    for oc in (1, 4):
        mlp = LinearChannelMLP([32, 256, oc]).to(dev).eval()
        for n in (500000, 8000000):
            inner = 10 if n <= 1000000 else 1
            x = torch.randn(n, 32, device=dev)
            dxs = [torch.randn(n, 32, device=dev) for _ in range(3)]
            pred, jac = torch.empty(n, oc, device=dev), torch.empty(n, oc, 3, device=dev)

            def run(fused):
                for i in range(0, n, step):
                    mlp.jvp_rows(x[i:i + step], [d[i:i + step] for d in dxs], fused=fused, out=(pred[i:i + step], jac[i:i + step]))
            timed(lambda: run(False), 1)                        # warm-up, and the two agree
            pc, jc = pred.clone(), jac.clone()
            timed(lambda: run(True), 1)
            same = torch.equal(pred, pc)
            dj = (jac - jc).abs().max().item() / jc.abs().max().item()
            del pc, jc
            ta, tb, pa, pb = [], [], 0, 0
            for _ in range(reps):
                t, p = timed(lambda: run(False), inner); ta.append(t); pa = max(pa, p)
                t, p = timed(lambda: run(True), inner); tb.append(t); pb = max(pb, p)
            (ma, lo_a, hi_a), (mb, lo_b, hi_b) = median(ta), median(tb)
            spread = max(hi_a - lo_a, hi_b - lo_b)
            print(f"N={n} out={oc} fp32: (a) jvp_rows(fused=False), chunk {step} {ma:9.3f} ms (min {lo_a:.3f}, max {hi_a:.3f}, spread "
                  f"{100 * (hi_a - lo_a) / ma:.1f} %), peak {pa / 2**20:9.1f} MiB")
            print(f"N={n} out={oc} fp32: (b) jvp_rows(fused=True),  chunk {step} {mb:9.3f} ms (min {lo_b:.3f}, max {hi_b:.3f}, spread "
                  f"{100 * (hi_b - lo_b) / mb:.1f} %), peak {pb / 2**20:9.1f} MiB  = {mb / ma:.3f} x (a) in time; (a) - (b) = {ma - mb:.3f} ms "
                  f"against a spread of {spread:.3f} ms; (b) faster beyond the spread: {ma - mb > spread}; y_a == y_b bit for bit: {same}, "
                  f"max|jac_a - jac_b| / peak = {dj:.1e}", flush=True)
            del x, dxs, pred, jac
elif what == "projection_bwd_f32":
    # The projection MLP's backward on its own (32 -> 256 -> out, out in {1, 4}, fp32 mode, random rows and cotangent), as
    # MAGNODecoder.sample_vjp_params calls it on one chunk: d_x, d_W1, d_b1, d_W2 and d_b2.
    #   (a) the GEMM chain (MAGNODecoder._project_bwd(fused=False)): gaot_gemm / gaot_act_bwd / gaot_colsum launches in row blocks with the
    #       [rows, hidden] tensors in memory;
    #   (b) one gaot_mlp2_bwd_f32 launch and its fixed-order completion (ops.mlp2_backward_f32), d_b2 by gaot_colsum.
    # (a) and (b) alternate in this one process after a warm-up of each; device events around synchronised work; `reps` rounds (7 for the
    # kept output); a row is the median with max - min, the peak is the rise of allocated memory over the operands.  Kept in
    # profiles/projection_bwd_f32_microbench.txt.
    from gaot_3d_amd.model.layers.magno import MAGNOConfig, MAGNODecoder
    gaot_3d_amd.set_precision("fp32")

    def timed(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - base, out

    def median(ts):
        ts = sorted(ts)
        return ts[len(ts) // 2], ts[0], ts[-1]

    for oc in (1, 4):
        cfg = MAGNOConfig(gno_coord_dim=3, lifting_channels=32, mlp_type="linear", use_geoembed=[True, False], neighbor_strategy="knn",
                          k_neighbors=8, out_gno_channel_mlp_hidden_layers=[64, 64], precompute_edges=False)
        dec = MAGNODecoder(in_channels=32, out_channels=oc, gno_config=cfg).to(dev).eval()
        for n in (1 << 20, 8000000):
            x, g = torch.randn(n, 32, device=dev), torch.randn(n, oc, device=dev)

            def run(fused):
                got = {id(p): torch.zeros_like(p) for p in dec.projection.parameters()}      # sample_vjp_params' accumulators
                with torch.no_grad(), ops.fp32_arithmetic():
                    dx = dec._project_bwd(x, g, lambda p, t: got[id(p)].add_(t.reshape(p.shape)), fused=fused)
                return [dx] + [got[id(p)] for p in dec.projection.parameters()]
            ra, rb = timed(lambda: run(False))[2], timed(lambda: run(True))[2]
            err = max(((a - b).abs().max() / a.abs().max()).item() for a, b in zip(ra, rb))
            del ra, rb
            ta, tb, pa, pb = [], [], 0, 0
            for _ in range(reps):
                t, p, _o = timed(lambda: run(False)); ta.append(t); pa = max(pa, p); del _o
                t, p, _o = timed(lambda: run(True)); tb.append(t); pb = max(pb, p); del _o
            (ma, lo_a, hi_a), (mb, lo_b, hi_b) = median(ta), median(tb)
            spread = max(hi_a - lo_a, hi_b - lo_b)
            print(f"N={n} out={oc} fp32: (a) the GEMM chain        {ma:9.3f} ms (max - min {hi_a - lo_a:.3f} ms), peak {pa / 2**20:9.1f} MiB")
            print(f"N={n} out={oc} fp32: (b) gaot_mlp2_bwd_f32     {mb:9.3f} ms (max - min {hi_b - lo_b:.3f} ms), peak {pb / 2**20:9.1f} MiB  = {mb / ma:.3f} x (a) "
                  f"in time; (a) - (b) = {ma - mb:.3f} ms against max - min {spread:.3f} ms of the rounds; (b) faster beyond it: {ma - mb > spread}; "
                  f"max |(a) - (b)| / peak over the five results = {err:.1e}", flush=True)
            del x, g
elif what == "decoder_param_adjoint":
    # The streamed gradients of the latent AND the decoder's parameters (MAGNODecoder.sample_vjp_params) on decoder_adjoint's decoders --
    # configs[1] (knn, k = 8), or with `--strategy bidirectional|radius` the reference YAML's decoder on row lists -- at 500 K and 8 M random
    # query points with a random cotangent, fp32 mode.  In this one process, alternated round by round after a warm-up of each:
    #   (a) sample_vjp_params, streamed in chunks;
    #   (b) the only other route to these gradients: the general decoder on an edge list for ALL queries under autograd (what
    #       forward(query_coord_pos=..) runs), then torch.autograd.grad of <cotangent, pred> to the latent and the decoder's parameters;
    #   (c) sample_vjp (the latent alone): what the parameters cost;
    #   (d) the split of (a) by the library's timing keys (device events around every launch group, one more pass).
    # Device events around synchronised work; `reps` rounds (7 for the kept output); a row is the median with max - min, the peak is the
    # rise of allocated memory over the inputs.  Kept in profiles/decoder_param_adjoint_microbench.txt.
    from gaot_3d_amd.data import latent_grid
    from gaot_3d_amd.model.layers.magno import MAGNOConfig, MAGNODecoder
    gaot_3d_amd.set_precision("fp32")
    latent = (64, 64, 32)
    strategy = sys.argv[sys.argv.index("--strategy") + 1] if "--strategy" in sys.argv else "knn"
    if strategy not in ("knn", "radius", "bidirectional"):
        sys.exit(f"--strategy must be knn, radius or bidirectional, got {strategy}")
    rows = strategy != "knn"
    cfg = MAGNOConfig(gno_coord_dim=3, lifting_channels=32, mlp_type="linear", use_geoembed=[True, False],
                      neighbor_strategy=["knn", strategy] if rows else "knn", k_neighbors=1 if rows else 8, gno_radius=0.033,
                      out_gno_channel_mlp_hidden_layers=[64, 64], precompute_edges=False)
    dec = MAGNODecoder(in_channels=32, out_channels=1, gno_config=cfg).to(dev).eval()
    dec.latent_dims = latent
    tokens = latent_grid(latent).to(dev)
    m_tok = tokens.shape[0]
    rn = torch.randn(m_tok, 32, device=dev)
    chunk = int(os.environ["MB_CHUNK"]) if os.environ.get("MB_CHUNK") else None
    tag = f"fp32{' ' + strategy if rows else ''}"
    names = [n for n, _ in dec.named_parameters()]

    def timed(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - base, out

    def median(ts):
        ts = sorted(ts)
        return ts[len(ts) // 2], ts[0], ts[-1]

    def replaced(q, g):
        leaf = rn.detach().clone().requires_grad_(True)
        zq = torch.zeros(q.shape[0], dtype=torch.long, device=dev)
        zl = torch.zeros(m_tok, dtype=torch.long, device=dev)
        pred = dec._decode(leaf, q, zq, tokens, zl, None, False)
        gl, *gp = torch.autograd.grad((pred * g).sum(), [leaf] + [p for _, p in dec.named_parameters()])
        return gl, dict(zip(names, gp))

    for nq in (500000, 8000000):
        q = torch.rand(nq, 3, device=dev) * 2 - 1
        g = torch.randn(nq, 1, device=dev)
        routes = {"(a) sample_vjp_params": lambda: dec.sample_vjp_params(rn, q, g, tokens, chunk_points=chunk),
                  "(b) decoder on an edge list + autograd.grad": lambda: replaced(q, g),
                  "(c) sample_vjp (the latent alone)": lambda: dec.sample_vjp(rn, q, g, tokens, chunk_points=chunk)}
        warm = {n: timed(f)[2] for n, f in routes.items()}
        (al, ap), (bl, bp) = warm["(a) sample_vjp_params"], warm["(b) decoder on an edge list + autograd.grad"]
        err = max([((al - bl).abs().max() / bl.abs().max()).item()] + [((ap[n] - bp[n]).abs().max() / bp[n].abs().max()).item() for n in names])
        del warm, al, ap, bl, bp
        ts, pk = {n: [] for n in routes}, {n: 0 for n in routes}
        for _ in range(reps):
            for n, f in routes.items():
                t, p, _o = timed(f); ts[n].append(t); pk[n] = max(pk[n], p); del _o
        med = {n: median(ts[n]) for n in routes}
        for n in routes:
            m, lo, hi = med[n]
            print(f"Nq={nq} {tag}: {n:45s} {m:9.3f} ms (max - min {hi - lo:.3f} ms = {100 * (hi - lo) / m:.1f} %), peak {pk[n] / 2**20:9.1f} MiB")
        ka, kb, kc = list(routes)
        print(f"Nq={nq} {tag}: (a) : (b) = {med[ka][0] / med[kb][0]:.2f} in time, {pk[ka] / max(pk[kb], 1):.3f} in peak memory "
              f"((a) {'below' if pk[ka] < pk[kb] else 'NOT below'} (b)); (a) : (c) = {med[ka][0] / med[kc][0]:.2f} in time, "
              f"{pk[ka] / max(pk[kc], 1):.2f} in peak memory; worst max |(a) - (b)| / max |(b)| over the latent and {len(names)} parameters = {err:.2e}")
        ops.timing_reset(True)
        dec.sample_vjp_params(rn, q, g, tokens, chunk_points=chunk)
        torch.cuda.synchronize()
        split = ops.timing_summary()
        ops.timing_reset(False)
        tot = sum(ms for _, ms in split.values())
        for key, (calls, ms) in sorted(split.items(), key=lambda kv: -kv[1][1]):
            print(f"Nq={nq} {tag}: (d) {key:24s} {calls:3d} calls {ms:9.3f} ms = {100 * ms / tot:5.1f} % of the timed launches' sum {tot:.3f} ms")
        sys.stdout.flush()
        del q, g
