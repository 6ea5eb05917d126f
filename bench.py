#!/usr/bin/env python3
"""bench.py -- mesh-points/sec of one GAOT-3D training step (zero_grad, forward, MSE, backward, AdamW step)
on ONE synthetic DrivAerNet++-shaped sample (BASELINE.json configs[1]: 500K points, latent 64x64x32, knn k=8
encoder + flipped decoder, model section of the reference's pressure.yaml: C=32, P=2, d=256, h=8, F=1024, L=10, rope).

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]

A plain run sets up, warms up, times the K steps and prints the line (`ms_per_step` = wall time of the timed region / K).
Everything else -- the secondary timings, the HBM copy peak, per-kernel HIP-event timings and the roofline figures built
on them, the CPU baseline, at N>1 the exchange profiles and the overlap_dw A/B -- runs only with ``--full``.
``--dump-outputs DIR``: after the timed steps, what the last one computed is written as float32 ``DIR/<name>.npy``
(loss, predictions, the updated parameters and their gradients; a fixed, seeded sample of an array above its cap).

N>1 from a plain shell: this process does NOT touch the GPU; it starts ``python -m torch.distributed.run --nnodes=1
--nproc-per-node N --master-addr 127.0.0.1 ...`` as a fresh child (one rank per GPU over RCCL), relays the child's
single JSON line and exits with its return code.  Under torchrun (WORLD_SIZE set) it is a rank.

N>1 is STRONG scaling by default (BASELINE.json configs[2]): the ONE 500K-point sample is split over the N GPUs --
physical points / edges by contiguous range, the latent Transformer by token rows, attention by heads (all-to-all on
either side), RCCL all-reduce of the encoder's per-token sums into the replicated latent grid; value = points of the
sample / step time.  ``--scaling weak`` keeps 500K points per GPU (an N x 500K-point sample) and says so in `metric`.
Rank 0 prints ONE JSON line.  The timed region starts with all inputs resident in HBM; the neighbour-list (CSR) build
and the geometric-embedding statistics are recomputed inside every timed step (nothing is cached across steps).
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", choices=["cfg1", "cfg3", "cfg4", "yaml"], default="cfg1",
                    help="cfg1 (default, the metric's configuration): BASELINE configs[1]/[2], 500K points, knn k=8 + flipped "
                         "decoder graph; cfg3: configs[3] shape -- radius-graph encoder (r=0.033, <=32 points per token) + "
                         "bidirectional decoder, statistical GeoEmbed on both sides, pos + [Mach, AOA] inputs; yaml: the graph "
                         "of the reference's config/examples/drivaernet/pressure.yaml (bidirectional both ways, r=0.033, k=1); "
                         "cfg4: configs[4] shape -- 8M points, 4 output fields, knn k=8.  Graphs are built once, outside the "
                         "timed step (precompute_edges=True as in the reference); their CSR forms inside it")
    ap.add_argument("--points", type=int, default=None, help="default 500000 (cfg4: 8000000)")
    ap.add_argument("--point-order", choices=["random", "morton"], default="random",
                    help="storage order of the synthetic points: the draw's (no locality, the worst case for the GNO gathers; "
                         "default) or along the Z-order curve (data.morton_order: what io.enrich_sample(reorder='morton') stores)")
    ap.add_argument("--latent", type=str, default="64,64,32")
    ap.add_argument("--layers", type=int, default=10)
    ap.add_argument("--knn", type=int, default=8)
    ap.add_argument("--precision", type=str, default=os.environ.get("GAOT_PRECISION", "bf16"), choices=["fp32", "bf16"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-baseline", choices=["auto", "sample", "full"], default="auto",
                    help="sample: the oracle on 1/8 of the points and of the latent grid (bounded, ~15 s); full: the oracle "
                         "on the SAME 500K-point sample, one timed step, attention dropout off on the CPU side (its mask "
                         "would be 8.6 GB per layer); auto (default): the bounded sample first, then the full sample as the "
                         "reported value when the host has the memory (>= 110 GB free) and the extrapolated time fits "
                         "--cpu-baseline-budget")
    ap.add_argument("--cpu-baseline-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--cpu-baseline-all-cores", action="store_true",
                    help="also time ONE step of the bounded CPU sample on os.cpu_count() threads (measured on the pool's 256-thread "
                         "hosts: 214 s against 5.1 s on 16 threads, the full sample 253.8 s against 28.3 s on 64 -- which is why it is "
                         "not part of the default run)")
    ap.add_argument("--cpu-baseline-dropout", action="store_true",
                    help="full-sample CPU step WITH attention dropout (torch's CPU SDPA then takes its written-out path: minutes "
                         "per step and ~90 GB at S = 16 384); default: dropout off on the CPU side, its best case")
    ap.add_argument("--cpu-baseline-budget", type=float, default=420.0,
                    help="auto: seconds the full-sample CPU step may be expected to take (extrapolated from the bounded sample)")
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel eagerly instead of replaying a hipGraph")
    ap.add_argument("--graph", action="store_true",
                    help="N>1: ALSO try capture + replay of the WHOLE step, RCCL collectives included, under a watchdog "
                         "(default at N>1: eager launches are timed first, then the SEGMENTED replay -- hipGraph segments "
                         "between eagerly issued collectives, gaot_3d_amd/comm.py -- which captures no collective)")
    ap.add_argument("--no-segmented", action="store_true", help="N>1: eager launches only")
    ap.add_argument("--no-overlap-dw", action="store_true",
                    help="N>1: skip the A/B of the weight-gradient side stream (ShardedStep(overlap_dw=True))")
    ap.add_argument("--overlap-dw-timeout", type=float, default=240.0,
                    help="N>1: seconds the overlap_dw A/B may take before the already measured line is printed and the ranks leave")
    ap.add_argument("--graph-attempt-timeout", type=float, default=150.0,
                    help="N>1 with --graph: seconds the guarded whole-step capture + replay may take; on a timeout the "
                         "already measured result is printed and the process exits with status 3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--atten-dropout", type=float, default=0.1,
                    help="attention dropout of the training step (reference default AttentionConfig.atten_dropout = 0.1, "
                         "attn.py:22; no shipped config overrides it)")
    ap.add_argument("--no-secondary", action="store_true",
                    help="skip the secondary timings (N=1: dropout-free step, fp32 mode; N>1: weak scaling)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="strong",
                    help="N>1: strong = ONE --points sample split over the N GPUs (BASELINE configs[2], default); weak = "
                         "every GPU owns --points points of one N x --points sample")
    ap.add_argument("--parallel", choices=["seq", "head", "replicated"], default="seq",
                    help="N>1, how the latent Transformer is divided: seq = token rows per rank + heads per rank inside "
                         "attention (all-to-all); head = replicated except the attention heads; replicated = not at all")
    ap.add_argument("--dry-run", action="store_true",
                    help="exercise launch + rendezvous only (gloo, no GPU work): prints a JSON line with n_ranks_seen")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: secondary timings (--no-secondary), HBM copy peak, "
                         "per-kernel timings and roofline figures, CPU baseline (--no-cpu-baseline); N>1: exchange profiles, "
                         "the overlap_dw A/B.  Default: set up, warm up, time --steps steps, print the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as float32 DIR/<name>.npy: loss, pred "
                         "(N=1), params and grads (after the optimizer step); above DUMP_CAP elements a fixed, seeded sample")
    return ap.parse_args(argv)


def spawn_command(args, argv, port):
    """the torchrun command line a plain `python bench.py --gpus N` (N>1) starts as its child"""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawn_ranks(args, argv):
    """Called BEFORE torch is imported / any HIP call: run the N ranks as a fresh child process tree, relay the JSON line."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // max(args.gpus, 1))))
    cmd = spawn_command(args, argv, _free_port())
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in r.stdout.splitlines():
        s = ln.strip()
        if s.startswith("{") and '"metric"' in s:
            line = s
        elif s:
            print(ln, file=sys.stderr)
    if line is not None:
        print(line)
    sys.stdout.flush()
    return r.returncode if (r.returncode != 0 or line is not None) else 1


WORKLOADS = {
    # name: (encoder strategy, decoder strategy, k, geoembed [enc, dec], input channels, output channels, default points)
    "cfg1": ("knn", "knn-flip", None, [True, False], 6, 1, 500000),
    "cfg3": ("radius", "bidirectional", 1, [True, True], 5, 1, 500000),
    "yaml": ("bidirectional", "bidirectional", 1, [True, False], 6, 1, 500000),
    "cfg4": ("knn", "knn-flip", None, [True, False], 6, 4, 8000000),
}


def model_config(latent, layers, k, atten_dropout=0.1, workload="cfg1"):
    from gaot_3d_amd.model.layers.attn import AttentionConfig, FFNConfig, TransformerConfig
    from gaot_3d_amd.model.layers.magno import MAGNOConfig
    enc_s, dec_s, kk, geo, _, _, _ = WORKLOADS[workload]
    strategy = "knn" if enc_s == "knn" else [enc_s, dec_s]
    return types.SimpleNamespace(
        magno=MAGNOConfig(use_gno=True, gno_coord_dim=3, neighbor_strategy=strategy, k_neighbors=kk or k, projection_channels=256,
                          in_gno_channel_mlp_hidden_layers=[64, 64, 64], out_gno_channel_mlp_hidden_layers=[64, 64],
                          lifting_channels=32, gno_radius=0.033, use_geoembed=list(geo),
                          embedding_method="statistical", encoder_feature_attr=["pos", "c"], mlp_type="linear",
                          precompute_edges=True),
        transformer=TransformerConfig(patch_size=2, hidden_size=256, use_attn_norm=True, use_ffn_norm=True, norm_eps=1e-6,
                                      num_layers=layers, positional_embedding="rope", use_long_range_skip=True,
                                      attn_config=AttentionConfig(hidden_size=256, num_heads=8, num_kv_heads=8,
                                                                  atten_dropout=atten_dropout),
                                      ffn_config=FFNConfig(hidden_size=1024)),
        latent_tokens=tuple(latent))


def make_workload_sample(workload, n_points, latent, k, seed, device, order="random"):
    """(batch, tokens) of a single-GPU workload: the synthetic surface sample with the workload's graphs as PRECOMPUTED edge
    lists (the reference's precompute_edges=True contract, stat.py:163-214), built once on the device by
    get_neighbor_strategy (csrc/graph.hip)"""
    import torch
    from gaot_3d_amd.data import make_synthetic_sample
    enc_s, dec_s, kk, _, cin, cout, _ = WORKLOADS[workload]
    batch, tokens = make_synthetic_sample(n_points, latent, k=k, seed=seed, device=device, out_channels=cout, order=order)
    tokens = tokens.to(device)
    if cin == 5:     # NASA CRM: pos + [Mach, AOA] broadcast per point (metadata.py:60-76)
        batch.c = torch.tensor([[0.85, 2.5]], device=device).expand(n_points, 2).contiguous()
    if enc_s != "knn":
        from gaot_3d_amd.model.layers.magno import get_neighbor_strategy
        lat_b = torch.zeros(tokens.shape[0], dtype=torch.long, device=device)
        enc = get_neighbor_strategy(enc_s, batch.pos, batch.batch, tokens, lat_b, 0.033, kk, False, latent_dims=tuple(latent))
        dec = get_neighbor_strategy(dec_s, batch.pos, batch.batch, tokens, lat_b, 0.033, kk, True, latent_dims=tuple(latent))
        batch.encoder_edge_index_s0 = enc.to(torch.int32).contiguous()
        batch.decoder_edge_index_s0 = dec.to(torch.int32).contiguous()
    return batch, tokens


def algorithmic_work(n_pts, m_lat, e_enc, e_dec, s_tok, layers, heads=8, dh=32, c=32, b=4):
    """Per-launch algorithmic flops / bytes of the instrumented kernels (SURVEY §8d per-unit figures)."""
    att = 2 * s_tok * s_tok * dh * heads  # one S x S x dh product over all heads
    return {
        "attn_fwd": dict(flops=2 * att, bytes=None, bound="mfma"),
        "attn_bwd": dict(flops=4 * att, bytes=None, bound="mfma"),       # fused backward: dP, dV, dK, dQ (S recompute not counted)
        "attn_bwd_fused_f32": dict(flops=4 * att, bytes=None, bound="mfma"),   # fp32 mode, one pass: dP, dV, dK, dQ (S recompute not counted; the slab reduction launched behind it is inside the timed span)
        "attn_bwd_dkv": dict(flops=3 * att, bytes=None, bound="mfma"),   # dP, dV, dK (S recompute not counted)
        "attn_bwd_dq": dict(flops=1 * att, bytes=None, bound="mfma"),    # dQ (S, dP recompute not counted)
        "gno_fwd_nh3": dict(flops=e_enc * 21280, bytes=e_enc * (32 + c * b) + m_lat * c * b, bound="hbm"),
        "gno_fwd_nh2": dict(flops=e_dec * 13088, bytes=e_dec * (32 + c * b) + n_pts * c * b, bound="hbm"),
        "gno_bwd_nh3": dict(flops=3 * e_enc * 21280, bytes=e_enc * (32 + 2 * c * b) + n_pts * c * b, bound="hbm"),
        "gno_bwd_nh2": dict(flops=3 * e_dec * 13088, bytes=e_dec * (32 + 2 * c * b) + m_lat * c * b, bound="hbm"),
    }


def dump_graph_structure(graph, path):
    """diagnostic (GAOT_BENCH_GRAPH_DOT): node types and the nodes whose in / out degree is not 1, through the HIP graph API"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    g = C.c_void_p(graph.raw_cuda_graph())
    n = C.c_size_t(0)
    hip.hipGraphGetNodes(g, None, C.byref(n))
    nodes = (C.c_void_p * n.value)()
    hip.hipGraphGetNodes(g, nodes, C.byref(n))
    ne = C.c_size_t(0)
    hip.hipGraphGetEdges(g, None, None, C.byref(ne))
    fr, to = (C.c_void_p * ne.value)(), (C.c_void_p * ne.value)()
    hip.hipGraphGetEdges(g, fr, to, C.byref(ne))
    idx = {nodes[i]: i for i in range(n.value)}
    types = []
    for i in range(n.value):
        t = C.c_int(-1)
        hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(t))
        types.append(t.value)
    indeg, outdeg = [0] * n.value, [0] * n.value
    edges = []
    for i in range(ne.value):
        a, b = idx[fr[i]], idx[to[i]]
        outdeg[a] += 1; indeg[b] += 1
        edges.append((a, b))
    import collections
    with open(path, "w") as f:
        f.write(f"nodes {n.value} edges {ne.value} types {dict(collections.Counter(types))}\n")
        f.write(f"indegree histogram {dict(collections.Counter(indeg))} outdegree histogram {dict(collections.Counter(outdeg))}\n")
        for i in range(n.value):
            if indeg[i] != 1 or outdeg[i] != 1 or types[i] != 0:
                f.write(f"node {i} type {types[i]} in {indeg[i]} out {outdeg[i]}\n")
        f.write("non-consecutive edges: " + " ".join(f"{a}->{b}" for a, b in edges if b != a + 1) + "\n")
    graph.instantiate()


def graph_node_counts(graph):
    """node census of a captured step through the HIP graph API (the graph must have been created with keep_graph=True and not
    yet be instantiated): every kernel node -- ours AND whatever ATen / the runtime put there -- plus memcpy / memset nodes"""
    import ctypes as C
    import collections
    hip = C.CDLL("libamdhip64.so")
    g = C.c_void_p(graph.raw_cuda_graph())
    n = C.c_size_t(0)
    if hip.hipGraphGetNodes(g, None, C.byref(n)) != 0:
        return None
    nodes = (C.c_void_p * n.value)()
    hip.hipGraphGetNodes(g, nodes, C.byref(n))
    names = {0: "kernel", 1: "memcpy", 2: "memset", 3: "host", 4: "child_graph", 5: "empty", 6: "wait_event", 7: "event_record"}
    cnt = collections.Counter()
    for i in range(n.value):
        t = C.c_int(-1)
        hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(t))
        cnt[names.get(t.value, f"type{t.value}")] += 1
    out = dict(cnt)
    out["total"] = n.value
    return out


def step_roofline_ms(n_pts, m_lat, e_enc, e_dec, s_tok, layers, precision, d=256, f=1024, c=32, out=1):
    """t_roof = sum over stages of max(bytes / HBM rate, flops / matrix rate of the arithmetic used).
    Transformer per layer forward 8 S d^2 + 4 S^2 d + 6 S d F (+ 4 S d^2 skip_proj in the decoder half), backward 2x;
    patch_linear 2 S d^2; GNO edge MLPs 21 280 / 13 088 flop per edge forward, 3x with backward; gather/scatter bytes
    per edge 32 + C b forward, 32 + 2 C b backward (+ one row written per output row); projection 16 896 flop per point."""
    mfma = 157.3e12 if precision == "fp32" else 2.5e15
    hbm = 8.0e12
    per_layer = 8 * s_tok * d * d + 4 * s_tok * s_tok * d + 6 * s_tok * d * f
    xf = layers * per_layer + (layers // 2) * 4 * s_tok * d * d + 2 * s_tok * d * d
    t_xf = 3 * xf / mfma
    gno_flops = 3 * (e_enc * 21280 + e_dec * 13088)
    gno_bytes = (e_enc * (32 + c * 4) + m_lat * c * 4 + e_dec * (32 + c * 4) + n_pts * c * 4
                 + e_enc * (32 + 2 * c * 4) + n_pts * c * 4 + e_dec * (32 + 2 * c * 4) + m_lat * c * 4)
    t_gno = max(gno_bytes / hbm, gno_flops / mfma)
    proj_flops = 3 * n_pts * 2 * (c * 256 + 256 * out)
    point_bytes = n_pts * (6 * 4 + c * 4 + 2 * out * 4) * 2 + m_lat * (9 * 4 + 3 * c * 4) * 2
    t_pt = max(point_bytes / hbm, proj_flops / mfma)
    t_opt = 28 * 11.25e6 / hbm      # AdamW: 28 B per parameter
    return dict(transformer_ms=t_xf * 1e3, gno_ms=t_gno * 1e3, per_node_ms=t_pt * 1e3, adamw_ms=t_opt * 1e3,
                t_roof_ms=(t_xf + t_gno + t_pt + t_opt) * 1e3)


def cpu_baseline(mode, layers, k, seed, atten_dropout, points, latent_full, cpu_dropout=False, all_cores_probe=False):
    """The oracle (CPU restatement of the reference, pure PyTorch fp32) timed on the host cores.  mode 'sample': a bounded
    sample of the same workload -- 1/8 of the points and 1/8 of the latent grid (so 1/8 of the tokens: attention, which is
    quadratic in them, is 1/64), same widths and depth; mode 'full': the same 500K-point sample the GPU step runs, one
    timed step after one warm-up, attention dropout off on the CPU side."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch
    import gaot_oracle as orc  # timed CPU baseline only
    from gaot_3d_amd.data import make_synthetic_sample
    from gaot_3d_amd.model import init_model
    if mode == "full":
        # dropout OFF on the CPU side unless --cpu-baseline-dropout: with dropout_p > 0 torch's CPU SDPA leaves its tiled kernel
        # for the written-out form ([S, S] weights, softmax, bernoulli_: measured x40 at S = 4 096 on 8 threads, 8.6 GB per layer
        # kept for the backward at S = 16 384), so the dropout-off step is the CPU's BEST case, stated in the line
        n, latent = points, tuple(latent_full)
        if not cpu_dropout:
            atten_dropout = 0.0
    else:
        n, latent = points // 8, (latent_full[0] // 2, latent_full[1] // 2, latent_full[2] // 2)
    # SURVEY 8d asks for the host's own cores.  MEASURED on the pool's 256-thread boxes: the full step on all 256 threads takes
    # 253.8 s against 28.3 s on 64 (profiles/archive/r5_j_bench_bf16_graph.json), the bounded step 214 s against 5.1 s on 16
    # (profiles/archive/r5_k_bench_default.json) -- the segmented reductions and the fp32 GEMMs of [16 384, 256] rows do not scale past a
    # socket's worth, oversubscribed they collapse.  So the full-sample step runs on at most 64 threads and never on more than the
    # process may keep busy (usable_cpus), the host's thread count and CPU model are named in the line, and
    # --cpu-baseline-all-cores repeats the all-cores measurement on request
    ncpu = os.cpu_count() or 1
    cores = min(usable_cpus(), 16 if mode == "sample" else 64)
    torch.set_num_threads(cores)
    cfg = model_config(latent, layers, k)
    torch.manual_seed(seed)
    model = init_model(6, 1, "gaot_3d", cfg)
    sd = {kk: v.clone() for kk, v in model.state_dict().items()}
    batch, tokens = make_synthetic_sample(n, latent, k=k, seed=seed)
    s_tok = latent[0] * latent[1] * latent[2] // 8

    def one_step():
        drop = None
        if atten_dropout > 0.0 and mode == "sample":   # explicit Bernoulli keep masks ([S, S] weights in memory: small S only)
            masks = [torch.empty(1, 8, s_tok, s_tok).bernoulli_(1.0 - atten_dropout) for _ in range(layers)]
            drop = (masks, atten_dropout)
        elif atten_dropout > 0.0:    # the reference's own training-mode call: SDPA draws its mask (attn.py:122-127)
            drop = ("torch", atten_dropout)
        orc.train_step_grads(sd, cfg, batch, tokens, drop=drop)

    times, tried = [], {}
    if mode == "sample":
        one_step()  # warm-up
        t_begin = time.perf_counter()
        while len(times) < 3 and time.perf_counter() - t_begin < 25.0:
            t0 = time.perf_counter()
            one_step()
            times.append(time.perf_counter() - t0)
        how = f"best of {len(times)} after 1 warm-up"
        t = min(times)
        tried[cores] = [round(v, 2) for v in times]
        if all_cores_probe and ncpu > cores:   # --cpu-baseline-all-cores: one more step of the bounded sample on every host thread
            torch.set_num_threads(ncpu)
            t0 = time.perf_counter()
            one_step()
            tried[ncpu] = [round(time.perf_counter() - t0, 2)]
            torch.set_num_threads(cores)
    else:           # one warm-up step, then up to three timed ones while a 75 s budget lasts (at least one): the median
        t0 = time.perf_counter()
        one_step()
        t_warm = time.perf_counter() - t0
        t_begin = time.perf_counter()
        while len(times) < 3 and (not times or time.perf_counter() - t_begin + t_warm < 75.0):
            t0 = time.perf_counter()
            one_step()
            times.append(time.perf_counter() - t0)
        t = statistics.median(times)
        tried[cores] = [round(v, 2) for v in times]
        how = f"median of {len(times)} after 1 warm-up on {cores} threads"
    frac = "the same sample as the GPU step" if mode == "full" else "1/8 of the points and 1/8 of the latent grid: a REDUCED sample"
    out = dict(value=n / t, unit="points/s", cores=cores, host_cpus=ncpu, cpu_model=cpu_model(), kind="port",
               reduced_sample=(mode != "full"), seconds_per_step=round(t, 2), timed_seconds=[round(v, 2) for v in times],
               sample=f"oracle fwd+MSE+bwd on N={n} points, latent {latent[0]}x{latent[1]}x{latent[2]} ({frac}), k={k}, "
                      f"L={layers}, d=256, attention dropout {atten_dropout}, fp32, {how} ({t:.2f} s/step)")
    if tried:
        out["seconds_by_threads"] = {str(kk): v for kk, v in tried.items()}
    return out


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.startswith("model name"):
                    return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline_auto(budget_s, layers, k, seed, atten_dropout, points, latent_full, cpu_dropout=False, all_cores_probe=False):
    """the bounded sample first; then, when the host can take it, ONE step on the metric's own 500K-point sample as the
    reported value (same input), the bounded figure kept beside it"""
    red = cpu_baseline("sample", layers, k, seed, atten_dropout, points, latent_full, all_cores_probe=all_cores_probe)
    # the bounded sample carries dropout masks (explicit attention weights), the full step runs without dropout through the
    # reference's own F.scaled_dot_product_attention (no [S, S] weights in memory): measured x5-x8 of the bounded step on 64 threads
    expect = 3.0 * 8.0 * red["seconds_per_step"]        # warm-up + up to two more steps
    try:
        import psutil
        free_gb = psutil.virtual_memory().available / 2 ** 30
    except Exception:
        free_gb = 0.0
    if free_gb < 48.0 or expect > budget_s:
        red["full_sample_skipped"] = (f"full 500K-point CPU step not run: {free_gb:.0f} GB free host memory (needs ~48), expected "
                                      f"{expect:.0f} s against a budget of {budget_s:.0f} s")
        return red
    # in a child process: if the kernel kills it for memory, the bench line survives with the bounded figure
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-child", "--layers", str(layers), "--knn", str(k), "--seed", str(seed),
           "--points", str(points), "--latent", ",".join(str(v) for v in latent_full), "--atten-dropout", str(atten_dropout)]
    if cpu_dropout:
        cmd.append("--cpu-baseline-dropout")
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=3.0 * budget_s + 120.0)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            raise RuntimeError(f"child exit code {r.returncode}: {r.stderr[-300:]}")
        full = json.loads(lines[-1])
    except Exception as ex:
        red["full_sample_skipped"] = f"full 500K-point CPU step failed ({type(ex).__name__}: {ex})"
        return red
    full["bounded_sample"] = {kk: red[kk] for kk in ("value", "cores", "seconds_per_step", "sample", "seconds_by_threads") if kk in red}
    return full


# keys of the result line that only a --full run fills in (their measurements take runs of their own)
FULL_ONLY_KEYS = ("kernel_launches_per_step", "foreign_kernel_nodes_per_step", "instrumented_eager_ms_per_step",
                  "instrumented_eager_host_ms_per_step", "without_attention_dropout", "geometry_cached", "hbm_copy_peak_measured",
                  "fp32_mode", "other_scaling", "roofline", "gno_hbm", "kernels")

# --dump-outputs: at most this many elements per array (13 Mi float32 = 52 MiB in all; loss is one element)
DUMP_CAP = {"pred": 3 << 20, "params": 5 << 20, "grads": 5 << 20}


def dump_outputs(out_dir, loss, pred, params):
    """what the step computed in its last run, as float32 .npy files: loss, pred (None: not written), and every parameter
    after the optimizer step with its gradient, flattened and concatenated in named_parameters() order.  An array above its
    DUMP_CAP is replaced by the elements at a fixed, seeded set of flat indices (the same set for params and grads).
    -> {name: shape written}"""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    params = list(params)
    arrays = {"loss": loss.detach().float().reshape(())}
    if pred is not None:
        arrays["pred"] = pred.detach().float()
    arrays["params"] = torch.cat([p.detach().float().reshape(-1) for p in params])
    arrays["grads"] = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().float().reshape(-1)
                                 for p in params])
    written = {}
    for name, t in arrays.items():
        cap = DUMP_CAP.get(name)
        if cap is not None and t.numel() > cap:
            idx = np.sort(np.random.default_rng(20261016).choice(t.numel(), size=cap, replace=False))
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        a = t.cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), a)
        written[name] = list(a.shape)
    return written


def usable_cpus():
    """CPUs this process may keep busy: os.cpu_count() counts the whole host, so cap it by the affinity mask, the cgroup CPU
    quota and OMP_NUM_THREADS when they are set"""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        pass
    try:
        omp = int(os.environ["OMP_NUM_THREADS"])
        if omp > 0:
            n = min(n, omp)
    except (KeyError, ValueError):
        pass
    return max(1, n)


def csrc_sha16():
    """hash of the kernel sources: profiles/pmc_traffic.json carries the hash of the sources it was measured on"""
    import glob
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "gaot_3d_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(d, "*.hip")) + glob.glob(os.path.join(d, "*.h")) + glob.glob(os.path.join(d, "*.inc"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def summarize_exchange_profiles(per_rank):
    """per_rank: one {"eager": ExchangeProfile.summary, "segmented": ...} per rank -> per mode MIN / MAX over the ranks of
    the step's device ms, of the part inside exchange steps and of the part inside kernels, plus per collective kind the
    count, the bytes per step and the MIN / MAX exposed device ms.  `grad_bucket_wait` is what the asynchronous bucketed
    weight-gradient all-reduce did NOT hide under the remaining backward."""
    out = {}
    for mode in ("eager", "segmented"):
        recs = [r.get(mode) for r in per_rank if isinstance(r, dict) and isinstance(r.get(mode), dict)]
        good = [r for r in recs if "error" not in r]
        if not good:
            if recs:
                out[mode] = dict(error=recs[0].get("error"))
            continue
        ent = {}
        for key in ("step_device_ms", "exchange_device_ms", "compute_device_ms"):
            vals = [r[key] for r in good]
            ent[key] = dict(min=round(min(vals), 4), max=round(max(vals), 4))
        kinds = {}
        for r in good:
            for kind, kv in r["kinds"].items():
                k = kinds.setdefault(kind, dict(count_per_step=kv["count"], bytes_per_step=kv["bytes"], device_ms=[]))
                k["device_ms"].append(kv["device_ms"])
        for kind, k in kinds.items():
            v = k.pop("device_ms")
            k["device_ms_min"], k["device_ms_max"] = round(min(v), 4), round(max(v), 4)
        ent["kinds"] = kinds
        ent["ranks"] = len(good)
        out[mode] = ent
    return out


def dry_run(args):
    """launch / rendezvous check without GPU work: every rank joins a gloo group and rank 0 prints the line"""
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    seen = 1
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="gloo", init_method="env://")
        t = torch.ones(1)
        dist.all_reduce(t)
        seen = int(t.item())
    if rank == 0:
        print(json.dumps({"metric": "dry-run (no GPU work)", "value": 0.0, "unit": "points/s", "n_gpus": world,
                          "n_ranks_seen": seen, "scaling": args.scaling, "dry_run": True}))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: start the ranks as a child BEFORE anything here touches the GPU
        sys.exit(spawn_ranks(args, argv))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.dry_run:
        return dry_run(args)
    if args.cpu_baseline_child:      # the full-sample CPU step of cpu_baseline_auto, in its own process (no GPU work)
        latent = tuple(int(v) for v in args.latent.split(","))
        print(json.dumps(cpu_baseline("full", args.layers, args.knn, args.seed, args.atten_dropout, args.points or 500000, latent,
                                      args.cpu_baseline_dropout)))
        return

    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # GAOT_BENCH_ONE_DEVICE=1 (testing only): every rank on cuda:0 over gloo, to exercise the N>1 code path -- sharding,
    # exchange steps, max-over-ranks timing -- on a single-GPU box.  The number it prints is not a scaling result.
    one_device = os.environ.get("GAOT_BENCH_ONE_DEVICE", "0") == "1"
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="gloo" if one_device else "nccl", init_method="env://")
    if one_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    import gaot_3d_amd
    from gaot_3d_amd import functional as GF
    from gaot_3d_amd import ops
    from gaot_3d_amd.data import make_synthetic_sample, make_synthetic_shard
    from gaot_3d_amd.model import init_model
    from gaot_3d_amd.optim import AdamW   # fused multi-tensor HIP step, same semantics as torch.optim.AdamW (tests)
    gaot_3d_amd.set_precision(args.precision)
    # deferred weight-gradient reductions are opt-in (ops.defer_ok): this step qualifies -- every parameter has one consumer, all of
    # them gaot operators, no hooks, no process group at N = 1 (with one initialised, defer_ok declines by itself)
    ops.defer_reductions(os.environ.get("GAOT_DEFER_REDUCE", "1") != "0")
    if args.points is None:
        args.points = WORKLOADS[args.workload][6]
    if world > 1 and args.workload not in ("cfg1", "cfg4"):
        raise SystemExit("--workload cfg3 / yaml are single-GPU lines (their graphs are built from the whole point set)")
    wl_in, wl_out = WORKLOADS[args.workload][4], WORKLOADS[args.workload][5]
    # tag of the measured-traffic file of this workload variant (tools/gpu_workloads.sh writes profiles/pmc_traffic_<tag>.json)
    wl_tag = args.workload
    if args.points != WORKLOADS[args.workload][6]:
        wl_tag += f"_{args.points // 1000000}m" if args.points % 1000000 == 0 else f"_{args.points}"
    if args.point_order != "random":
        wl_tag += f"_{args.point_order}"
    latent = tuple(int(v) for v in args.latent.split(","))
    m_lat = latent[0] * latent[1] * latent[2]
    s_tok = m_lat // 8

    geometry_cached = {"on": False}
    outputs = {}      # what the latest step returned beside its loss (N=1: the predictions)

    def build(n_total, atten_dropout, parallel):
        """model + optimizer + rank-local inputs + step() for one sample of n_total points"""
        cfg = model_config(latent, args.layers, args.knn, atten_dropout, args.workload)
        torch.manual_seed(args.seed)
        model = init_model(wl_in, wl_out, "gaot_3d", cfg).to(dev).train()
        opt = AdamW(model.parameters(), lr=3e-4, weight_decay=1e-5)
        if world > 1:
            from gaot_3d_amd import sharding
            # every rank generates only ITS point range on the device (host RNG draws are the whole sample's: 7 floats/point)
            batch, tokens = make_synthetic_shard(n_total, latent, rank, world, k=args.knn, seed=args.seed, device=str(dev),
                                                 out_channels=wl_out, order=args.point_order)
            step_ctx = sharding.ShardedStep(model, dist.group.WORLD, n_total, parallel=parallel, grad_group=grad_group)
        else:
            batch, tokens = make_workload_sample(args.workload, n_total, latent, args.knn, args.seed, str(dev), args.point_order)
            step_ctx = None
        tokens = tokens.to(dev)
        # edges of THIS rank's graphs (variable for the radius / bidirectional workloads)
        edges = dict(enc=int(batch.encoder_edge_index_s0.shape[1]), dec=int(batch.decoder_edge_index_s0.shape[1]))

        def step():
            if not geometry_cached["on"]:
                # CSR build and GeoEmbed statistics are per-sample constants (the reference precomputes its edges offline,
                # stat.py:126-224): the headline step rebuilds them every time, the `geometry_cached` figure serves them from
                # the per-sample cache on the batch
                gaot_3d_amd.clear_graph_cache(batch)
            opt.zero_grad(set_to_none=True)
            if step_ctx is None:
                pred = model(batch=batch, tokens_pos=tokens)
                outputs["pred"] = pred.detach()     # --dump-outputs (of a captured step: the graph's own output buffer)
                loss = GF.mse_loss(pred, batch.x)
                loss.backward()
                loss = loss.detach()    # nothing of the step's autograd graph outlives the step: a live AccumulateGrad node of
                                        # an eager step would drag its (default) stream into the next step's capture
            else:
                loss = step_ctx.forward_backward(batch, tokens)
            opt.step()
            return loss
        return model, step, edges, step_ctx

    # The step is a few hundred short kernels; launched eagerly from Python the host can become the bottleneck.  Capture
    # ONE whole step (CSR build, forward, loss, backward, gradient exchange, AdamW) into a hipGraph after the warm-up and
    # replay it: the timed region then measures the device work.  --no-graph times the eager launches instead.
    last_step_ms = []      # device ms of every timed step of the latest measure() call
    last_capture = {"error": None, "nodes": None}     # of the latest measure() call: why a capture failed / the node census

    def measure(step, steps, warmup, use_graph):
        graph = None
        loss = None
        last_capture["error"], last_capture["nodes"] = None, None
        if use_graph:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(max(warmup, 1)):
                    step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            outputs.clear()     # an eager step's tensors are released here, not inside the capture
            try:
                dot = os.environ.get("GAOT_BENCH_GRAPH_DOT")    # diagnostic: node / edge structure of the captured step
                graph = torch.cuda.CUDAGraph(keep_graph=True)
                # N>1: ProcessGroupNCCL's watchdog thread polls events of earlier collectives while this thread captures;
                # under the default "global" capture mode that query is an error that aborts the process
                with torch.cuda.graph(graph, capture_error_mode="global" if world == 1 else "thread_local"):
                    loss = step()
                try:
                    last_capture["nodes"] = graph_node_counts(graph)
                except Exception as ex:
                    last_capture["nodes"] = {"error": f"{type(ex).__name__}: {ex}"}
                if dot:
                    dump_graph_structure(graph, dot)        # instantiates
                else:
                    graph.instantiate()
            except Exception as ex:  # capture is a launch optimisation only; the eager launches are timed and the line SAYS so
                print(f"[bench] hipGraph capture failed ({type(ex).__name__}: {ex}); timing eager launches", file=sys.stderr)
                last_capture["error"] = f"{type(ex).__name__}: {str(ex)[:200]}"
                graph = None
                torch.cuda.synchronize()
        for _ in range(warmup):
            if graph is None:
                loss = step()
            else:
                graph.replay()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        # one HIP event per step boundary on the step's stream, inside the timed region (the MEDIAN of the timed steps is
        # reported beside the mean the contract's `ms_per_step` is)
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        t0 = time.perf_counter()
        marks[0].record()
        for i in range(steps):
            if graph is None:
                loss = step()
            else:
                graph.replay()
            marks[i + 1].record()
        t_host = time.perf_counter() - t0
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        if world > 1:
            tt = torch.tensor([elapsed], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            elapsed = tt.item()
        last_step_ms[:] = [marks[i].elapsed_time(marks[i + 1]) for i in range(steps)]
        return elapsed, graph, loss, t_host

    def measure_graph_guarded(step, steps, warmup, on_timeout, timeout_s):
        """N>1: capture + replay of the whole sharded step (RCCL collectives included).  This cannot be exercised on the
        one-GPU development boxes, so it runs under a watchdog: if capture or replay has not finished after timeout_s,
        rank 0 prints the (already measured) eager result and every rank leaves the process."""
        import threading
        done = threading.Event()

        def fire():
            if done.is_set():
                return
            try:
                on_timeout()
            finally:
                os._exit(3)     # the ranks are wedged in a capture / replay: not a clean run, say so
        timer = threading.Timer(timeout_s + (0.0 if rank == 0 else 15.0), fire)
        timer.daemon = True
        timer.start()
        try:
            e, g, l, th = measure(step, steps, warmup, True)
        except Exception as ex:
            done.set()
            timer.cancel()
            return None, f"{type(ex).__name__}: {ex}"
        done.set()
        timer.cancel()
        if g is None:
            return None, "capture failed (see stderr); eager launches timed instead"
        return (e, g, l, th), "ok"

    def record_segmented(step, sg, warmup):
        """N>1 default launch mode: the step recorded as hipGraph segments between eagerly issued exchange steps
        (gaot_3d_amd/comm.py).  No collective is captured, and the recording pass itself issues none."""
        for _ in range(max(warmup, 1)):
            step()                              # eager: lazy initialisation, co-located weights
        torch.cuda.synchronize()
        sg.capture(step)

    def time_segmented(sg, steps, warmup):
        """-> (elapsed, loss, host seconds of the timed region, host seconds of it spent inside the exchange closures)"""
        for _ in range(max(warmup, 1)):
            sg.replay()
        torch.cuda.synchronize()
        dist.barrier()
        torch.cuda.synchronize()
        sg.host_exchange_s = 0.0
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        t0 = time.perf_counter()
        marks[0].record(sg.stream)
        for i in range(steps):
            sg.replay(timed=True)
            marks[i + 1].record(sg.stream)
        t_host = time.perf_counter() - t0
        torch.cuda.synchronize()
        dist.barrier()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        tt = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        last_step_ms[:] = [marks[i].elapsed_time(marks[i + 1]) for i in range(steps)]
        return tt.item(), sg.result, t_host, sg.host_exchange_s

    n_total = args.points * world if args.scaling == "weak" else args.points
    use_graph = (not args.no_graph) and world == 1
    if world > 1:
        # eager steps, recording and replay of the sharded step all on ONE side stream: nothing of the step (autograd's
        # stream-bound gradient accumulators included) ever involves the default stream, which a capture cannot contain
        torch.cuda.set_stream(torch.cuda.Stream())
    # second process group over the same ranks: the bucketed weight-gradient all-reduce runs on its own RCCL stream
    grad_group = dist.new_group(backend="gloo" if one_device else "nccl") if world > 1 else None
    model, step, edge_counts, step_ctx = build(n_total, args.atten_dropout, args.parallel)
    elapsed, graph, loss, t_host_main = measure(step, args.steps, args.warmup, use_graph)
    main_step_ms = list(last_step_ms)
    main_capture = dict(last_capture)
    eager_rec = seg_rec = None
    exchange_profile = {}

    def sharded_modes(e_eager, loss_eager, th_eager, ms_eager, profile):
        """N > 1: given the timed EAGER step, add its exchange profile, then record + time + profile the SEGMENTED replay
        (profile=False: no exchange profiles, the two timings only)
        -> (eager record, segmented record, profiles, best = (elapsed, loss, host s, graph or None, per-step ms))"""
        from gaot_3d_amd import comm
        prof_out = {}
        e_rec = dict(ms_per_step=e_eager / args.steps * 1e3, value=n_total / (e_eager / args.steps),
                     host_ms_per_step=round(th_eager / args.steps * 1e3, 3))
        best = (e_eager, loss_eager, th_eager, None, list(ms_eager))
        # per-rank split of the EAGER step's device time first (no capture involved): exchange steps vs kernels
        if profile:
            try:
                k_prof = max(1, min(args.steps, 3))
                with comm.eager_profile() as prof:
                    for _ in range(k_prof):
                        step()
                torch.cuda.synchronize()
                prof_out["eager"] = prof.summary(k_prof)
            except Exception as ex:
                prof_out["eager"] = dict(error=f"{type(ex).__name__}: {ex}")
        sg = None
        seg_err = None
        try:
            sg = comm.SegmentedGraph()
            record_segmented(step, sg, args.warmup)
        except Exception as ex:
            seg_err = f"{type(ex).__name__}: {ex}"
            sg = None
            print(f"[bench] rank {rank}: segmented capture failed ({seg_err})", file=sys.stderr)
            torch.cuda.synchronize()
        # every rank must take the SAME branch: one rank replaying while another launches eagerly would pair different
        # collectives and hang.  MIN over the ranks' success flags decides.
        okf = torch.tensor([1.0 if sg is not None else 0.0], device=dev)
        dist.all_reduce(okf, op=dist.ReduceOp.MIN)
        if okf.item() >= 1.0:
            e_s, loss_s, th_s, tx_s = time_segmented(sg, args.steps, args.warmup)
            s_rec = dict(ms_per_step=e_s / args.steps * 1e3, value=n_total / (e_s / args.steps),
                         host_ms_per_step=round(th_s / args.steps * 1e3, 3),
                         host_ms_per_step_outside_exchange=round((th_s - tx_s) / args.steps * 1e3, 3),
                         graph_segments=sg.num_segments, exchanges=sg.num_exchanges,
                         host_launches_plus_collectives=sg.num_segments + sg.num_exchanges,
                         side_stream_closures=sum(len(v) for v in sg.side))
            if profile:
                try:
                    prof_out["segmented"] = sg.replay_profiled(max(1, min(args.steps, 3)))
                except Exception as ex:
                    prof_out["segmented"] = dict(error=f"{type(ex).__name__}: {ex}")
            if e_s < e_eager:
                best = (e_s, loss_s, th_s, sg, list(last_step_ms))
        else:
            s_rec = dict(error=seg_err or "the recording failed on another rank: every rank reports its eager launches")
        return e_rec, s_rec, prof_out, best

    if world > 1 and not args.no_graph and not args.no_segmented:
        eager_rec, seg_rec, exchange_profile, best = sharded_modes(elapsed, loss, t_host_main, main_step_ms, args.full)
        elapsed, loss, t_host_main, graph, main_step_ms = best

    if args.dump_outputs and rank == 0:
        # before anything else runs a step: at N>1 the last step run is the last timed one of the launch mode timed last
        written = dump_outputs(args.dump_outputs, loss, outputs.get("pred"), model.parameters())
        print(f"[bench] outputs of the last timed step written to {args.dump_outputs}: {written}", file=sys.stderr)

    secondary = None
    fp32_mode = None
    weak = None
    geom_cached = None
    copy_peak = None
    if world == 1 and args.full:
        try:
            copy_peak = round(ops.stream_copy_gbps(), 1)     # float4 copy, 1 GiB, read + written bytes / HIP-event time
        except Exception as ex:
            copy_peak = None
            print(f"[bench] stream copy failed ({type(ex).__name__}: {ex})", file=sys.stderr)
    if world == 1 and args.full and not args.no_secondary:
        # the same step with the per-sample constants (neighbour lists, GeoEmbed statistics) served from the cache on the
        # batch, as the reference's offline edge precompute does (stat.py:126-224); SURVEY 8d asks for both figures
        try:
            geometry_cached["on"] = True
            eg, gg, _, _ = measure(step, args.steps, args.warmup, use_graph)
            geom_cached = dict(ms_per_step=eg / args.steps * 1e3, value=n_total / (eg / args.steps),
                               note="CSR build + GeoEmbed statistics cached per sample (built once, outside the step)")
            del gg
        except Exception as ex:
            geom_cached = dict(error=f"{type(ex).__name__}: {ex}")
        finally:
            geometry_cached["on"] = False
        if args.atten_dropout > 0.0:
            # the same step with the dropout switched off (what the kernels do in eval mode / atten_dropout = 0)
            for mod in model.modules():
                if hasattr(mod, "atten_dropout"):
                    mod.atten_dropout = 0.0
            e2, g2, _, _ = measure(step, args.steps, args.warmup, use_graph)
            secondary = dict(ms_per_step=e2 / args.steps * 1e3, value=n_total / (e2 / args.steps), atten_dropout=0.0)
            del g2
            for mod in model.modules():
                if hasattr(mod, "atten_dropout"):
                    mod.atten_dropout = args.atten_dropout
        if args.precision != "fp32":
            # the reference's own arithmetic is fp32 end to end: the same step on the exact-fp32 MFMA kernels
            try:
                gaot_3d_amd.set_precision("fp32")
                k3 = max(2, min(args.steps, 10))
                e3, g3, _, _ = measure(step, k3, 1, use_graph)
                fp32_mode = dict(ms_per_step=e3 / k3 * 1e3, value=n_total / (e3 / k3), dtype="f32", steps=k3,
                                 ms_per_step_median=round(statistics.median(last_step_ms), 3) if last_step_ms else None,
                                 launch="hipGraph replay of one captured step" if g3 is not None else "eager")
                del g3
                # the reference's own arithmetic as a measured mode: HIP events around the instrumented launches of
                # two eager fp32 steps -> the dominant kernel against the fp32 matrix peak (157.3 TF/s, MI355X_MICROARCH.md)
                ops.timing_reset(True)
                for _ in range(2):
                    step()
                torch.cuda.synchronize()
                t32 = ops.timing_summary()
                ops.timing_reset(False)
                w32 = algorithmic_work(n_total // world, m_lat, edge_counts["enc"], edge_counts["dec"], s_tok, args.layers)
                k32 = {nm: dict(avg_ms=round(tot / c, 4), calls_per_step=c / 2, total_ms_per_step=round(tot / 2, 4),
                                tflops=round(w32[nm]["flops"] / (tot / c * 1e-3) / 1e12, 2)) for nm, (c, tot) in t32.items() if nm in w32 and c}
                if k32:
                    dom32 = max(k32, key=lambda nm: k32[nm]["total_ms_per_step"])
                    fp32_mode["roofline_fp32"] = dict(kernel=dom32, bound="mfma", achieved=k32[dom32]["tflops"], peak=157.3, unit="TFLOP/s",
                                                      frac=round(k32[dom32]["tflops"] / 157.3, 4), avg_ms=k32[dom32]["avg_ms"], traffic=None)
                    fp32_mode["kernels"] = k32
                    tr32 = step_roofline_ms(n_total // world, m_lat, edge_counts["enc"], edge_counts["dec"], s_tok, args.layers, "fp32", out=wl_out)
                    fp32_mode["step_roofline"] = dict(t_roof_ms=round(tr32["t_roof_ms"], 3), frac=round(tr32["t_roof_ms"] / fp32_mode["ms_per_step"], 4))
            except Exception as ex:
                fp32_mode = dict(error=f"{type(ex).__name__}: {ex}")
            finally:
                gaot_3d_amd.set_precision(args.precision)

    # per-kernel durations: HIP events around the instrumented launches of two more (eager) steps on the same stream
    timing, launches, t_host, t_eager, n_timed_steps = {}, None, None, None, 2
    if args.full:
        ops.timing_reset(True)
        ops.launch_count_reset()
        t_e = time.perf_counter()
        for _ in range(2):
            step()
        t_host = (time.perf_counter() - t_e) / 2
        torch.cuda.synchronize()
        t_eager = (time.perf_counter() - t_e) / 2
        timing = ops.timing_summary()
        launches = ops.launch_count() / n_timed_steps
        ops.timing_reset(False)

    if world > 1 and args.full and not args.no_secondary:
        other = "weak" if args.scaling == "strong" else "strong"
        try:
            n2 = args.points * world if other == "weak" else args.points
            model2, step2, _, _ = build(n2, args.atten_dropout, args.parallel)
            k2 = max(2, min(args.steps, 5))
            e2, _, _, _ = measure(step2, k2, 1, False)
            weak = dict(scaling=other, points=n2, ms_per_step=e2 / k2 * 1e3, value=n2 / (e2 / k2), steps=k2, launch="eager")
            del model2, step2
        except Exception as ex:
            weak = dict(scaling=other, error=f"{type(ex).__name__}: {ex}")

    def gno_hbm(per_kernel):
        """the gather / scatter kernels against the HBM roof: algorithmic GB/s (SURVEY 8d bytes per edge) / 8 TB/s, with the
        measured FETCH_SIZE / WRITE_SIZE bytes per launch when profiles/pmc_traffic*.json is from these sources + workload"""
        pj = {}
        try:
            name = "pmc_traffic.json" if wl_tag == "cfg1" else f"pmc_traffic_{wl_tag}.json"
            cand = json.load(open(os.path.join(ROOT, "profiles", name)))
            if cand.get("_source", {}).get("csrc_sha16") == csrc_sha16() and world == 1:
                pj = cand
        except Exception:
            pass
        sq_file = {}
        try:
            cand = json.load(open(os.path.join(ROOT, "profiles", "pmc_sq.json")))
            if cand.get("_source", {}).get("csrc_sha16") == csrc_sha16() and world == 1 and args.workload == "cfg1":
                sq_file = cand
        except Exception:
            pass
        out = {}
        for kname, ent in per_kernel.items():
            if not kname.startswith("gno_") or "gbps" not in ent:
                continue
            out[kname] = dict(avg_ms=round(ent["avg_ms"], 4), algorithmic_gbps=round(ent["gbps"], 1),
                              frac_of_8tbps=round(ent["gbps"] / 8000.0, 4),
                              measured_bytes_per_launch=pj.get(kname, {}).get("bytes_per_launch"))
            mb = out[kname]["measured_bytes_per_launch"]
            if mb:
                out[kname]["measured_gbps"] = round(mb / (ent["avg_ms"] * 1e-3) / 1e9, 1)
            dd = sq_file.get(kname, {}).get("derived") if kname != "_source" else None
            if dd:      # the roof the kernel actually sits under (SQ counters): these kernels are instruction-issue bound, not HBM bound
                out[kname]["issue_busy"] = dd.get("issue_busy")
                out[kname]["mfma_busy_counted"] = dd.get("mfma_busy_counted")
                out[kname]["bound_actual"] = ("instruction issue" if dd.get("issue_busy", 0.0) >= 0.6 and out[kname]["frac_of_8tbps"] < 0.4
                                              else "hbm")
        tot = sum(v["avg_ms"] for v in out.values())
        return dict(kernels=out, total_ms_per_step=round(tot, 4)) if out else None

    def make_out(elapsed, launch_txt, host_ms, step_ms=None):
        ms = elapsed / args.steps * 1e3
        e_enc, e_dec = edge_counts["enc"], edge_counts["dec"]      # this rank's edges
        work = algorithmic_work(n_total // world, m_lat, e_enc, e_dec, s_tok, args.layers,
                                heads=8 // world if (world > 1 and args.parallel != "replicated" and 8 % world == 0) else 8)
        peaks = {"mfma": (157.3 if args.precision == "fp32" else 2500.0, "TFLOP/s"), "hbm": (8000.0, "GB/s")}
        per_kernel = {}
        for name, (calls, tot_ms) in timing.items():
            if name not in work or calls == 0:
                continue
            avg_s = tot_ms / calls * 1e-3
            w = work[name]
            ent = dict(calls_per_step=calls / n_timed_steps, avg_ms=tot_ms / calls, total_ms_per_step=tot_ms / n_timed_steps,
                       tflops=w["flops"] / avg_s / 1e12)
            if w["bytes"]:
                ent["gbps"] = w["bytes"] / avg_s / 1e9
            ent["bound"] = w["bound"]
            per_kernel[name] = ent
        dom = max(per_kernel, key=lambda kname: per_kernel[kname]["total_ms_per_step"]) if per_kernel else None
        roof = None
        if dom:
            d = per_kernel[dom]
            # GNO kernels: layer 0 always runs on exact-fp32 MFMA, the other layers on the precision's matrix rate;
            # report against whichever roof (matrix rate of the arithmetic used, or HBM) binds tighter
            if d["bound"] == "hbm" and d["tflops"] / peaks["mfma"][0] > d.get("gbps", 0) / 8000.0:
                ach, (peak, unit), bound = d["tflops"], peaks["mfma"], "mfma"
            elif d["bound"] == "hbm":
                ach, (peak, unit), bound = d["gbps"], peaks["hbm"], "hbm"
            else:
                ach, (peak, unit), bound = d["tflops"], peaks["mfma"], "mfma"
            roof = dict(kernel=dom, bound=bound, achieved=round(ach, 3), peak=peak, unit=unit, frac=round(ach / peak, 4),
                        traffic=None, avg_ms=round(d["avg_ms"], 4))
            # HBM bytes per launch come from separate rocprofv3 --pmc passes (tools/gpu_pass.sh); they are reported only
            # when the committed file was measured on exactly these kernel sources, otherwise null
            # (one file per workload: the GNO kernels' bytes depend on the graph)
            pmc_name = "pmc_traffic.json" if wl_tag == "cfg1" else f"pmc_traffic_{wl_tag}.json"
            pmc = os.path.join(ROOT, "profiles", pmc_name)
            try:
                pj = json.load(open(pmc))
                src = pj.get("_source", {})
                if src.get("csrc_sha16") == csrc_sha16() and world == 1:
                    roof["traffic"] = pj.get(dom, {}).get("bytes_per_launch")
                    roof["traffic_source"] = f"profiles/{pmc_name} (tag {src.get('tag')}, csrc {src.get('csrc_sha16')})"
                else:
                    roof["traffic_source"] = f"profiles/{pmc_name} is from other kernel sources or another N: not reported"
            except Exception:
                pass
        # SQ counters of these kernel sources (tools/gpu_pass.sh -> tools/pmc_sq.py -> profiles/pmc_sq.json): what the kernel is
        # REALLY bound by.  mfma_busy_counted = matrix-pipe time, recomputed products included (the algorithmic `frac` counts the
        # useful flops only); issue_busy = share of the SIMDs' time spent issuing instructions -- vector and LDS instructions of
        # the waves of a SIMD issue one at a time, so a kernel near 0.9 sits on its instruction stream, not on MFMA or HBM
        sq = {}
        try:
            cand = json.load(open(os.path.join(ROOT, "profiles", "pmc_sq.json")))
            if cand.get("_source", {}).get("csrc_sha16") == csrc_sha16() and world == 1 and args.workload == "cfg1":
                sq = cand
        except Exception:
            pass
        if roof is not None and sq.get(dom):
            dd = sq[dom]["derived"]
            roof["counters"] = dict(dd, source=f"profiles/pmc_sq.json (tag {sq['_source'].get('tag')})")
            if dd.get("issue_busy", 0.0) >= 0.75:
                roof["bound_actual"] = ("instruction issue: the SIMDs spend %.0f %% of the kernel issuing vector (%.0f %%) and LDS (%.0f %%) "
                                        "instructions, which share one issue port per SIMD; matrix pipe busy %.0f %%"
                                        % (100 * dd["issue_busy"], 100 * dd.get("valu_issue", 0), 100 * dd.get("lds_issue", 0),
                                           100 * dd.get("mfma_busy_counted", 0)))
        troof = step_roofline_ms(n_total // world, m_lat, e_enc, e_dec, s_tok, args.layers, args.precision, out=wl_out)
        if world > 1 and args.parallel == "seq":   # per-rank work of a perfectly divided step (token rows / heads / points)
            troof["transformer_ms"] /= world
            troof["t_roof_ms"] = troof["transformer_ms"] + troof["gno_ms"] + troof["per_node_ms"] + troof["adamw_ms"]
        troof = {kk: round(v, 4) for kk, v in troof.items()}
        troof["frac"] = round(troof["t_roof_ms"] / ms, 4)
        graph_txt = {"cfg1": f"knn k={args.knn} encoder + flipped decoder",
                     "cfg4": f"knn k={args.knn} encoder + flipped decoder, {wl_out} output fields",
                     "cfg3": "radius-graph encoder (r=0.033, <=32 points per token) + bidirectional decoder (knn k=1 U radius), "
                             "statistical GeoEmbed on both sides, inputs pos + [Mach, AOA]",
                     "yaml": "the reference pressure.yaml graph: bidirectional (knn k=1 U radius r=0.033) encoder and decoder"}[args.workload]
        if args.workload != "cfg1" and args.scaling == "strong":
            metric = {"cfg3": f"mesh-points/sec fwd+bwd, {n_total // 1000}K-pt NASA-CRM-shaped sample (BASELINE configs[3])",
                      "yaml": f"mesh-points/sec fwd+bwd, {n_total // 1000}K-pt DrivAerNet++ sample, pressure.yaml graph",
                      "cfg4": f"mesh-points/sec fwd+bwd, {n_total // 1000000}M-pt DrivAerML-shaped sample, {wl_out} fields (BASELINE configs[4])"}[args.workload]
            wl = {"cfg3": "configs[3]", "yaml": "configs[1] with the reference yaml's graph", "cfg4": "configs[4]"}[args.workload]
            if world > 1:
                wl += f" split over {world} GPUs"
        elif args.scaling == "strong":
            metric = f"mesh-points/sec fwd+bwd, {n_total // 1000}K-pt DrivAerNet++ sample"
            wl = "configs[1]" if world == 1 else f"configs[2] (the one sample split over {world} GPUs)"
        else:
            metric = (f"mesh-points/sec fwd+bwd, WEAK scaling: one {n_total // 1000}K-pt sample = {args.points // 1000}K points "
                      f"per GPU x {world} GPUs")
            wl = f"configs[1] x {world} points"
        shard_txt = "none"
        if world > 1:
            shard_txt = {"seq": f"point-shard x{world}; latent Transformer split by token rows, attention by heads "
                                f"(all-to-all), weight gradients all-reduced",
                         "head": f"point-shard x{world}; latent Transformer replicated except the attention heads "
                                 f"(all-gather of head outputs)",
                         "replicated": f"point-shard x{world}; latent Transformer replicated"}[args.parallel]
        line = {
            "metric": metric,
            "value": n_total / (elapsed / args.steps),
            "unit": "points/s",
            "n_gpus": world,
            "n_ranks_seen": dist.get_world_size() if world > 1 else 1,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms,
            # median of the timed steps (HIP events at the step boundaries inside the timed region) beside the mean
            "ms_per_step_median": round(statistics.median(step_ms), 4) if step_ms else None,
            "ms_per_step_min_max": [round(min(step_ms), 4), round(max(step_ms), 4)] if step_ms else None,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f32" if args.precision == "fp32" else "bf16",
            "data": "synthetic",
            "config": {"workload": f"{wl}: one {n_total}-point car-like surface sample, latent "
                                   f"{latent[0]}x{latent[1]}x{latent[2]}, {graph_txt}, "
                                   f"C=32 P=2 d=256 h=8 F=1024 L={args.layers} rope, attention dropout {args.atten_dropout} "
                                   f"(training mode), MSE + AdamW step; CSR build and geoembed stats inside the step (a decoder list that is the "
                                   f"encoder's with its rows swapped shares the encoder's two lists)",
                       "points": n_total, "latent_tokens": list(latent), "edges": e_enc if world == 1 else n_total * args.knn,
                       "edges_decoder": e_dec if world == 1 else n_total * args.knn, "layers": args.layers,
                       "precision": args.precision, "points_per_gpu": n_total // world, "atten_dropout": args.atten_dropout,
                       "point_order": args.point_order,
                       "sharding": shard_txt},
            "loss": float(loss.detach()),
            "launch": launch_txt,
            "kernel_launches_per_step": launches,
            # census of the REPLAYED graph (HIP graph API): kernel nodes = our launches + whatever ATen / the runtime added
            "graph_nodes_per_step": main_capture["nodes"],
            "foreign_kernel_nodes_per_step": (main_capture["nodes"]["kernel"] - launches
                                              if launches is not None and main_capture["nodes"] and "kernel" in main_capture["nodes"]
                                              else None),
            "host_ms_per_step_timed_region": round(host_ms / args.steps * 1e3, 3),
            # wall / host time of the two instrumented eager steps (right after a capture the eager allocations go back
            # to hipMalloc, so with a captured graph these overstate a warmed-up eager step)
            "instrumented_eager_ms_per_step": round(t_eager * 1e3, 3) if t_eager is not None else None,
            "instrumented_eager_host_ms_per_step": round(t_host * 1e3, 3) if t_host is not None else None,
            "without_attention_dropout": secondary,
            "geometry_cached": geom_cached,
            "hbm_copy_peak_measured": (dict(gbps=copy_peak, frac_of_8tbps=round(copy_peak / 8000.0, 4),
                                            how="float4 copy of 1 GiB (non-temporal loads and stores, 16-KiB chunk per workgroup, 4 loads in flight per "
                                                "thread), read + written bytes, HIP events, same run")
                                       if copy_peak else None),
            "fp32_mode": fp32_mode,
            "other_scaling": weak,
            "roofline": roof,
            "gno_hbm": gno_hbm(per_kernel),
            "step_roofline": troof,
            "kernels": {kname: {kk: (round(v, 4) if isinstance(v, float) else v) for kk, v in ent.items()}
                        for kname, ent in per_kernel.items()},
            "full": args.full,
        }
        if not args.full:       # figures that need runs of their own: --full
            for kk in FULL_ONLY_KEYS:
                del line[kk]
        return line

    if world > 1 and graph is not None:
        launch_txt = (f"segmented hipGraph replay: {graph.num_segments} graph launches + {graph.num_exchanges} eagerly issued "
                      f"exchange steps per step, no collective captured")
    else:
        if graph is not None:
            launch_txt = "hipGraph replay of one captured step"
        elif main_capture["error"]:
            launch_txt = f"eager (hipGraph capture failed: {main_capture['error']})"
        else:
            launch_txt = "eager"
    out = make_out(elapsed, launch_txt, t_host_main, main_step_ms) if rank == 0 else None
    if world > 1 and args.full:
        # one line that explains a flat curve: per rank, the device time inside exchange steps (per collective kind, with the
        # bytes moved) against the device time inside the kernels between them; MIN / MAX over the ranks
        gathered = [None] * world
        dist.all_gather_object(gathered, exchange_profile)
        if rank == 0:
            out["exchange_profile"] = summarize_exchange_profiles(gathered)
            out["exchange_profile"]["backend"] = dict(
                name=str(dist.get_backend()), world_size=dist.get_world_size(),
                rccl_version=(".".join(str(v) for v in torch.cuda.nccl.version()) if not one_device else None),
                grad_group="second communicator (bucketed weight-gradient all-reduce, asynchronous)")
    if rank == 0 and world > 1:
        out["eager"], out["segmented"] = eager_rec, seg_rec
    # ---- N > 1: the same step with the weight-gradient GEMMs, bucket copies and bucket all-reduces on a SIDE stream
    # (ShardedStep(overlap_dw=True): gaot_3d_amd/comm.py side_run), both launch modes again, under a watchdog: a mode that
    # wedges reports the already measured line and leaves instead of hanging the job
    if world > 1 and args.full and not args.no_graph and not args.no_segmented and not args.no_overlap_dw and step_ctx is not None:
        import threading
        ab_done = threading.Event()

        def ab_timeout():
            if ab_done.is_set():
                return
            try:
                if rank == 0:
                    out["overlap_dw"] = dict(error=f"no result after {args.overlap_dw_timeout:.0f} s: the default mode is reported")
                    print(json.dumps(out))
                    sys.stdout.flush()
            finally:
                os._exit(0)
        timer = threading.Timer(args.overlap_dw_timeout + (0.0 if rank == 0 else 15.0), ab_timeout)
        timer.daemon = True
        timer.start()
        ab = {}
        try:
            step_ctx.set_overlap_dw(True)
            e_o, _, loss_o, th_o = measure(step, args.steps, args.warmup, False)
            e_rec, s_rec, prof_o, best_o = sharded_modes(e_o, loss_o, th_o, list(last_step_ms), True)
            ab = dict(eager=e_rec, segmented=s_rec)
            gathered = [None] * world
            dist.all_gather_object(gathered, prof_o)
            if rank == 0:
                ab["exchange_profile"] = summarize_exchange_profiles(gathered)
            if best_o[0] < elapsed:
                elapsed, loss, t_host_main, graph, main_step_ms = best_o
                ab["reported_as_value"] = True
        except Exception as ex:
            ab["error"] = f"{type(ex).__name__}: {ex}"
            print(f"[bench] rank {rank}: overlap_dw A/B failed ({ab['error']})", file=sys.stderr)
        finally:
            ab_done.set()
            timer.cancel()
            step_ctx.set_overlap_dw(False)
        # all ranks agree on which mode is reported (MAX-reduced times are equal on all ranks, so the choice already is)
        if rank == 0:
            if ab.get("reported_as_value"):
                keep = {kk: out[kk] for kk in ("eager", "segmented", "exchange_profile") if kk in out}
                launch_txt = ("overlap_dw: " + (f"segmented hipGraph replay: {graph.num_segments} graph launches + {graph.num_exchanges} "
                                                f"exchange steps + side-stream closures" if graph is not None else "eager"))
                out = make_out(elapsed, launch_txt, t_host_main, main_step_ms)
                out.update(keep)
            out["overlap_dw"] = ab
    attempted = False
    if world > 1 and args.graph and not args.no_graph and not one_device:
        def on_timeout():
            if rank == 0:
                out["graph_attempt"] = f"no result after {args.graph_attempt_timeout:.0f} s: eager result reported"
                print(json.dumps(out))
                sys.stdout.flush()
        attempted = True
        res, note = measure_graph_guarded(step, args.steps, args.warmup, on_timeout, args.graph_attempt_timeout)
        if rank == 0:
            out["graph_attempt"] = note
            if res is not None:
                eg, _, _, thg = res
                out["graph"] = dict(ms_per_step=eg / args.steps * 1e3, value=n_total / (eg / args.steps))
                if eg < elapsed:
                    keep = {kk: out[kk] for kk in ("eager", "segmented", "graph", "graph_attempt", "exchange_profile") if kk in out}
                    out = make_out(eg, "hipGraph replay of one captured step (RCCL collectives captured)", thg)
                    out.update(keep)
    if rank == 0:
        if args.full and not args.no_cpu_baseline and world == 1:
            if args.cpu_baseline == "auto":
                out["cpu_baseline"] = cpu_baseline_auto(args.cpu_baseline_budget, args.layers, args.knn, args.seed,
                                                        args.atten_dropout, 500000, latent, args.cpu_baseline_dropout,
                                                        args.cpu_baseline_all_cores)
            else:
                out["cpu_baseline"] = cpu_baseline(args.cpu_baseline, args.layers, args.knn, args.seed, args.atten_dropout,
                                                   500000, latent, args.cpu_baseline_dropout, args.cpu_baseline_all_cores)
        print(json.dumps(out))
        sys.stdout.flush()
    if world > 1:
        if attempted:
            # tearing the process group down after its collectives were captured into a hipGraph was seen to block
            # (1-rank RCCL group, tools/try_graph_rccl1.py): the result is out, leave without the teardown
            sys.stderr.flush()
            os._exit(0)
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
