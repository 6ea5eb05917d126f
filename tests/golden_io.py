"""Loader for tests/golden/*.npz (made by oracle/make_goldens.py from the reference)."""
import json
import os
import types

import numpy as np
import torch

from gaot_3d_amd.data import MeshBatch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def part_paths(name):
    """name.npz, then name.part1.npz, name.part2.npz, ... while they exist (a golden that would reach the 1 MiB limit of a
    committed file is stored in parts, oracle/make_goldens.py: write_parts)"""
    paths = [os.path.join(GOLDEN_DIR, name + ".npz")]
    while os.path.exists(os.path.join(GOLDEN_DIR, f"{name}.part{len(paths)}.npz")):
        paths.append(os.path.join(GOLDEN_DIR, f"{name}.part{len(paths)}.npz"))
    return paths


def load(name):
    meta = None
    groups = {"sd": {}, "in": {}, "out": {}, "grad": {}}
    for path in part_paths(name):
        z = np.load(path)
        for k in z.files:
            if k == "__meta__":
                meta = json.loads(bytes(z["__meta__"]).decode())
                continue
            g, rest = k.split("/", 1)
            groups[g][rest] = torch.from_numpy(np.array(z[k]))
    return meta, groups


def sub(d, prefix):
    """entries of d under 'prefix/' with the prefix stripped"""
    p = prefix + "/"
    return {k[len(p):]: v for k, v in d.items() if k.startswith(p)}


def batch_from(meta, ins):
    b = MeshBatch()
    for k, v in ins.items():
        if k != "tokens_pos":
            setattr(b, k, v)
    b.num_graphs = meta["num_graphs"]
    return b


def ns_config(meta):
    """Plain-namespace config (for the oracle, which is duck-typed)."""
    mag = dict(use_gno=True, gno_radius=0.033, in_gno_channel_mlp_hidden_layers=[64, 64, 64],
               in_gno_transform_type="linear", projection_channels=256,
               out_gno_channel_mlp_hidden_layers=[64, 64], out_gno_transform_type="linear", mlp_type="channel",
               scales=[1.0], use_scale_weights=False, use_attn=None, attention_type="cosine",
               use_geoembed=[True, True], embedding_method="statistical", pooling="max",
               sampling_strategy=None, neighbor_strategy="radius", k_neighbors=1)
    mag.update(meta["magno"])
    attn = dict(hidden_size=256, num_heads=8, num_kv_heads=8, atten_dropout=0.1)
    attn.update(meta["attn"])
    ffn = dict(hidden_size=1024)
    ffn.update(meta["ffn"])
    tr = dict(patch_size=8, hidden_size=256, use_attn_norm=True, use_ffn_norm=True, norm_eps=1e-6, num_layers=3,
              positional_embedding="absolute", use_long_range_skip=True)
    tr.update(meta["transformer"])
    tr["attn_config"] = types.SimpleNamespace(**attn)
    tr["ffn_config"] = types.SimpleNamespace(**ffn)
    return types.SimpleNamespace(magno=types.SimpleNamespace(**mag), transformer=types.SimpleNamespace(**tr),
                                 latent_tokens=tuple(meta["latent_tokens"]))
