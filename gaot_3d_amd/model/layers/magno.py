"""MAGNO encoder / decoder with the reference's class names, constructor signatures, config dataclass
and state_dict layout (src/model/layers/magno.py: MAGNOConfig :21-66, MAGNOEncoder :377-600,
MAGNODecoder :605-798), computing through the HIP kernels.

Edges are INPUTS of the hot path (precompute_edges=True, magno.py:506-511 / 715-720).  Building them
(get_neighbor_strategy, :116-295) is the next row of SURVEY §8f; ``get_neighbor_strategy`` here covers
the strategies through plain torch helpers so the data layer keeps its import, and is not the measured
path."""
from dataclasses import dataclass, field
from typing import Any, List, Optional, Tuple, Union

import torch
import torch.nn as nn

from ... import functional as GF
from ...data import coalesce_edges, knn_edges_bruteforce, radius_edges_bruteforce
from .geoembed import GeometricEmbedding
from ...graph import apply_neighbor_sampling  # noqa: F401  (the reference exports it from this module, magno.py:297-371)
from .integral_transform import IntegralTransform, graph_for
from .mlp import ChannelMLP, LinearChannelMLP


@dataclass
class MAGNOConfig:
    # GNO parameters
    use_gno: bool = True
    gno_coord_dim: int = 2
    gno_radius: float = 0.033
    # MAGNOEncoder
    lifting_channels: int = 16
    encoder_feature_attr: Any = "x"
    in_gno_channel_mlp_hidden_layers: list = field(default_factory=lambda: [64, 64, 64])
    in_gno_transform_type: str = "linear"
    # MAGNODecoder
    projection_channels: int = 256
    out_gno_channel_mlp_hidden_layers: list = field(default_factory=lambda: [64, 64])
    out_gno_transform_type: str = "linear"
    mlp_type: str = "channel"
    # multiscale aggregation
    scales: list = field(default_factory=lambda: [1.0])
    use_scale_weights: bool = False
    use_graph_cache: bool = True
    gno_use_torch_cluster: bool = False
    gno_use_torch_scatter: str = True
    node_embedding: bool = False
    use_attn: Optional[bool] = None
    attention_type: str = "cosine"
    # Geometric embedding
    use_geoembed: Any = field(default_factory=lambda: [True, True])
    embedding_method: str = "statistical"
    pooling: str = "max"
    # Sampling
    sampling_strategy: Optional[str] = None
    max_neighbors: Optional[int] = None
    sample_ratio: Optional[float] = None
    # neighbor finding strategy
    neighbor_strategy: Any = "radius"
    k_neighbors: int = 1
    # Dataset
    precompute_edges: bool = True
    asynchronous_graph_building: bool = False


def parse_neighbor_strategy(neighbor_strategy: Union[str, List[str]]) -> Tuple[str, str]:
    if isinstance(neighbor_strategy, str):
        return neighbor_strategy, neighbor_strategy
    if isinstance(neighbor_strategy, (list, tuple)) and len(neighbor_strategy) == 2:
        return neighbor_strategy[0], neighbor_strategy[1]
    raise ValueError(f"neighbor_strategy must be str or list of length 2, got {neighbor_strategy}")


def parse_geoembed_strategy(use_geoembed: Union[bool, List[bool]]) -> Tuple[bool, bool]:
    if isinstance(use_geoembed, bool):
        return use_geoembed, use_geoembed
    if isinstance(use_geoembed, (list, tuple)) and len(use_geoembed) == 2:
        return use_geoembed[0], use_geoembed[1]
    raise ValueError(f"use_geoembed must be bool or list of length 2, got {use_geoembed}")


def _per_graph(fn, phys_pos, batch_idx_phys, latent_pos, batch_idx_latent):
    """apply a single-graph edge builder per batch element and offset the indices"""
    nb = int(batch_idx_phys.max().item()) + 1 if batch_idx_phys.numel() else 1
    out = []
    for b in range(nb):
        pm = (batch_idx_phys == b).nonzero(as_tuple=True)[0]
        lm = (batch_idx_latent == b).nonzero(as_tuple=True)[0]
        e = fn(phys_pos[pm], latent_pos[lm])  # rows index into the per-graph subsets
        out.append((e, pm, lm))
    return out


def get_neighbor_strategy(neighbor_strategy: str, phys_pos, batch_idx_phys, latent_tokens_pos, batch_idx_latent,
                          radius: float, k_neighbors: int = 1, is_decoder: bool = False, latent_dims=None):
    """Edge construction with the reference's conventions (magno.py:116-295): encoder edges are
    [phys_idx, latent_idx], decoder edges [latent_idx, phys_idx]; 'bidirectional' = coalesce(knn U radius);
    'reverse' (decoder only) = flip of the *bidirectional* encoder graph; PyG radius keeps at most 32
    neighbours per centre.  With the points on the HIP device the graph is built by the device kernels
    (gaot_3d_amd/graph.py, csrc/graph.hip): closed-form cell lookups when the tokens are the model's regular
    D x H x W grid (``latent_dims``), brute-force scans of all tokens for any other token set; for CPU tensors by
    the brute-force torch restatement below (host-side data preparation, also the checker of the device path in
    tests/test_graph_gpu.py)."""
    if phys_pos.is_cuda:   # device kernels: cell lookups on the regular token grid, brute-force scans for any other token set
        from ... import graph as device_graph
        return device_graph.get_neighbor_strategy(neighbor_strategy, phys_pos, batch_idx_phys, latent_tokens_pos,
                                                  batch_idx_latent, radius, k_neighbors, is_decoder, latent_dims=latent_dims)

    def enc(strategy, p, l):
        knn = rad = None
        if strategy in ("knn", "bidirectional"):
            knn = knn_edges_bruteforce(p, l, k_neighbors)
        if strategy in ("radius", "bidirectional"):
            rad = radius_edges_bruteforce(p, l, radius, 32, centers="latent")
        if strategy == "knn":
            return knn
        if strategy == "radius":
            return rad
        if strategy == "bidirectional":
            return coalesce_edges(torch.cat([knn, rad], dim=1), l.shape[0])
        raise ValueError(f"Unknown encoder strategy: {strategy}")

    def dec(strategy, p, l):
        if strategy == "reverse":
            return enc("bidirectional", p, l).flip(0)
        knn = rad = None
        if strategy in ("knn", "bidirectional"):
            knn = knn_edges_bruteforce(p, l, k_neighbors).flip(0)
        if strategy in ("radius", "bidirectional"):
            rad = radius_edges_bruteforce(p, l, radius, 32, centers="phys")
        if strategy == "knn":
            return knn
        if strategy == "radius":
            return rad
        if strategy == "bidirectional":
            return coalesce_edges(torch.cat([knn, rad], dim=1), p.shape[0])
        raise ValueError(f"Unknown decoder strategy: {strategy}")

    parts = _per_graph((lambda p, l: dec(neighbor_strategy, p, l)) if is_decoder else
                       (lambda p, l: enc(neighbor_strategy, p, l)),
                       phys_pos, batch_idx_phys, latent_tokens_pos, batch_idx_latent)
    outs = []
    for e, pm, lm in parts:
        if is_decoder:
            outs.append(torch.stack([lm[e[0]], pm[e[1]]]))
        else:
            outs.append(torch.stack([pm[e[0]], lm[e[1]]]))
    return torch.cat(outs, dim=1) if outs else torch.empty((2, 0), dtype=torch.long, device=phys_pos.device)


def _make_mlp(mlp_type, layers):
    if mlp_type == "linear":
        return LinearChannelMLP(layers=layers)
    if len(layers) == 2:
        return ChannelMLP(in_channels=layers[0], out_channels=layers[1], n_layers=1)
    return ChannelMLP(in_channels=layers[0], out_channels=layers[-1], hidden_channels=layers[1], n_layers=len(layers) - 1,
                      n_dim=1)


def _check_unsupported(cfg: MAGNOConfig):
    if cfg.sampling_strategy not in (None, "max_neighbors", "ratio"):
        raise ValueError(f"Invalid sampling strategy: {cfg.sampling_strategy}")


def _sample(module, edge_index, num_query):
    """reference magno.py:529-538 / 739-748"""
    if module.sampling_strategy is None:
        return edge_index
    from ...graph import apply_neighbor_sampling
    return apply_neighbor_sampling(edge_index, num_query, edge_index.device, module.sampling_strategy, module.max_neighbors,
                                   module.sample_ratio, module.training)


def _sum_scales(outs):
    acc = outs[0]
    for o in outs[1:]:
        acc = GF.add(acc, o)
    return acc


def _make_scale_weighting(coord_dim, num_scales):
    return nn.Sequential(nn.Linear(coord_dim, 16), nn.ReLU(), nn.Linear(16, num_scales))


def _scale_logits(module, pos):
    """the logits of the scale weights, l = W_2 relu(W_1 pos + b_1) + b_2 -> (l [n, scales], the hidden layer relu(..) [n, 16])"""
    sw = module.scale_weighting
    h = GF.linear(pos, sw[0].weight, sw[0].bias, act="relu", precision=0)
    return GF.linear(h, sw[2].weight, sw[2].bias, precision=0), h


def _mix_scales(module, outs, pos):
    """sum over scales, or softmax-weighted by an MLP of the query coordinates (reference magno.py:586-596)"""
    if len(outs) == 1:
        return outs[0]
    if not module.use_scale_weights:
        return _sum_scales(outs)
    return GF.ScaleMixFn.apply(_scale_logits(module, pos)[0], *outs)


def _softmax_weight_tangents(w, active, w1, w2, rows_matmul):
    """The derivative of the scale weights w = softmax(l), l = W_2 relu(W_1 pos + b_1) + b_2, with respect to the position:
        d_d l = W_2 (1[z > 0] * W_1[:, d]),    d_d w_s = w_s (d_d l_s - sum_t w_t d_d l_t)
    ``w`` [n, scales], ``active`` = 1[z > 0] [n, hidden], ``w1`` [hidden, dims], ``w2`` [scales, hidden];
    ``rows_matmul(x, W)`` = x W^T row by row.  -> one [n, scales] tensor per direction.  The sum over the scales is written term by
    term: a row's result does not depend on how many rows there are."""
    return [_softmax_weight_jets(w, dl)[0] for dl in _logit_tangents(active, w1, w2, rows_matmul)]


def _logit_tangents(active, w1, w2, rows_matmul):
    """d_d l = W_2 (1[z > 0] * W_1[:, d]) of ``_softmax_weight_tangents``, one [n, scales] tensor per coordinate axis"""
    return [rows_matmul(active * w1[:, d], w2) for d in range(w1.shape[1])]


def _softmax_weight_jets(w, dl, second=False):
    """The first and second directional derivative of w = softmax(l) along a direction in which l' = ``dl`` [n, scales] and l'' = 0
    (l is piecewise linear in the position):
        m = sum_t w_t l'_t,   w'_s = w_s (l'_s - m),   m' = sum_t w'_t l'_t,   w''_s = w'_s (l'_s - m) - w_s m'
    -> (w' [n, scales], w'' [n, scales] or None without ``second``); sum_s w'_s = sum_s w''_s = 0.  The sums over the scales are
    written term by term: a row's result does not depend on how many rows there are."""
    ns = w.shape[1]
    mean = w[:, 0] * dl[:, 0]
    for s in range(1, ns):
        mean = mean + w[:, s] * dl[:, s]
    dw = torch.stack([w[:, s] * (dl[:, s] - mean) for s in range(ns)], dim=1)
    if not second:
        return dw, None
    dmean = dw[:, 0] * dl[:, 0]
    for s in range(1, ns):
        dmean = dmean + dw[:, s] * dl[:, s]
    ddw = torch.stack([dw[:, s] * (dl[:, s] - mean) - w[:, s] * dmean for s in range(ns)], dim=1)
    return dw, ddw


def _logit_tangent_rows(dls, v):
    """the logit tangent along a PER-ROW direction: l'_v = sum_c v[:, c] * d_c l from the axis tangents ``dls`` (``_logit_tangents``),
    ``v`` [n, 3], summed in the order c = 0, 1, 2 -> [n, scales].  Per-row operations: a row's result does not depend on the other
    rows; a row whose direction is an axis gets that axis tangent itself (products with 1 and sums with 0 are exact)."""
    dl = v[:, 0:1] * dls[0]
    for c in range(1, min(len(dls), v.shape[1])):
        dl = dl + v[:, c:c + 1] * dls[c]
    return dl


def _logit_tangent_along(dls, dirs, i, like):
    """l'_v along direction i of ``dirs`` from the axis tangents ``dls``: per-row directions [n, nd, 3] (``_logit_tangent_rows``) or host
    values [nd][3] (an axis: that tangent itself; zeros of ``like``'s shape for the zero direction) -- ``_mix_jet2_planes``'s
    expressions, for the transposed mix (``MAGNODecoder._mix_cot``)"""
    if isinstance(dirs, torch.Tensor):
        return _logit_tangent_rows(dls, dirs[:, i])
    dl = None
    for c, vc in enumerate(dirs[i]):
        if vc == 0.0 or c >= len(dls):
            continue
        term = dls[c] if vc == 1.0 else vc * dls[c]
        dl = term if dl is None else dl + term
    return torch.zeros_like(like) if dl is None else dl


def _mix_jet2_planes(w, dls, outs, d1s, d2s, dirs, second=True):
    """The softmax-weighted mix of the scales' 2-jets: ``w`` [n, scales], ``dls`` the logit tangents along the coordinate axes
    (``_logit_tangents``), ``outs[s]`` [n, C] and ``d1s[s]`` / ``d2s[s]`` [nd, n, C] the value, D_v and D_v^2 planes of scale s along
    ``dirs`` (host values [nd][3]) -> (D_v mix per direction, D_v^2 mix per direction, w' per direction, w'' per direction):
        D_v mix = sum_s (w_s D_v o_s + w'_s o_s),     D_v^2 mix = sum_s (w_s D_v^2 o_s + 2 w'_s D_v o_s + w''_s o_s)
    with l'_v = sum_c v_c d_c l formed from the axis tangents (an axis direction: that tangent itself; e_i + e_j: their sum).  Per-row
    operations with the sums over the scales written term by term, in the dtype of the operands.  ``dirs`` may also be a TENSOR
    [n, nd, 3] of per-row directions: then l'_v is the per-row expression of ``_logit_tangent_rows`` and everything after it is the
    same code (rows whose directions are the axes get the axis results bit for bit).  Without ``second`` (first order:
    ``d2s`` is not read) neither w'' nor a D_v^2 mix is formed: no second-order plane is returned and every w'' is None."""
    ns = len(outs)
    p1, p2, dws, ddws = [], [], [], []
    per_row = isinstance(dirs, torch.Tensor)            # PER-ROW directions [n, nd, 3] (``sample_directional``)
    for i in range(dirs.shape[1]) if per_row else range(len(dirs)):
        if per_row:
            dl = _logit_tangent_rows(dls, dirs[:, i])
        else:
            dl = None
            for c, vc in enumerate(dirs[i]):
                if vc == 0.0 or c >= len(dls):
                    continue
                term = dls[c] if vc == 1.0 else vc * dls[c]
                dl = term if dl is None else dl + term
            if dl is None:
                dl = torch.zeros_like(w)
        dw, ddw = _softmax_weight_jets(w, dl, second=second)
        a1 = a2 = None
        for s in range(ns):
            ws, dws_ = w[:, s:s + 1], dw[:, s:s + 1]
            t1 = ws * d1s[s][i] + dws_ * outs[s]
            a1 = t1 if a1 is None else a1 + t1
            if second:
                t2 = ws * d2s[s][i] + (2.0 * dws_) * d1s[s][i] + ddw[:, s:s + 1] * outs[s]
                a2 = t2 if a2 is None else a2 + t2
        p1.append(a1)
        if second:
            p2.append(a2)
        dws.append(dw)
        ddws.append(ddw)
    return p1, p2, dws, ddws


def _num_dirs(dirs) -> int:
    """the number of directions: host values [nd][3], or a tensor [n, nd, 3] of per-row directions"""
    return int(dirs.shape[1]) if isinstance(dirs, torch.Tensor) else len(dirs)


def _mix_scales_jet2(module, outs, d1s, d2s, pos, dirs):
    """``_mix_scales`` with its jets along ``dirs`` (host values [nd][3] or per-row directions [n, nd, 3]):``outs[s]`` [n, C], ``d1s[s]`` / ``d2s[s]`` [nd, n, C] of every scale
    -> [value, D_v per direction ..., D_v^2 per direction ...], [n, C] each; FIRST ORDER with ``d2s`` None: [value, D_v per direction ...]
    and nothing of second order is computed.  The value is ``_mix_scales``'s bit for bit, and a direction's D_v plane does not depend
    on the order.  Summed scales: the sum of each plane; one scale: the planes as they are.  Softmax weights w = softmax(l),
    l = W_2 relu(W_1 pos + b_1) + b_2, depend on the query position themselves, and the scales of a row-list decoder see different
    lists, so neither sum_s w'_s o_s nor sum_s w''_s o_s vanishes (``_mix_jet2_planes``); the logits are piecewise linear in the
    position (l'' = 0 away from the ReLU kinks of the weighting MLP).  Per-row fp32 operations only (the row kernels and elementwise
    torch ops): a row's result does not depend on the chunk it is in."""
    ns, nd = len(outs), _num_dirs(dirs)
    jets = [d1s] if d2s is None else [d1s, d2s]
    if ns == 1:
        return [outs[0]] + [p for js in jets for p in js[0].unbind(0)]
    if not module.use_scale_weights:
        return [_sum_scales(outs)] + [_sum_scales([j[d] for j in js]) for js in jets for d in range(nd)]
    sw = module.scale_weighting
    logits, h = _scale_logits(module, pos)
    value = GF.ScaleMixFn.apply(logits, *outs)
    w = torch.softmax(logits, dim=1)                       # [n, scales]
    active = (h > 0).to(h.dtype)                           # relu'(z): [n, 16]
    dls = _logit_tangents(active, sw[0].weight, sw[2].weight, lambda x, wt: GF.linear(x, wt, None, precision=0))
    p1, p2, _, _ = _mix_jet2_planes(w, dls, outs, d1s, d2s, dirs, second=d2s is not None)
    return [value, *p1, *p2]


class MAGNOEncoder(nn.Module):
    def __init__(self, in_channels, out_channels, gno_config: MAGNOConfig):
        super().__init__()
        _check_unsupported(gno_config)
        self.sampling_strategy = gno_config.sampling_strategy
        self.max_neighbors = gno_config.max_neighbors
        self.sample_ratio = gno_config.sample_ratio
        self.gno_radius = gno_config.gno_radius
        self.scales = gno_config.scales
        self.lifting_channels = gno_config.lifting_channels
        self.coord_dim = gno_config.gno_coord_dim
        self.feature_attr_name = gno_config.encoder_feature_attr
        self.precompute_edges = gno_config.precompute_edges
        self.mlp_type = gno_config.mlp_type
        self.encoder_strategy, self.decoder_strategy = parse_neighbor_strategy(gno_config.neighbor_strategy)
        self.k_neighbors = gno_config.k_neighbors
        self.use_gno = gno_config.use_gno
        if self.use_gno:
            kin = self.coord_dim * 2
            if gno_config.in_gno_transform_type in ("nonlinear", "nonlinear_kernelonly"):
                kin += in_channels
            layers = [kin] + list(gno_config.in_gno_channel_mlp_hidden_layers) + [self.lifting_channels]
            self.gno = IntegralTransform(channel_mlp_layers=layers, transform_type=gno_config.in_gno_transform_type,
                                         use_attn=gno_config.use_attn, coord_dim=self.coord_dim,
                                         attention_type=gno_config.attention_type)
            self.lifting = _make_mlp(gno_config.mlp_type, [in_channels, self.lifting_channels])
        else:
            self.gno = None
            self.lifting = None
        self.use_geoembed = parse_geoembed_strategy(gno_config.use_geoembed)[0]
        if self.use_geoembed:
            self.geoembed = GeometricEmbedding(input_dim=self.coord_dim, output_dim=self.lifting_channels,
                                               method=gno_config.embedding_method, pooling=gno_config.pooling)
            self.recovery = _make_mlp(gno_config.mlp_type, [2 * self.lifting_channels, self.lifting_channels])
        self.use_scale_weights = gno_config.use_scale_weights
        if self.use_scale_weights:
            self.num_scales = len(self.scales)
            self.scale_weighting = _make_scale_weighting(self.coord_dim, self.num_scales)
            self.scale_weight_activation = nn.Softmax(dim=-1)

    def _features(self, batch):
        names = self.feature_attr_name if isinstance(self.feature_attr_name, (list, tuple)) else [self.feature_attr_name]
        feats = []
        for a in names:
            f = getattr(batch, a, None)
            if f is None:
                if self.use_gno:
                    raise AttributeError(f"MAGNOEncoder requires feature attribute '{a}' but it was not found in the batch.")
            else:
                feats.append(f)
        return feats

    def forward(self, batch, latent_tokens_pos: torch.Tensor, latent_tokens_batch_idx: torch.Tensor) -> torch.Tensor:
        phys_pos = batch.pos
        device = phys_pos.device
        num_graphs = batch.num_graphs
        m_per_graph = latent_tokens_pos.shape[0] // num_graphs
        phys_feat = self._features(batch)
        lifted = None
        if self.use_gno:  # scale-independent: lift once; [f0|f1|..] W^T is evaluated without materialising the cat
            if len(self.lifting.fcs) == 1 and not (self.training and getattr(self.lifting, "dropout_p", 0.0) > 0.0):
                lifted = GF.cat_linear(phys_feat, self.lifting.fcs[0].weight, self.lifting.fcs[0].bias, precision=0)
            else:   # a caller-supplied deeper lifting MLP (the reference's constructor always builds one layer)
                lifted = self.lifting.forward_rows(phys_feat[0] if len(phys_feat) == 1 else torch.cat(phys_feat, dim=1))
        outs = []
        for si, scale in enumerate(self.scales):
            if self.precompute_edges:
                attr = f"encoder_edge_index_s{si}"
                if not hasattr(batch, attr):
                    raise AttributeError(f"Batch object missing pre-computed '{attr}'")
                edge_index = getattr(batch, attr).to(device)
            else:
                edge_index = get_neighbor_strategy(self.encoder_strategy, phys_pos, batch.batch, latent_tokens_pos,
                                                   latent_tokens_batch_idx, self.gno_radius * scale, self.k_neighbors,
                                                   False, latent_dims=getattr(self, "latent_dims", None)).to(device)
            edge_index = _sample(self, edge_index, latent_tokens_pos.shape[0])
            g = graph_for(edge_index, phys_pos.shape[0], latent_tokens_pos.shape[0],
                          batch if self.sampling_strategy is None else None, ("enc", si))
            enc = self.gno(y_pos=phys_pos, x_pos=latent_tokens_pos, edge_index=edge_index, f_y=lifted,
                           graph=g) if self.use_gno else None
            shard_group = getattr(self, "_shard_group", None)
            if shard_group is not None and enc is not None:
                # point-sharded sample (gaot_3d_amd/sharding.py): the local mean becomes the mean over every rank's edges
                from ...sharding import GlobalSegmentMeanFn
                deg = (g.by_dst.rowptr[1:] - g.by_dst.rowptr[:-1]).to(enc.dtype)
                enc = GlobalSegmentMeanFn.apply(enc, deg, shard_group)
            # GeoEmbed statistics of a sharded sample: additive moments of the local edges, summed over the ranks
            geo = self.geoembed(phys_pos, latent_tokens_pos, edge_index, graph=g, shard_group=shard_group) \
                if self.use_geoembed else None
            if enc is not None and geo is not None:
                enc = GF.cat_linear([enc, geo], self.recovery.fcs[0].weight, self.recovery.fcs[0].bias, precision=0)
            elif enc is None and geo is not None:
                enc = geo
            elif enc is None:
                raise ValueError("GNO and GeoEmbed are both disabled. No encoding will be performed.")
            outs.append(enc)
        out = _mix_scales(self, outs, latent_tokens_pos)
        return out.view(num_graphs, m_per_graph, self.lifting_channels)


class MAGNODecoder(nn.Module):
    def __init__(self, in_channels, out_channels, gno_config: MAGNOConfig):
        super().__init__()
        _check_unsupported(gno_config)
        self.sampling_strategy = gno_config.sampling_strategy
        self.max_neighbors = gno_config.max_neighbors
        self.sample_ratio = gno_config.sample_ratio
        self.gno_radius = gno_config.gno_radius
        self.scales = gno_config.scales
        self.coord_dim = gno_config.gno_coord_dim
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.use_geoembed = parse_geoembed_strategy(gno_config.use_geoembed)[1]
        self.use_scale_weights = gno_config.use_scale_weights
        self.precompute_edges = gno_config.precompute_edges
        self.mlp_type = gno_config.mlp_type
        self.encoder_strategy, self.decoder_strategy = parse_neighbor_strategy(gno_config.neighbor_strategy)
        self.k_neighbors = gno_config.k_neighbors
        kin = self.coord_dim * 2
        if gno_config.out_gno_transform_type in ("nonlinear", "nonlinear_kernelonly"):
            kin += in_channels
        layers = [kin] + list(gno_config.out_gno_channel_mlp_hidden_layers) + [in_channels]
        self.gno = IntegralTransform(channel_mlp_layers=layers, transform_type=gno_config.out_gno_transform_type,
                                     use_attn=gno_config.use_attn, coord_dim=self.coord_dim,
                                     attention_type=gno_config.attention_type)
        self.projection = _make_mlp(gno_config.mlp_type, [in_channels, gno_config.projection_channels, out_channels])
        if self.use_geoembed:
            self.geoembed = GeometricEmbedding(input_dim=self.coord_dim, output_dim=in_channels,
                                               method=gno_config.embedding_method, pooling=gno_config.pooling)
            self.recovery = _make_mlp(gno_config.mlp_type, [2 * in_channels, in_channels])
        if self.use_scale_weights:
            self.num_scales = len(self.scales)
            self.scale_weighting = _make_scale_weighting(self.coord_dim, self.num_scales)
            self.scale_weight_activation = nn.Softmax(dim=-1)

    def forward(self, rndata_flat, phys_pos_query, batch_idx_phys_query, latent_tokens_pos, latent_tokens_batch_idx,
                batch=None) -> torch.Tensor:
        return self._decode(rndata_flat, phys_pos_query, batch_idx_phys_query, latent_tokens_pos, latent_tokens_batch_idx, batch,
                            self.precompute_edges)

    def _decode(self, rndata_flat, phys_pos_query, batch_idx_phys_query, latent_tokens_pos, latent_tokens_batch_idx, batch,
                precomputed: bool) -> torch.Tensor:
        """``forward``; ``precomputed``: the edge lists are the batch's ``decoder_edge_index_s*`` (else built here for the queries)"""
        device = rndata_flat.device
        outs = []
        for si, scale in enumerate(self.scales):
            if precomputed:
                attr = f"decoder_edge_index_s{si}"
                if not hasattr(batch, attr):
                    raise AttributeError(f"Batch object missing pre-computed '{attr}'")
                edge_index = getattr(batch, attr).to(device)
            else:
                edge_index = get_neighbor_strategy(self.decoder_strategy, phys_pos_query, batch_idx_phys_query,
                                                   latent_tokens_pos, latent_tokens_batch_idx, self.gno_radius * scale,
                                                   self.k_neighbors, True,
                                                   latent_dims=getattr(self, "latent_dims", None)).to(device)
            edge_index = _sample(self, edge_index, phys_pos_query.shape[0])
            g = graph_for(edge_index, latent_tokens_pos.shape[0], phys_pos_query.shape[0],
                          batch if self.sampling_strategy is None else None, ("dec", si))
            dec = self.gno(y_pos=latent_tokens_pos, x_pos=phys_pos_query, edge_index=edge_index, f_y=rndata_flat, graph=g)
            if self.use_geoembed:
                sg = getattr(self, "_shard_group", None)
                if sg is not None:   # point-sharded sample: the z-score (geoembed.py:177-180) runs over ALL query points
                    total = getattr(batch, "shard", (0, 0, 0, 0, phys_pos_query.shape[0]))[4]
                    geo = self.geoembed(latent_tokens_pos, phys_pos_query, edge_index, graph=g, shard_group=sg,
                                        sharded_queries_total=total)
                else:
                    geo = self.geoembed(latent_tokens_pos, phys_pos_query, edge_index, graph=g)
                dec = GF.cat_linear([dec, geo], self.recovery.fcs[0].weight, self.recovery.fcs[0].bias, precision=0)
            outs.append(dec)
        return self.projection.forward_rows(_mix_scales(self, outs, phys_pos_query))

    SAMPLE_CHUNK = 1 << 20      # queries per pass of ``sample`` when the caller names no chunk size

    def _sample_grid(self, latent_tokens_pos):
        """The regular-grid descriptor of the tokens for the streaming path of ``sample`` (None: not the regular grid).  Found once
        per token tensor (object identity + in-place version, as ``graph_for`` keys its cache): ``as_latent_grid`` reads the grid's
        corners on the host, which is a synchronisation and illegal while a stream is being captured -- a capture must follow one
        eager call with the same token tensor."""
        from ... import graph as device_graph
        from ..._lib import GaotError
        dims = getattr(self, "latent_dims", None)
        if dims is None or not latent_tokens_pos.is_cuda or latent_tokens_pos.dim() != 2 or latent_tokens_pos.shape[1] != 3:
            return None
        ent = self.__dict__.get("_gaot_sample_grid")
        if ent is not None and ent[0] is latent_tokens_pos and ent[1] == latent_tokens_pos._version:
            return ent[2]
        if torch.cuda.is_current_stream_capturing():
            raise GaotError("MAGNODecoder.sample: the token grid has not been described yet; call sample once eagerly with this "
                            "token tensor before capturing it in a graph")
        try:
            grid = device_graph.as_latent_grid(latent_tokens_pos, dims)
        except GaotError:
            grid = None
        self.__dict__["_gaot_sample_grid"] = (latent_tokens_pos, latent_tokens_pos._version, grid)
        return grid

    def _stream_grid(self, rndata_flat, query_pos, lat):
        """the token grid's descriptor when the operands allow a streaming path of ``sample`` / ``sample_jacobian`` (the decoder
        strategy is the caller's condition): no neighbour sampling, no decoder GeoEmbed, fp32 3-D coordinates on the device, ONE
        graph's tokens on the model's regular grid, a transform the fused kernels evaluate; None otherwise"""
        if not (self.sampling_strategy is None and not self.use_geoembed
                and rndata_flat.is_cuda and query_pos.dim() == 2 and query_pos.shape[1] == 3 and query_pos.dtype == torch.float32
                and lat.dtype == torch.float32 and lat.is_contiguous() and rndata_flat.shape[0] == lat.shape[0]
                and self.gno._fused_plan(list(self.gno.channel_mlp.fcs), rndata_flat, lat, query_pos) is not None):
            return None
        grid = self._sample_grid(lat)
        if grid is not None and grid.num_tokens != lat.shape[0]:
            grid = None                                   # a batch of several graphs: no streaming
        return grid

    def _project_into(self, x, out) -> None:
        """out[:] = projection(x), rows in blocks.  Unless the projection MLP runs as one fused launch (``Mlp2Fn``, bf16 mode) its
        hidden layer [rows, projection_channels] goes through memory, 8 x the size of x at the shipped 32 -> 256: the blocks keep
        that tensor no larger than x itself, so that a chunk's footprint stays its ids, its GNO rows and its predictions."""
        fcs = self.projection.fcs
        n, hid = x.shape[0], max([fc.weight.shape[0] for fc in fcs[:-1]], default=0)
        step = n
        if hid > x.shape[1] and not GF.Mlp2Fn.eligible(x, fcs, self.projection.non_linearity):
            step = max(1024, n * x.shape[1] // hid)
        for j in range(0, n, step):
            out[j:j + step] = self.projection.forward_rows(x[j:j + step])

    def _sample_args(self, fn, chunk_points) -> int:
        """the argument rules of every ``sample*`` method -> the queries per pass"""
        if self.decoder_strategy == "reverse":
            raise ValueError(f"MAGNODecoder.{fn}: decoder strategy 'reverse' is the flip of the encoder's graph of the sample's own "
                             "points and is undefined for other query points")
        if chunk_points is not None and int(chunk_points) < 1:
            raise ValueError(f"chunk_points must be positive, got {chunk_points}")
        return int(chunk_points) if chunk_points is not None else self.SAMPLE_CHUNK

    def _stream_route(self):
        """the lists the decoder's strategy streams on: 'knn' (the regular lists of ``knn_to_grid``, k_neighbors in ``ops.GNO_KNN_K``),
        'rows' (``graph.query_lists``: 'radius', and 'bidirectional' up to ``graph.QUERY_LIST_MAX_K`` neighbours) or None"""
        from ... import graph as device_graph
        from ... import ops
        strategy, k = self.decoder_strategy, int(self.k_neighbors)
        if strategy == "knn":
            return "knn" if k in ops.GNO_KNN_K else None
        return "rows" if strategy == "radius" or (strategy == "bidirectional" and k <= device_graph.QUERY_LIST_MAX_K) else None

    def _stream_chunks(self, grid, query_pos, chunk: int, route: str, lead: bool = True):
        """The chunks of a streaming route: yields (slice, q, lists) per ``chunk`` queries.  Route 'knn': ``lists`` is the regular list
        (nbr, k) of ``knn_to_grid``, the same for every scale.  Route 'rows': one ``graph.query_lists`` graph per scale, with the
        radius of every scale as ``_decode`` derives it.  With ``lead`` a chunk's list is led by as many padding edges as put its rows
        against the kernel's 32-edge tiles where the list of ALL queries has them, so that a row is summed in the same order whatever
        the chunking (``sample`` streams without)."""
        from ... import graph as device_graph
        strategy, k = self.decoder_strategy, int(self.k_neighbors)
        before = [0] * len(self.scales)           # edges of the earlier chunks, per scale
        for i in range(0, int(query_pos.shape[0]), chunk):
            q = query_pos[i:i + chunk]
            if route == "knn":
                lists = (device_graph.knn_to_grid(q, grid, k), k)
            else:
                lists = []
                for si, scale in enumerate(self.scales):
                    pad = {"lead": before[si] % 32} if lead else {}
                    rows = device_graph.query_lists(strategy, q, grid, self.gno_radius * scale, k, **pad)
                    before[si] += rows.by_dst.num_edges - pad.get("lead", 0)
                    lists.append(rows)
            yield slice(i, i + chunk), q, lists

    def _new(self, like, nq, *tail):
        """an uninitialised result [nq, out_channels, *tail] with the dtype and device of ``like``"""
        return torch.empty(nq, self.out_channels, *tail, dtype=like.dtype, device=like.device)

    @torch.no_grad()
    def sample(self, rndata_flat, query_pos, latent_tokens_pos, chunk_points: Optional[int] = None) -> torch.Tensor:
        """Predictions [Nq, out_channels] of ONE sample's processed token features ``rndata_flat`` [M, C] at any query coordinates
        ``query_pos`` [Nq, coord_dim]: what ``forward`` computes with edges built for the queries, forward only (no autograd graph is
        recorded, the result never requires grad), ``chunk_points`` queries at a time (None: ``SAMPLE_CHUNK``) into one preallocated
        result.

        STREAMING path -- decoder strategy 'knn' with k_neighbors in ``ops.GNO_KNN_K``, tokens on the model's regular grid, no
        neighbour sampling, no decoder GeoEmbed, a transform the fused kernels evaluate (``IntegralTransform._fused_plan``): per
        chunk one ``knn_to_grid`` launch, whose [n, k] id array IS the by-query neighbour list, one ``forward_knn`` launch per
        32-channel pass, the scale mix and the projection MLP.  No edge_index, no sorted lists, nothing sized by Nq but the result.
        (The knn lists do not depend on the scale, so a multi-scale decoder evaluates the transform once and mixes that one result
        with itself, as ``forward`` does with equal operands.)
        Decoder strategies 'radius' and 'bidirectional' (k_neighbors <= 32) stream under the same conditions on ROW lists: per chunk
        and scale ``graph.query_lists`` writes every query's tokens (within the scale's radius, the 32 lowest ids; united with its k
        nearest for 'bidirectional') in ascending order straight into the by-query list -- the list ``forward``'s route reaches
        through cat, coalesce and two CSR builds -- and the fused forward (``gaot_gno_fwd`` / ``gaot_gno_fwd_nl``) reads it as it
        stands: no edge_index, no sort, no by-source list.  The list's length is read on the host once per chunk and scale (it
        sizes the two id arrays), so this route cannot be captured in a graph: it raises GaotError before any launch.
        Every other configuration FALLS BACK to ``forward``'s route -- ``get_neighbor_strategy`` + ``build_graph`` + the general
        decoder -- chunked in the same way.  The exception is a 'statistical' decoder GeoEmbed: its z-score runs over ALL query rows
        (geoembed.py:177-180), so it takes the queries in one piece whatever ``chunk_points`` says.
        'reverse' raises ValueError: it is the flip of a graph of the ENCODER's points and is undefined for other queries."""
        chunk = self._sample_args("sample", chunk_points)
        nq = int(query_pos.shape[0])
        lat = latent_tokens_pos
        route = self._stream_route()
        grid = self._stream_grid(rndata_flat, query_pos, lat) if route else None
        out = self._new(rndata_flat, nq)
        if grid is not None:
            for sl, q, lists in self._stream_chunks(grid, query_pos, chunk, route, lead=False):
                if route == "knn":
                    dec = self._mix_equal_scales([self.gno.forward_knn(lat, q, *lists, rndata_flat)], q)[0]
                else:
                    dec = _mix_scales(self, [self.gno(y_pos=lat, x_pos=q, edge_index=None, f_y=rndata_flat, graph=rows) for rows in lists], q)
                self._project_into(dec, out[sl])
            return out
        if self.use_geoembed and self.geoembed.method == "statistical":
            chunk = max(nq, 1)
        lat_bidx = torch.zeros(lat.shape[0], dtype=torch.long, device=lat.device)
        for i in range(0, nq, chunk):
            q = query_pos[i:i + chunk]
            q_bidx = torch.zeros(q.shape[0], dtype=torch.long, device=q.device)
            out[i:i + chunk] = self._decode(rndata_flat, q, q_bidx, lat, lat_bidx, None, False)
        return out

    # the directions of a Hessian by polarisation: H_ii = D^2_{e_i}, H_ij = (D^2_{e_i + e_j} - D^2_{e_i} - D^2_{e_j}) / 2
    HESSIAN_DIRS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 1.0, 0.0), (0.0, 1.0, 1.0), (1.0, 0.0, 1.0))
    HESSIAN_PAIRS = ((0, 1), (1, 2), (0, 2))      # the axes of directions 3, 4, 5

    def _jet2_stream(self, fn, rndata_flat, query_pos, lat, chunk_points, rows=False, what="second derivatives", jets=True):
        """the argument rules and streaming conditions shared by ``sample_hessian`` and ``sample_laplacian`` and, with ``rows``, by
        ``sample_hessian_rows`` and ``sample_laplacian_rows`` on a 'radius' / 'bidirectional' decoder -> (grid, chunk); raises for
        every configuration they do not stream, naming the condition.  ``sample_vjp`` (``what`` = its name in the refusals) shares
        them without the projection's jet-kernel shape (``jets`` False): it needs the 'linear' transform and a projection of two
        linear layers with a named activation instead."""
        from ... import graph as device_graph
        from ... import ops
        chunk = self._sample_args(fn, chunk_points)
        k = int(self.k_neighbors)
        if rows:
            no = lambda why: NotImplementedError(f"MAGNODecoder.{fn}: {what} on row lists stream for 'radius' and "
                                                 f"'bidirectional' decoders; {why}")
            if self.decoder_strategy not in ("radius", "bidirectional"):
                raise no(f"decoder strategy {self.decoder_strategy!r} is neither")
            if self.decoder_strategy == "bidirectional" and k > device_graph.QUERY_LIST_MAX_K:
                raise no(f"k_neighbors = {k} is above {device_graph.QUERY_LIST_MAX_K}, the longest list graph.query_lists unites")
        else:
            no = lambda why: NotImplementedError(f"MAGNODecoder.{fn}: {what} stream on the regular k-neighbour lists only; {why}")
            if self.decoder_strategy != "knn":
                raise no(f"decoder strategy {self.decoder_strategy!r} is not 'knn'")
            if k not in ops.GNO_KNN_K:
                raise no(f"k_neighbors = {k} is not in {ops.GNO_KNN_K}")
        if getattr(self.gno, "use_attn", False):
            raise no("the attention-weighted transform (use_attn) is not supported")
        if self.use_geoembed:
            raise no("a decoder GeoEmbed is not supported")
        if self.sampling_strategy is not None:
            raise no(f"neighbour sampling ({self.sampling_strategy!r}) is not supported")
        fcs = list(self.projection.fcs)
        if not jets:
            if self.gno.transform_type != "linear":
                raise no(f"transform type {self.gno.transform_type!r} is not 'linear' (the adjoint kernel is the linear transform's)")
            if not (len(fcs) == 2 and self.projection.non_linearity in ops.ACT):
                raise no("the projection is not two linear layers with a named activation between them (layers "
                         f"{[tuple(fc.weight.shape[:2]) for fc in fcs]}, activation {self.projection.non_linearity!r})")
        elif not (len(fcs) == 2 and self.projection.non_linearity == "gelu" and fcs[0].bias is not None and ops.mlp2_jet2_supported(
                fcs[0].weight.shape[1], fcs[0].weight.shape[0], fcs[1].weight.shape[0], 3, ops.ACT["gelu"])):
            raise no("the projection is not a two-layer erf-GELU MLP 32 -> {64, 128, 256} -> 1..4 with a first bias (layers "
                     f"{[tuple(fc.weight.shape[:2]) for fc in fcs]})")
        grid = self._stream_grid(rndata_flat, query_pos, lat)
        if grid is None:
            raise no("the operands do not stream (fp32 3-D query coordinates on the device, ONE graph's tokens on the model's regular "
                     "grid and a transform the fused kernels evaluate are needed)")
        return grid, chunk

    def _mix_equal_scales(self, planes, q):
        """the scale mix of the knn route applied to every plane with the same weights: every scale sees the same list, so the mix is
        of equal operands and the derivatives of its softmax weights drop out (``sample_jacobian``); one scale: the planes as they are"""
        ns = len(self.scales)
        if ns > 1 and self.use_scale_weights:
            logits = _scale_logits(self, q)[0]
            return [GF.ScaleMixFn.apply(logits, *([p] * ns)) for p in planes]
        if ns > 1:
            return [_sum_scales([p] * ns) for p in planes]
        return planes

    def _jet_planes(self, rndata_flat, q, lat, lists, dirs=None):
        """The mixed GNO planes of one chunk, [value, D_v per direction ..., D_v^2 per direction ...] along ``dirs``; first order with
        ``dirs`` None: [value, d/dx, d/dy, d/dz]; ``dirs`` a tensor [n, nd, 3]: every query's own directions.  On the regular list every scale sees the same rows and the mix is of equal operands
        (``_mix_equal_scales``); on row lists every scale has its own and the mix carries the jets of its weights (``_mix_scales_jet2``)."""
        qd = isinstance(dirs, torch.Tensor)       # per-query directions [n, nd, 3] (``sample_directional``): the ..._qd kernels
        if isinstance(lists, tuple):
            jet2 = self.gno.jet2_knn_qd if qd else self.gno.jet2_knn
            jets = self.gno.jacobian_knn(lat, q, *lists, rndata_flat) if dirs is None else jet2(lat, q, *lists, rndata_flat, dirs)
            return self._mix_equal_scales([jets[0]] + [p for js in jets[1:] for p in js.unbind(0)], q)
        jet2 = self.gno.jet2_rows_qd if qd else self.gno.jet2_rows
        jets = [self.gno.jacobian_rows(lat, q, rndata_flat, rows) if dirs is None else jet2(lat, q, rndata_flat, rows, dirs)
                for rows in lists]
        outs, d1s = [j[0] for j in jets], [j[1] for j in jets]
        d2s = None if dirs is None else [j[2] for j in jets]
        return _mix_scales_jet2(self, outs, d1s, d2s, q, self.HESSIAN_DIRS[:3] if dirs is None else dirs)

    def _jet2_chunk(self, rndata_flat, q, lat, lists, dirs, pred):
        """one chunk of queries: -> (d1, d2) [n, out_channels, nd], the jets of the prediction along ``dirs`` (``_jet_planes``, then the
        projection's jets), the value written into ``pred``.  A call of its own, so that a chunk's GNO planes are freed before the next
        chunk's are allocated."""
        nd = _num_dirs(dirs)
        planes = self._jet_planes(rndata_flat, q, lat, lists, dirs)
        d1 = self._new(pred, q.shape[0], nd)
        d2 = torch.empty_like(d1)
        self.projection.jet2_rows(planes[0], planes[1:1 + nd], planes[1 + nd:1 + 2 * nd], out=(pred, d1, d2))
        return d1, d2

    def _polarise(self, d1, d2, jac, hess) -> None:
        """``jac`` [n, out_channels, 3] and ``hess`` [n, out_channels, 3, 3] from the jets along ``HESSIAN_DIRS``: the D_v planes of the
        three axes, H_ii = D^2_{e_i} and H_ij = H_ji = (D^2_{e_i + e_j} - D^2_{e_i} - D^2_{e_j}) / 2 written from one value"""
        jac[:] = d1[:, :, :3]
        for a in range(3):
            hess[:, :, a, a] = d2[:, :, a]
        for n, (a, b) in enumerate(self.HESSIAN_PAIRS):
            off = 0.5 * (d2[:, :, 3 + n] - d2[:, :, a] - d2[:, :, b])
            hess[:, :, a, b] = off
            hess[:, :, b, a] = off

    def _hessian(self, fn, rndata_flat, query_pos, lat, chunk_points, rows):
        """``sample_hessian`` (``rows`` False) / ``sample_hessian_rows`` on a row-list decoder (True)"""
        rndata_flat, query_pos = rndata_flat.detach(), query_pos.detach()
        grid, chunk = self._jet2_stream(fn, rndata_flat, query_pos, lat, chunk_points, rows=rows)
        nq = int(query_pos.shape[0])
        pred, jac, hess = self._new(rndata_flat, nq), self._new(rndata_flat, nq, 3), self._new(rndata_flat, nq, 3, 3)
        for sl, q, lists in self._stream_chunks(grid, query_pos, chunk, "rows" if rows else "knn"):
            d1, d2 = self._jet2_chunk(rndata_flat, q, lat, lists, self.HESSIAN_DIRS, pred[sl])
            self._polarise(d1, d2, jac[sl], hess[sl])
        return pred, jac, hess

    def _laplacian(self, fn, rndata_flat, query_pos, lat, chunk_points, rows):
        """``sample_laplacian`` (``rows`` False) / ``sample_laplacian_rows`` on a row-list decoder (True): the ordered trace
        (d2_x + d2_y) + d2_z from the three axis directions"""
        rndata_flat, query_pos = rndata_flat.detach(), query_pos.detach()
        grid, chunk = self._jet2_stream(fn, rndata_flat, query_pos, lat, chunk_points, rows=rows)
        nq = int(query_pos.shape[0])
        pred, lap = self._new(rndata_flat, nq), self._new(rndata_flat, nq)
        for sl, q, lists in self._stream_chunks(grid, query_pos, chunk, "rows" if rows else "knn"):
            _, d2 = self._jet2_chunk(rndata_flat, q, lat, lists, self.HESSIAN_DIRS[:3], pred[sl])
            torch.add(d2[:, :, 0] + d2[:, :, 1], d2[:, :, 2], out=lap[sl])
        return pred, lap

    @torch.no_grad()
    def sample_hessian(self, rndata_flat, query_pos, latent_tokens_pos, chunk_points: Optional[int] = None):
        """``sample_jacobian`` with the SECOND spatial derivatives of the field: -> (pred [Nq, out_channels], jac [Nq, out_channels, 3],
        hess [Nq, out_channels, 3, 3]) with hess[q, o, i, j] = d^2 pred[q, o] / d query_pos[q, i] d query_pos[q, j], every query's
        neighbour list held fixed: valid almost everywhere, NOT defined across the surfaces where a query's k nearest tokens change.

        The kernels carry directional 2-jets (value, D_v, D_v^2): per chunk one ``knn_to_grid`` launch, one ``jet2_knn`` launch per
        32-channel pass with the six directions ``HESSIAN_DIRS``, the scale mix on every plane with the same weights, and the
        projection's jets (``jet2_rows``, two launches).  The Hessian follows by polarisation, H_ii = D^2_{e_i} and
        H_ij = (D^2_{e_i + e_j} - D^2_{e_i} - D^2_{e_j}) / 2, in plain tensor operations; hess[..., i, j] and hess[..., j, i] are written
        from the same value.  ``jac`` is the D_v planes of the three axis directions: ``pred`` and ``jac`` are ``sample_jacobian``'s
        bit for bit.  Exact fp32 in both precision modes, no autograd graph, no host synchronisation (capturable after one eager
        call, as ``sample``), results independent of ``chunk_points``.

        Streams under exactly the conditions of ``sample_jacobian``'s 'knn' route plus a projection in the fused family (two-layer
        erf-GELU 32 -> {64, 128, 256} -> 1..4); every other configuration -- 'radius' / 'bidirectional' decoders, other k, use_attn, a
        decoder GeoEmbed, neighbour sampling, tokens off the regular grid, other projections -- raises NotImplementedError naming the
        condition.  'reverse' and a non-positive ``chunk_points`` raise ValueError."""
        return self._hessian("sample_hessian", rndata_flat, query_pos, latent_tokens_pos, chunk_points, False)

    @torch.no_grad()
    def sample_laplacian(self, rndata_flat, query_pos, latent_tokens_pos, chunk_points: Optional[int] = None):
        """``sample_hessian``'s trace without the off-diagonal work: -> (pred [Nq, out_channels], lap [Nq, out_channels]) with
        lap = d^2 pred / dx^2 + d^2 pred / dy^2 + d^2 pred / dz^2, summed in that order from the D_v^2 planes of the three axis
        directions -- bit for bit hess[..., 0, 0] + hess[..., 1, 1] + hess[..., 2, 2] of ``sample_hessian``.  Conditions, errors,
        exactness and capture as there."""
        return self._laplacian("sample_laplacian", rndata_flat, query_pos, latent_tokens_pos, chunk_points, False)

    @torch.no_grad()
    def sample_hessian_rows(self, rndata_flat, query_pos, latent_tokens_pos, chunk_points: Optional[int] = None):
        """``sample_hessian`` for 'radius' and 'bidirectional' decoders, on ROW lists: -> (pred [Nq, out_channels],
        jac [Nq, out_channels, 3], hess [Nq, out_channels, 3, 3]), every query's list held fixed (valid almost everywhere: not across
        the surfaces where a query's list changes, nor -- with softmax scale weights -- across the ReLU kinks of the weighting MLP, where
        the second derivative of its piecewise linear logits is taken as 0).

        Per chunk and scale ``graph.query_lists`` writes the by-query list and ``jet2_rows`` runs the jet kernel on its ragged rows
        (two launches per 32-channel pass, the six directions ``HESSIAN_DIRS``); the scale mix carries the first AND second derivative
        of its softmax weights, since the scales see different lists (``_mix_scales_jet2``); then the projection's jets and the
        polarisation of ``sample_hessian``.  ``pred`` and ``jac`` are ``sample_jacobian(row_lists=True)``'s bit for bit; exact fp32 in
        both precision modes; results independent of ``chunk_points`` (padding edges lead every chunk's list).  The lists are sized
        by a host read: inside a stream capture the call raises GaotError before any launch.

        Streams for 'radius', and for 'bidirectional' with k_neighbors <= ``graph.QUERY_LIST_MAX_K``, under ``sample``'s row-list
        conditions plus a projection in the fused family (``sample_hessian``); on a 'knn' decoder the call IS ``sample_hessian``.
        use_attn, a decoder GeoEmbed, neighbour sampling, tokens off the regular grid, 'bidirectional' with larger k and other
        projections raise NotImplementedError naming the condition; 'reverse' and a non-positive ``chunk_points`` raise ValueError."""
        if self.decoder_strategy == "knn":
            return self.sample_hessian(rndata_flat, query_pos, latent_tokens_pos, chunk_points=chunk_points)
        return self._hessian("sample_hessian_rows", rndata_flat, query_pos, latent_tokens_pos, chunk_points, True)

    @torch.no_grad()
    def sample_laplacian_rows(self, rndata_flat, query_pos, latent_tokens_pos, chunk_points: Optional[int] = None):
        """``sample_hessian_rows``'s trace from the three axis directions: -> (pred [Nq, out_channels], lap [Nq, out_channels]), summed as
        (d2_x + d2_y) + d2_z -- bit for bit hess[..., 0, 0] + hess[..., 1, 1] + hess[..., 2, 2] of ``sample_hessian_rows``.  Conditions
        and errors as there; on a 'knn' decoder the call IS ``sample_laplacian``."""
        if self.decoder_strategy == "knn":
            return self.sample_laplacian(rndata_flat, query_pos, latent_tokens_pos, chunk_points=chunk_points)
        return self._laplacian("sample_laplacian_rows", rndata_flat, query_pos, latent_tokens_pos, chunk_points, True)

    @staticmethod
    def _query_dirs(fn, dirs, query_pos):
        """``sample_directional``'s directions as a contiguous [Nq, nd, 3] tensor ([Nq, 3]: nd = 1); ValueError for everything else"""
        nq = int(query_pos.shape[0])
        if not isinstance(dirs, torch.Tensor):
            raise ValueError(f"{fn}: dirs must be a float32 tensor [{nq}, nd, 3] or [{nq}, 3], got {type(dirs).__name__}")
        if dirs.dtype != torch.float32 or dirs.device != query_pos.device:
            raise ValueError(f"{fn}: dirs must be float32 on the queries' device ({query_pos.device}), got {dirs.dtype} on {dirs.device}")
        if dirs.dim() == 2:
            dirs = dirs[:, None, :]
        if dirs.dim() != 3 or dirs.shape[0] != nq:
            raise ValueError(f"{fn}: dirs must hold the directions of the {nq} queries, [{nq}, nd, 3] or [{nq}, 3], got {tuple(dirs.shape)}")
        if dirs.shape[2] != 3:
            raise ValueError(f"{fn}: a direction has 3 components, got dirs {tuple(dirs.shape)}")
        if not 1 <= dirs.shape[1] <= 6:
            raise ValueError(f"{fn}: 1..6 directions per query, got nd = {dirs.shape[1]}")
        return dirs.detach().contiguous()

    @torch.no_grad()
    def sample_directional(self, rndata_flat, query_pos, dirs, latent_tokens_pos, chunk_points: Optional[int] = None):
        """Derivatives of the field along PER-QUERY directions -- the wall-normal derivative d/dn and d^2/dn^2 of a surface field, the
        derivatives in a local frame (n, t_1, t_2): -> (pred [Nq, out_channels], d1 [Nq, out_channels, nd], d2 [Nq, out_channels, nd])
        with d1[q, o, i] = sum_d v[d] d pred[q, o] / d query_pos[q, d] and d2[q, o, i] = v^T (d^2 pred[q, o] / d query_pos[q]^2) v for
        v = dirs[q, i], every query's neighbour list held fixed (valid almost everywhere, with the caveats of ``sample_hessian`` /
        ``sample_hessian_rows``).  ``dirs``: float32 [Nq, nd, 3] on the queries' device, 1 <= nd <= 6 ([Nq, 3]: nd = 1), used AS GIVEN
        -- no normalisation, d1 is linear and d2 quadratic in a direction's length.

        One value chain and two per direction through the per-edge MLP (``sample_hessian`` runs 13 for v^T H v of any v): the jet
        kernels with the direction of a pass loaded per lane from ``dirs`` (``jet2_knn_qd`` / ``jet2_rows_qd``), then the scale mix and
        the projection's jets exactly as in ``sample_hessian`` / ``sample_hessian_rows``; on row lists with softmax scale weights the
        logit tangent is formed along every row's own direction (``_logit_tangent_rows``).  The route follows the decoder strategy:
        'knn' (k_neighbors in ``ops.GNO_KNN_K``) the regular lists -- no host synchronisation, capturable after one eager call, and
        since ``dirs`` is read on the device a replay sees the directions then in the tensor; 'radius', and 'bidirectional' with
        k_neighbors <= ``graph.QUERY_LIST_MAX_K``, row lists -- GaotError inside a stream capture, before any launch.  Exact fp32 in
        both precision modes, outside autograd, results independent of ``chunk_points``.  With the three axes as every query's
        directions ``pred`` / ``d1`` are ``sample_jacobian``'s (``row_lists=True``) and ``d2`` is the diagonal of ``sample_hessian``'s
        (``_rows``) Hessian, bit for bit, softmax scale weights included.

        Streams under exactly the conditions of ``sample_hessian`` resp. ``sample_hessian_rows`` and raises their NotImplementedError
        otherwise; 'reverse' and a non-positive ``chunk_points`` raise ValueError, and so does a ``dirs`` that is not float32, is on
        another device, or is not [Nq, 1..6, 3]."""
        fn = "sample_directional"
        self._sample_args(fn, chunk_points)
        dirs = self._query_dirs(fn, dirs, query_pos)
        rndata_flat, query_pos = rndata_flat.detach(), query_pos.detach()
        rows = self.decoder_strategy != "knn"
        grid, chunk = self._jet2_stream(fn, rndata_flat, query_pos, latent_tokens_pos, chunk_points, rows=rows)
        nq, nd = int(query_pos.shape[0]), int(dirs.shape[1])
        pred, d1, d2 = self._new(rndata_flat, nq), self._new(rndata_flat, nq, nd), self._new(rndata_flat, nq, nd)
        for sl, q, lists in self._stream_chunks(grid, query_pos, chunk, "rows" if rows else "knn"):
            d1[sl], d2[sl] = self._jet2_chunk(rndata_flat, q, latent_tokens_pos, lists, dirs[sl], pred[sl])
        return pred, d1, d2

    def _project_vjp(self, x, g):
        """the cotangent of the projection's input: dx [rows, C] = g (d projection(x) / d x) for x [rows, C] (the mixed GNO rows) and
        the cotangent g [rows, out_channels], in exact fp32 on the GEMM / activation kernels: z = x W_1^T + b_1,
        dh = (g W_2) * act'(z), dx = dh W_1.  Rows in blocks, so that the [rows, projection_channels] tensors stay no larger than x
        itself (``_project_into``)."""
        return self._project_cot(0, [x], g)[0]

    @torch.no_grad()
    def sample_vjp(self, rndata_flat, query_pos, cotangent, latent_tokens_pos, chunk_points: Optional[int] = None) -> torch.Tensor:
        """The ADJOINT of ``sample``: -> grad_latent [M, C] (fp32) = sum_q cotangent[q] . d pred[q] / d rndata_flat, the vector-Jacobian
        product of the sampled field with respect to the latent for a cotangent [Nq, out_channels] -- the gradient of any number
        computed from sampled values (an integrated load sum_q a_q n_q p(x_q), a misfit at sensor points), which the autograd of
        ``GAOT3D.latent`` carries on into the encoder, the processor and the sample's coordinates.  The decoder's parameters and the
        query coordinates are CONSTANTS here (the derivative with respect to the query is ``sample_jacobian``'s).  ``sample_vjp_params`` returns
        the parameters' gradients as well (``GAOT3D.sample_autograd_params``).

        Streamed as ``sample`` is, ``chunk_points`` queries at a time through the same chunk loop: per chunk the lists
        (``knn_to_grid``, or ``graph.query_lists`` per scale), the GNO rows recomputed at fp32 arithmetic and mixed, the cotangent
        of the mixed rows through the projection (``_project_vjp``: z = x W_1^T + b_1, dh = (g W_2) * act'(z), dx = dh W_1 in row
        blocks), the scale mix's cotangent per scale (its softmax weights depend on the query only; on the 'knn' route the operands
        are equal and it is the weights' sum times the cotangent, formed as the forward forms it), then ``graph.by_source`` and the
        adjoint kernel (``IntegralTransform.adjoint_knn`` / ``adjoint_rows``: the per-edge kernel MLP evaluated forward once and
        reduced by TOKEN -- no MLP backward, no weight gradients, no ``gno_bwd``), and the chunk's [M, C] part added into the result
        in chunk order.  Nothing sized by Nq exists but the caller's own tensors.

        Exact fp32 in both precision modes (bf16 and fp32 mode give the same bits); outside autograd; bit-reproducible run to run
        for a given ``chunk_points``; NOT bit-identical across different ``chunk_points``, because a token's sum is split at the
        chunk boundaries (the difference is fp32 rounding of a sum).  The 'rows' route sizes its lists by a host read and raises
        GaotError inside a stream capture before any launch; capturing the 'knn' route is not promised.

        Routes and refusals are ``sample_hessian``'s / ``sample_hessian_rows``'s: 'knn' with k_neighbors in ``ops.GNO_KNN_K`` on the
        regular lists; 'radius', and 'bidirectional' with k_neighbors <= ``graph.QUERY_LIST_MAX_K``, on row lists.  use_attn, a decoder
        GeoEmbed, neighbour sampling, tokens off the regular grid, other k, the 'nonlinear' / 'nonlinear_kernelonly' transforms, a
        projection that is not two linear layers with a named activation, and a point-sharded model raise NotImplementedError naming
        the condition; 'reverse', a non-positive ``chunk_points`` and a cotangent that is not float32 [Nq, out_channels] on the queries'
        device raise ValueError."""
        return self._adjoint("sample_vjp", 0, rndata_flat, query_pos, [("the cotangent", cotangent, (), False)], latent_tokens_pos,
                             chunk_points)

    @torch.no_grad()
    def sample_vjp_params(self, rndata_flat, query_pos, cotangent, latent_tokens_pos, chunk_points: Optional[int] = None):
        """``sample_vjp`` WITH the decoder's parameters: -> (grad_latent [M, C] (fp32), grads), ``grads`` a dict keyed as
        ``named_parameters()`` keys them that holds, for EVERY parameter of this decoder, sum_q cotangent[q] . d pred[q] / d parameter
        in fp32 -- what trains the decoder through the streamed field, at the memory of one chunk.

        The chunk loop, the checks and the refusals are ``sample_vjp``'s (``_adjoint`` at order 0).  Per chunk: the lists and the GNO
        rows recomputed and mixed as ``_adjoint_chunk`` does; the projection's backward -- ONE ``ops.mlp2_backward_f32`` launch over the
        chunk's rows for the erf-GELU family 32 -> {64, 128, 256} -> 1..4 (the hidden layer never reaches memory), else the GEMM chain
        in the row blocks of ``_project_cot`` (``ops.gemm_dw`` / ``ops.colsum`` / ``ops.act_bwd``), d_b2 by ``ops.colsum``; the scale
        mix's cotangent, whose ``dlogits`` (``ops.scale_mix_bwd``) go on through the 3 -> 16 -> scales weighting MLP on row lists;
        ``graph.by_source``; then per scale and 32-channel pass of ``_fused_passes`` ONE exact-fp32 ``ops.gno_backward`` launch, which
        gives the kernel MLP's weight gradients and the latent's part together (``gaot_gno_adj`` is not run here), padded and cut as
        ``GnoFn``'s passes are.  On a regular list the by-query offsets are q k.  The chunk's parts are added in fp32 and in chunk
        order into ``grad_latent`` and one accumulator per parameter.

        On the 'knn' route every scale sees the same list: the mix is of EQUAL operands, sum_s w_s = 1 whatever the logits, so the
        gradient of the scale-weighting MLP is identically zero and its entries are exact zeros.

        Exact fp32 in both precision modes (the same bits), outside autograd, bit-reproducible for a given ``chunk_points``, NOT
        bit-identical across chunkings; ``grad_latent`` is not bit-identical to ``sample_vjp``'s (another kernel, another order of
        summation).  Refusals are ``sample_vjp``'s, and a kernel MLP with four hidden layers raises NotImplementedError (the exact-fp32
        ``gaot_gno_bwd`` has no such instantiation); everything is refused before any launch."""
        from ... import ops
        fn = "sample_vjp_params"
        self._sample_args(fn, chunk_points)
        self._check_cotangents(fn, query_pos, [("the cotangent", cotangent, (), False)])
        self._param_adjoint_layers(fn)
        grid, chunk, rows = self._adjoint_stream(fn, 0, rndata_flat, query_pos, latent_tokens_pos, chunk_points,
                                                 "the adjoint of the sampled field with the decoder's parameters")
        rndata_flat, query_pos, cot = rndata_flat.detach(), query_pos.detach(), cotangent.detach().contiguous()
        names = {id(p): name for name, p in self.named_parameters()}
        grads = {name: torch.zeros(p.shape, dtype=torch.float32, device=p.device) for name, p in self.named_parameters()}

        def add(p, g):
            if p is not None:
                grads[names[id(p)]].add_(g.reshape(p.shape))

        with ops.fp32_arithmetic():
            f = rndata_flat.to(torch.float32).contiguous()
            grad = torch.zeros_like(f)
            for sl, q, lists in self._stream_chunks(grid, query_pos, chunk, "rows" if rows else "knn", lead=False):
                grad.add_(self._param_adjoint_chunk(f, q.contiguous(), cot[sl], latent_tokens_pos, lists, add))
        return grad, grads

    def _param_adjoint_layers(self, fn) -> None:
        """the refusal ``sample_vjp_params`` adds to ``sample_vjp``'s: the kernel MLP's gradients come from the exact-fp32
        ``gaot_gno_bwd``, which is instantiated for one to three hidden layers"""
        nfc = len(list(self.gno.channel_mlp.fcs))
        if nfc > 4:
            raise NotImplementedError(f"MAGNODecoder.{fn}: the decoder's parameter gradients with a kernel MLP of {nfc - 1} hidden layers "
                                      "are not supported: the exact-fp32 backward of the transform (gaot_gno_bwd) takes three at most")

    def _project_bwd(self, x, g, add, fused: bool = True):
        """the projection's backward for ``sample_vjp_params``: -> dx [rows, C]; the gradients of its parameters go to ``add``.  One
        ``ops.mlp2_backward_f32`` launch when the fused kernel takes the shape, else (or with ``fused`` False: the measurement's other
        side) the GEMM chain in ``_project_cot``'s row blocks with the blocks' weight gradients added in block order."""
        from ... import ops
        fc1, fc2 = self.projection.fcs
        w1, w2 = GF._w2d(fc1.weight).detach().contiguous(), GF._w2d(fc2.weight).detach().contiguous()
        act = ops.ACT[self.projection.non_linearity]
        n, c = x.shape
        hid, oc = w1.shape[0], w2.shape[0]
        if fc2.bias is not None:
            add(fc2.bias, ops.colsum(g, n, oc, oc))
        if fused and act == ops.ACT["gelu"] and fc1.bias is not None and ops.mlp2_bwd_f32_supported(c, hid, oc, act):
            dx, dw1, db1, dw2 = ops.mlp2_backward_f32(x, w1, fc1.bias.detach().contiguous(), w2, g)
            add(fc1.weight, dw1), add(fc1.bias, db1), add(fc2.weight, dw2)
            return dx
        dx = torch.empty_like(x)
        step = n if hid <= c else max(1024, n * c // hid)
        for j in range(0, n, step):
            xb, gb = x[j:j + step], g[j:j + step]
            m = xb.shape[0]
            if act > 3:
                z = ops.gemm(xb, w1, m, hid, c, c, c, False, True, fc1.bias, 0, precision=0)
                h = ops.act_fwd(z, act)
            elif act:
                h, z = ops.gemm(xb, w1, m, hid, c, c, c, False, True, fc1.bias, act, want_preact=True, precision=0)
            else:
                h = z = ops.gemm(xb, w1, m, hid, c, c, c, False, True, fc1.bias, 0, precision=0)
            if oc == 1:     # the wide dimension on the tile rows (LinearFn.backward)
                add(fc2.weight, ops.gemm_dw(h, gb, hid, 1, m, hid, 1, precision=0))
            else:
                add(fc2.weight, ops.gemm_dw(gb, h, oc, hid, m, oc, hid, precision=0))
            del h
            a = ops.gemm(gb, w2, m, hid, oc, oc, hid, False, False, precision=0)
            dz = ops.act_bwd(z, a, act) if act else a
            del z, a
            add(fc1.weight, ops.gemm_dw(dz, xb, hid, c, m, hid, c, precision=0))
            if fc1.bias is not None:
                add(fc1.bias, ops.colsum(dz, m, hid, hid))
            ops.gemm(dz, w1, m, c, hid, hid, c, False, False, out=dx[j:j + step], ldc=c, precision=0)
            del dz
        return dx

    def _scale_weighting_bwd(self, q, dlogits, add) -> None:
        """the cotangent ``dlogits`` [n, scales] of the scale weights' logits l = W_2 relu(W_1 q + b_1) + b_2 carried into the four
        parameters of the weighting MLP: two ``gemm_dw``, two ``colsum`` and the ReLU mask (relu'(h) read from h itself)"""
        from ... import ops
        sw = self.scale_weighting
        n, ns = dlogits.shape
        w1, w2 = sw[0].weight.detach().contiguous(), sw[2].weight.detach().contiguous()
        hd, cd = w1.shape
        h = _scale_logits(self, q)[1].contiguous()
        dl = dlogits.contiguous()
        add(sw[2].weight, ops.gemm_dw(dl, h, ns, hd, n, ns, hd, precision=0))
        add(sw[2].bias, ops.colsum(dl, n, ns, ns))
        dh = ops.gemm(dl, w2, n, hd, ns, ns, hd, False, False, precision=0)
        dz = ops.act_bwd(h, dh, ops.ACT["relu"])
        add(sw[0].weight, ops.gemm_dw(dz, q, hd, cd, n, hd, cd, precision=0))
        add(sw[0].bias, ops.colsum(dz, n, hd, hd))

    def _param_adjoint_chunk(self, rndata_flat, q, cot, lat, lists, add):
        """One chunk of ``sample_vjp_params`` -> its [M, C] part of the latent's gradient; the chunk's parameter gradients go to
        ``add``.  A call of its own, so that a chunk's rows and lists are freed before the next chunk's are allocated."""
        from ... import graph as device_graph
        from ... import ops
        m, knn = lat.shape[0], isinstance(lists, tuple)
        outs = w = None
        if knn:
            x = self._mix_equal_scales([self.gno.forward_knn(lat, q, *lists, rndata_flat)], q)[0]
        else:
            outs = [self.gno(y_pos=lat, x_pos=q, edge_index=None, f_y=rndata_flat, graph=rows) for rows in lists]
            if len(outs) > 1 and self.use_scale_weights:
                outs = [o.contiguous() for o in outs]
                x, w = ops.scale_mix_fwd(outs, _scale_logits(self, q)[0].contiguous())
            else:
                x, outs = _mix_scales(self, outs, q), None
        d = self._project_bwd(x.contiguous(), cot, add)
        del x
        if knn:
            per = self._mix_equal_scales([d], q)        # (sum_s w_s) d: the weighting MLP's gradient is identically zero
        elif w is not None:
            per, dlogits = ops.scale_mix_bwd(outs, w, d)
            self._scale_weighting_bwd(q, dlogits, add)
            del dlogits
        else:
            per = [d] * len(lists)
        del d, outs, w
        part = None
        for rows, g in zip([lists] if knn else lists, per):
            graph = device_graph.by_source(rows, m)
            if knn:                                      # a regular list: query q's edges are q k .. q k + k - 1 (only the offsets are read)
                n, k = int(q.shape[0]), int(lists[1])
                offs = torch.arange(0, (n + 1) * k, k, dtype=torch.int32, device=q.device)
                graph = ops.BipartiteGraph(ops.SortedEdges(offs, None, None, lists[0].reshape(-1), n), graph.by_src, m, n)
            p = self.gno._param_adjoint(lat, q, rndata_flat, g, graph, add)
            part = p if part is None else part.add_(p)
        return part

    # the projection activations ``sample_jacobian_vjp`` differentiates twice: act' and act'' as plain fp32 tensor operations
    JAC_VJP_ACTS = (None, "none", "gelu", "relu")

    @staticmethod
    def _act_jets(z, act):
        """(act'(z), act''(z)) for the names in ``JAC_VJP_ACTS``; None stands for a factor that is identically 1 (first) or 0 (second):
        gelu' = Phi(z) + z phi(z), gelu'' = phi(z) (2 - z^2); relu' = 1[z > 0], relu'' = 0"""
        if act in (None, "none"):
            return None, None
        if act == "relu":
            return (z > 0).to(z.dtype), None
        phi = torch.exp(-0.5 * z * z) * 0.3989422804014327
        return 0.5 * (1.0 + torch.erf(z * 0.7071067811865476)) + z * phi, phi * (2.0 - z * z)

    def _project_jac_vjp(self, planes, gy, gj):
        """The cotangent of the projection's input JET: for the mixed GNO planes ``planes`` = [x, x'_0, x'_1, x'_2] ([rows, C] each) and
        the cotangents ``gy`` [rows, out_channels] (or None) on y = W_2 act(z) + b_2 and ``gj`` [rows, out_channels, 3] on
        y'_d = W_2 (act'(z) * W_1 x'_d), z = W_1 x + b_1 -> [dx, dx'_0, dx'_1, dx'_2]:
            a = g_y W_2,  a_d = g_y'd W_2,  u_d = x'_d W_1^T
            dz = act'(z) * a + act''(z) * sum_d u_d * a_d,   dx = dz W_1;      du_d = act'(z) * a_d,   dx'_d = du_d W_1
        Exact fp32: three GEMMs per row block on the four planes STACKED ([4 rows, .]: one launch per product, precision 0) and the
        elementwise middle as plain fp32 tensor operations (``_act_jets``).  Rows in blocks sized as in ``_project_vjp``."""
        return self._project_cot(1, planes, gy, gj)

    @torch.no_grad()
    def sample_jacobian_vjp(self, rndata_flat, query_pos, cot_pred, cot_jac, latent_tokens_pos,
                            chunk_points: Optional[int] = None) -> torch.Tensor:
        """The ADJOINT of ``sample_jacobian(row_lists=True)``: -> grad_latent [M, C] (fp32)
            = sum_q cot_pred[q] . d pred[q] / d rndata_flat + sum_q cot_jac[q] . d jac[q] / d rndata_flat,
        the vector-Jacobian product of the sampled field AND its spatial derivative with respect to the latent -- the gradient of a
        loss on the field's derivative (a misfit of d p / d n against measured wall-normal gradients, a Sobolev term, a first-order
        PDE or boundary residual at collocation points), which the autograd of ``GAOT3D.latent`` carries on into the encoder, the
        processor and the sample's coordinates.  ``cot_pred``: float32 [Nq, out_channels], or None for a loss on the derivative
        alone; ``cot_jac``: float32 [Nq, out_channels, 3].  The decoder's parameters and the query coordinates are CONSTANTS here.

        Streamed as ``sample_vjp`` is, through the same chunk loop.  Per chunk: the lists; the mixed value and three tangent planes
        recomputed at fp32 (``_jet_planes``, as ``sample_jacobian`` forms them; on row lists with the tangents of the scale weights);
        the cotangent of that jet through the projection (``_project_jac_vjp``: it needs act'' -- gelu'' = phi(z)(2 - z^2),
        relu'' = 0); the scale mix's cotangent (``knn``: equal operands, ``_mix_equal_scales`` on the four planes; row lists with
        softmax weights: G_s = w_s dx + sum_d w'_s,d dx'_d and J_s,d = w_s dx'_d, the weights being functions of the query alone);
        then per scale ``graph.by_source`` and the adjoint of the tangent kernel (``IntegralTransform.adjoint_jac_knn`` /
        ``adjoint_jac_rows``: value and three tangent chains through the per-edge MLP, contracted with the four cotangent planes and
        reduced by TOKEN -- no MLP backward, no weight gradients, no ``gno_bwd``), and the chunk's [M, C] part added in chunk order.
        Nothing sized by Nq exists but the caller's own tensors.

        Exact fp32 in both precision modes (the same bits), outside autograd, bit-reproducible run to run for a given
        ``chunk_points``; not bit-identical across chunkings (a token's sum is split at the chunk boundaries).  Routes and refusals
        are ``sample_vjp``'s; in addition a projection activation outside ``JAC_VJP_ACTS`` raises NotImplementedError naming it, and
        cotangents of the wrong dtype, shape or device raise ValueError."""
        return self._adjoint("sample_jacobian_vjp", 1, rndata_flat, query_pos,
                             [("cot_pred", cot_pred, (), True), ("cot_jac", cot_jac, (3,), False)], latent_tokens_pos, chunk_points)

    def _project_lap_vjp(self, planes, gy, gj, gl):
        """The cotangent of the projection's input LAPLACIAN jet: for the mixed GNO planes ``planes`` = [x, x'_0, x'_1, x'_2, x''_0,
        x''_1, x''_2] ([rows, C] each; only the SUM of the three second-order planes enters) and the cotangents ``gy``
        [rows, out_channels] (or None) on y = W_2 a(z) + b_2, ``gj`` [rows, out_channels, 3] on y'_d = W_2 (a'(z) * u_d) and ``gl``
        [rows, out_channels] on Lap y = W_2 (a''(z) * sum_d u_d^2 + a'(z) * s), z = W_1 x + b_1, u_d = W_1 x'_d, s = W_1 sum_d x''_d
        -> [dx, dx'_0, dx'_1, dx'_2, dx''] (dx'' is the cotangent of EVERY x''_d):
            A = g_y W_2,  A_d = g_y'd W_2,  A_L = g_Lap W_2
            dz = a' A + a'' sum_d u_d A_d + (a''' sum_d u_d^2 + a'' s) A_L,   du_d = a' A_d + 2 a'' u_d A_L,   ds = a' A_L
            dx = dz W_1,  dx'_d = du_d W_1,  dx'' = ds W_1
        Exact fp32: three GEMMs per row block on the planes STACKED (one launch per product, precision 0) and the elementwise middle
        as ONE kernel (``ops.mlp2_lap_cot_mid``, erf-GELU: the only projection ``_jet2_stream`` admits), written over the cotangent
        stack.  Rows in blocks sized as in ``_project_jac_vjp``."""
        return self._project_cot(2, planes, gy, gj, gl)

    LAP_VJP_DIRS = HESSIAN_DIRS[:3]       # the three axes: D_v^2 along them sums to the Laplacian

    # ---- ONE host path for the three adjoints, by ``order``: 0 the value (``sample_vjp``), 1 and d/dx (``sample_jacobian_vjp``), 2 and
    # the Laplacian (``sample_laplacian_vjp``).  A step is shared where the orders run the same operations; where sharing it would
    # change an operation's rounding or its launch the order keeps its branch (bit-equality outranks uniformity).
    # order 3: the GENERAL second-order case -- nd directions (per query, or host values) with a cotangent on every first- and every
    # second-order plane (``sample_directional_vjp``, ``sample_hessian_vjp``).  A branch beside order 2, which stays as it is.
    ADJOINT_WHAT = ("the adjoint of the sampled field", "the adjoint of the field's Jacobian", "the adjoint of the field's Laplacian",
                    "the adjoint of the field's directional derivatives")

    def _project_cot(self, order, planes, gy, gj=None, gl=None):
        """The skeleton of ``_project_vjp`` / ``_project_jac_vjp`` / ``_project_lap_vjp`` (their docstrings hold the formulas): rows in
        blocks sized so that the [rows, projection_channels] tensors stay no larger than the planes; per block the planes STACKED,
        [z; u ...] = X W_1^T, [A ...] = G W_2, the elementwise middle, dX = mid W_1 (one GEMM launch per product, precision 0) and the
        stack taken apart -> the cotangent planes.  Per order: the stack -- [x], [x, x'_d], [x, x'_d, sum_d x''_d] -- and the middle --
        ``ops.act_bwd`` on z with b_1 from the GEMM's epilogue; the torch expressions of ``_act_jets`` after z += b_1; the one kernel
        ``ops.mlp2_lap_cot_mid``, which adds b_1 itself.  The one plane of order 0 is read and written in place (no stack).
        Order 3 (``planes`` = [x, x'_0.., x''_0..] along nd directions, ``gj`` / ``gl`` [rows, out_channels, nd] on y'_i / y''_i): the
        stack of all 1 + 2 nd planes, the middle ``ops.mlp2_jet2_cot_mid``
            dz = a' A + a'' sum_i u_i A_i + sum_i (a''' u_i^2 + a'' s_i) B_i,   du_i = a' A_i + 2 a'' u_i B_i,   ds_i = a' B_i
        and a block of rows cut so that a [rows, hidden] stack is never larger than order 2's five planes' worth (5 n C floats: at
        nd = 6, 13 planes, a block is 5/13 of order 2's)."""
        from ... import ops
        fc1, fc2 = self.projection.fcs
        w1, w2 = GF._w2d(fc1.weight).contiguous(), GF._w2d(fc2.weight).contiguous()
        act = self.projection.non_linearity
        n, c = planes[0].shape
        hid, oc = w1.shape[0], w2.shape[0]
        npl = len(planes) if order == 3 else (1, 4, 5)[order]
        nd = (npl - 1) // 2
        outs = [torch.empty_like(planes[0]) for _ in range(npl)]
        step = n if hid <= c else max(1024, n * c // hid)
        if order == 3 and npl > 5:                       # the stacks [npl rows, hidden] stay within order 2's bound
            step = max(1024, step * 5 // npl)
        b1 = fc1.bias.detach().to(torch.float32).contiguous() if order >= 2 else None
        for j in range(0, n, step):
            sl = slice(j, j + step)
            m = planes[0][sl].shape[0]
            if order == 0:
                x, g, ng = planes[0][sl], gy[sl], 1
            elif order == 3:
                g = [gj[sl, :, i] for i in range(nd)] + [gl[sl, :, i] for i in range(nd)]
                if gy is not None:
                    g.insert(0, gy[sl])
                x, g, ng = torch.cat([p[sl] for p in planes]), torch.cat(g), len(g)
            else:
                xs = [p[sl] for p in planes[:4]]
                if order == 2:
                    xs.append(torch.add(planes[4][sl] + planes[5][sl], planes[6][sl]))         # (x''_0 + x''_1) + x''_2
                g = [gj[sl, :, d] for d in range(3)] + ([gl[sl]] if order == 2 else [])
                if gy is not None or order == 1:         # order 1 always stacks a value plane; order 2 runs without the A plane
                    g.insert(0, gy[sl] if gy is not None else gj.new_zeros(m, oc))
                x, g, ng = torch.cat(xs), torch.cat(g), len(g)
                del xs
            zu = ops.gemm(x, w1, npl * m, hid, c, c, c, False, True, fc1.bias if order == 0 else None, precision=0)
            a = ops.gemm(g, w2, ng * m, hid, oc, oc, hid, False, False, precision=0)
            del x, g
            if order == 0:
                mid = ops.act_bwd(zu, a, ops.ACT[act]) if ops.ACT[act] else a
            elif order == 1:                             # a = [A; A_0; A_1; A_2] becomes [dz; du_0; du_1; du_2] in place
                z = zu[:m]
                if fc1.bias is not None:
                    z += fc1.bias
                d1, d2 = self._act_jets(z, act)
                if d2 is not None:
                    s = zu[m:2 * m] * a[m:2 * m]
                    for d in (1, 2):
                        s += zu[(1 + d) * m:(2 + d) * m] * a[(1 + d) * m:(2 + d) * m]
                    s *= d2
                del z
                zu = None
                if d1 is not None:
                    a.view(4, m, hid).mul_(d1)
                if d2 is not None:
                    a[:m] += s
                    del s
                mid = a
            elif order == 3:
                zu, a = zu.view(npl, m, hid), a.view(ng, m, hid)
                if gy is None:                           # no A plane: the result goes over the z stack
                    mid = ops.mlp2_jet2_cot_mid(zu, None, a, b1, out=zu)
                else:                                    # [A; A_i; B_i] becomes [dz; du_i; ds_i] in place
                    mid = ops.mlp2_jet2_cot_mid(zu, a[0], a[1:], b1, out=a)
                mid = mid.view(npl * m, hid)
            else:
                zu, a = zu.view(5, m, hid), a.view(ng, m, hid)
                if gy is None:                           # no A plane: the result goes over the z stack
                    mid = ops.mlp2_lap_cot_mid(zu, None, a[:3], a[3], b1, out=zu)
                else:                                    # [A; A_d; A_L] becomes [dz; du_d; ds] in place
                    mid = ops.mlp2_lap_cot_mid(zu, a[0], a[1:4], a[4], b1, out=a)
                mid = mid.view(5 * m, hid)
            dx = ops.gemm(mid, w1, npl * m, c, hid, hid, c, False, False, out=outs[0][sl] if order == 0 else None, ldc=c, precision=0)
            del zu, a, mid
            for p in range(npl if order else 0):
                outs[p][sl] = dx[p * m:(p + 1) * m]
        return outs

    def _check_cotangents(self, fn, query_pos, cots) -> None:
        """``cots``: (name, tensor, the shape's tail after [Nq, out_channels], may be None) per cotangent; ValueError unless each is
        float32, of that shape and on the queries' device"""
        nq = int(query_pos.shape[0])
        for name, cot, tail, optional in cots:
            if cot is None and optional:
                continue
            shape = (nq, self.out_channels, *tail)
            if not isinstance(cot, torch.Tensor) or cot.dtype != torch.float32 or cot.device != query_pos.device \
                    or tuple(cot.shape) != shape:
                got = f"{cot.dtype} {tuple(cot.shape)} on {cot.device}" if isinstance(cot, torch.Tensor) else type(cot).__name__
                raise ValueError(f"MAGNODecoder.{fn}: {name} must be float32 {list(shape)} on the queries' device "
                                 f"({query_pos.device}){' or None' if optional else ''}, got {got}")

    @torch.no_grad()
    def _adjoint_stream(self, fn, order, rndata_flat, query_pos, lat, chunk_points, what=None):
        """The refusals of the adjoint of ``order``, before anything runs -> (grid, chunk, rows: the route is the row lists'): the
        argument rules, a point-sharded model, at order 2 a transform that is not 'linear' (the forward's jets cover the others, so it
        is named before their conditions), the streaming conditions at fp32 arithmetic (``_jet2_stream``: with the jet kernels'
        projection at order 2, else the 'linear' transform and two linear layers around a named activation), at order 1 an activation
        whose second derivative is not written.  ``GAOT3D.sample_*_autograd`` refuse through it before their forward runs."""
        from ... import ops
        self._sample_args(fn, chunk_points)
        if getattr(self, "_shard_group", None) is not None:
            raise NotImplementedError(f"MAGNODecoder.{fn}: a point-sharded model is not supported (every rank would hold a partial sum)")
        what = what or self.ADJOINT_WHAT[order]
        if order >= 2 and self.gno.transform_type != "linear":
            raise NotImplementedError(f"MAGNODecoder.{fn}: {what} needs the 'linear' transform (the adjoint kernel is the linear "
                                      f"transform's); transform type {self.gno.transform_type!r} is not")
        rows = self.decoder_strategy != "knn"
        with ops.fp32_arithmetic():
            grid, chunk = self._jet2_stream(fn, rndata_flat.detach(), query_pos.detach(), lat, chunk_points, rows=rows, what=what,
                                            jets=order >= 2)
        if order == 1 and self.projection.non_linearity not in self.JAC_VJP_ACTS:
            raise NotImplementedError(f"MAGNODecoder.{fn}: the second derivative of the projection's activation "
                                      f"{self.projection.non_linearity!r} is not written (covered: {self.JAC_VJP_ACTS})")
        return grid, chunk, rows

    def _adjoint(self, fn, order, rndata_flat, query_pos, cots, lat, chunk_points, dirs=None, what=None):
        """The driver of ``sample_vjp`` / ``sample_jacobian_vjp`` / ``sample_laplacian_vjp`` (``cots`` as ``_check_cotangents`` takes
        them, in the order value, Jacobian, Laplacian): the checks, the refusals, then at fp32 arithmetic the chunk loop of ``sample``
        with every chunk's [M, C] part (``_adjoint_chunk``) added into the zeroed gradient in chunk order.  Order 3: ``cots`` = value, first-
        and second-order planes along ``dirs`` -- the per-query directions [Nq, nd, 3], cut per chunk, or host values [nd][3] --, each
        may be None but not all three; ``what`` names the call in the refusals."""
        from ... import ops
        self._sample_args(fn, chunk_points)
        self._check_cotangents(fn, query_pos, cots)
        if order == 3 and all(cot is None for _, cot, _, _ in cots):
            raise ValueError(f"MAGNODecoder.{fn}: {', '.join(name for name, _, _, _ in cots)} are all None: there is nothing to pull back")
        grid, chunk, rows = self._adjoint_stream(fn, order, rndata_flat, query_pos, lat, chunk_points, what)
        rndata_flat, query_pos = rndata_flat.detach(), query_pos.detach()
        cots = [None if cot is None else cot.detach() for _, cot, _, _ in cots]
        if order == 0:
            cots[0] = cots[0].contiguous()                # its GEMM reads the block's rows where they are
        if order == 2 and cots[1] is None:                # the stack of ``_project_lap_vjp`` always holds the three A_d planes
            cots[1] = torch.zeros(*cots[2].shape, 3, dtype=torch.float32, device=query_pos.device)
        if order == 3:                                    # the stack of ``_project_cot`` always holds the A_i and the B_i planes
            shape = next(cot.shape for cot in cots[1:] + cots[:1] if cot is not None)
            for i in (1, 2):
                if cots[i] is None:
                    cots[i] = torch.zeros(*shape[:2], _num_dirs(dirs), dtype=torch.float32, device=query_pos.device)
        qd = isinstance(dirs, torch.Tensor)
        with ops.fp32_arithmetic():
            f = rndata_flat.to(torch.float32).contiguous()
            grad = torch.zeros_like(f)
            for sl, q, lists in self._stream_chunks(grid, query_pos, chunk, "rows" if rows else "knn", lead=False):
                grad.add_(self._adjoint_chunk(order, f, q.contiguous(), [None if cot is None else cot[sl] for cot in cots], lat, lists,
                                              dirs[sl] if qd else dirs))
        return grad

    def _adjoint_chunk(self, order, rndata_flat, q, cots, lat, lists, dirs=None):
        """One chunk of ``_adjoint`` -> its [M, C] part of the latent's gradient: the mixed planes recomputed -- at order 0 on the value
        route (``forward_knn`` / the fused forward on the rows; on row lists with softmax weights through ``ops.scale_mix_fwd``, which
        hands its weights to the mix's cotangent kernel), else ``_jet_planes`` --, the projection's cotangent (``_project_cot``), the
        scale mix's (``_mix_cot``), then per scale ``graph.by_source`` and the transform's adjoint, the parts added in scale order.
        A call of its own, so that a chunk's planes and lists are freed before the next chunk's are allocated."""
        from ... import graph as device_graph
        from ... import ops
        m, knn = lat.shape[0], isinstance(lists, tuple)
        if order != 3:
            dirs = self.LAP_VJP_DIRS if order == 2 else None
        qd = isinstance(dirs, torch.Tensor)               # order 3 with the chunk's per-query directions [n, nd, 3]: the ..._qd kernels
        outs = w = None
        if order:
            planes = self._jet_planes(rndata_flat, q, lat, lists, dirs)
        elif knn:
            planes = self._mix_equal_scales([self.gno.forward_knn(lat, q, *lists, rndata_flat)], q)
        else:
            outs = [self.gno(y_pos=lat, x_pos=q, edge_index=None, f_y=rndata_flat, graph=rows) for rows in lists]
            if len(outs) > 1 and self.use_scale_weights:
                outs = [o.contiguous() for o in outs]
                x, w = ops.scale_mix_fwd(outs, _scale_logits(self, q)[0].contiguous())
            else:
                x, outs = _mix_scales(self, outs, q), None
            planes = [x]
            del x
        d = self._project_cot(order, planes, *cots)
        del planes
        per = self._mix_cot(d, q, knn, outs, w, dirs if order == 3 else None)
        del d, outs, w
        part = None
        for rows, cot in zip([lists] if knn else lists, per):
            p = self.gno._adjoint(lat, q, cot, device_graph.by_source(rows, m), lists if knn else None, dirs, qd=qd)
            part = p if part is None else part.add_(p)
        return part

    def _mix_cot(self, d, q, knn, outs=None, w=None, dirs=None):
        """The scale mix's cotangent.  ``d`` = [G], [G, G'_0, G'_1, G'_2] or [G, G'_d ..., L]: the cotangents of the mixed value, of its
        derivative along the three axes and of EVERY second-order plane -> per scale (ONE entry on the 'knn' route) the planes as the
        transform's adjoint takes them, [G_s], [G_s, G'_s [3, n, C]] or [G_s, G'_s, L_s [1, n, C]].
        'knn': every scale sees the same list, the mix is of equal operands and the jets of its weights drop out
        (``_mix_equal_scales`` on every plane: (sum_s w_s) G, formed as the forward forms sum_s w_s x).  One scale, or summed
        scales: every scale gets the planes as they are.  Softmax weights on row lists: with x = sum_s w_s o_s,
        x'_d = sum_s (w_s o'_s,d + w'_s,d o_s), x''_d = sum_s (w_s o''_s,d + 2 w'_s,d o'_s,d + w''_s,d o_s) and w = softmax(l(q)) a
        function of the query alone,
            G_s = w_s G + sum_d w'_s,d G'_d + (sum_d w''_s,d) L,   G'_s,d = w_s G'_d + 2 w'_s,d L,   L_s = w_s L
        without the terms in L at order 1; at order 0, G_s = w_s G alone, it is the mix kernel's own backward on its operands
        ``outs`` and weights ``w`` (``ops.scale_mix_bwd``).
        With ``dirs`` (order 3: per-row directions [n, nd, 3] or host values [nd][3]) ``d`` = [G, P_0.., S_0..] holds a cotangent per
        first- and per second-order plane -> [G_s, P_s [nd, n, C], S_s [nd, n, C]]; with w'_s,i and w''_s,i the derivatives of the
        weights along direction i (``_logit_tangent_along``, ``_softmax_weight_jets``) the transposes of ``_mix_jet2_planes`` are
            G_s = w_s G + sum_i w'_s,i P_i + sum_i w''_s,i S_i,   P_s,i = w_s P_i + 2 w'_s,i S_i,   S_s,i = w_s S_i"""
        from ... import ops
        nd = 0 if dirs is None else _num_dirs(dirs)
        if nd:
            pack = lambda g, *t: [g, torch.stack(t[:nd]), torch.stack(t[nd:])]
        else:
            pack = lambda g, *t: [g] + ([torch.stack(t[:3])] if t else []) + [p.unsqueeze(0) for p in t[3:]]
        ns = len(self.scales)
        if knn:
            return [pack(*self._mix_equal_scales(d, q))]
        if ns == 1 or not self.use_scale_weights:
            return [pack(*d)] * ns
        if len(d) == 1:
            return [[g] for g in ops.scale_mix_bwd(outs, w, d[0])[0]]
        second = len(d) == 5 or nd > 0
        sw = self.scale_weighting
        logits, hdn = _scale_logits(self, q)
        w = torch.softmax(logits, dim=1)
        dls = _logit_tangents((hdn > 0).to(hdn.dtype), sw[0].weight, sw[2].weight, lambda x, wt: GF.linear(x, wt, None, precision=0))
        if nd:
            jets = [_softmax_weight_jets(w, _logit_tangent_along(dls, dirs, i, w), second=True) for i in range(nd)]
            per = []
            for s in range(ns):
                ws = w[:, s:s + 1]
                g = ws * d[0]
                for i, (dw, ddw) in enumerate(jets):
                    g += dw[:, s:s + 1] * d[1 + i]
                    g += ddw[:, s:s + 1] * d[1 + nd + i]
                per.append(pack(g, *(ws * d[1 + i] + (2.0 * jets[i][0][:, s:s + 1]) * d[1 + nd + i] for i in range(nd)),
                                *(ws * d[1 + nd + i] for i in range(nd))))
            return per
        jets = [_softmax_weight_jets(w, dl, second=second) for dl in dls]
        dws = [j[0] for j in jets]
        if second:
            lw = torch.add(jets[0][1] + jets[1][1], jets[2][1])          # the Laplacian of the weights
        per = []
        for s in range(ns):
            ws = w[:, s:s + 1]
            g = ws * d[0]
            for di, dw in enumerate(dws):
                g += dw[:, s:s + 1] * d[1 + di]
            if not second:
                per.append(pack(g, *(ws * d[1 + di] for di in range(3))))
                continue
            g += lw[:, s:s + 1] * d[4]
            per.append(pack(g, *(ws * d[1 + di] + (2.0 * dws[di][:, s:s + 1]) * d[4] for di in range(3)), ws * d[4]))
        return per

    @torch.no_grad()
    def sample_laplacian_vjp(self, rndata_flat, query_pos, cot_pred, cot_jac, cot_lap, latent_tokens_pos,
                             chunk_points: Optional[int] = None) -> torch.Tensor:
        """The ADJOINT of the field's value, spatial derivative AND Laplacian: -> grad_latent [M, C] (fp32)
            = sum_q cot_pred[q] . d pred[q] / d rndata_flat + sum_q cot_jac[q] . d jac[q] / d rndata_flat
              + sum_q cot_lap[q] . d lap[q] / d rndata_flat,
        the vector-Jacobian product of ``sample_laplacian`` / ``sample_laplacian_rows`` (and of the derivative planes of
        ``sample_hessian`` / ``sample_hessian_rows``) with respect to the latent -- the gradient of a loss on a PDE residual at
        collocation points (a Poisson residual Lap p - s, a diffusion term nu Lap u, a convection-diffusion residual), which the
        autograd of ``GAOT3D.latent`` carries on into the encoder, the processor and the sample's coordinates.  ``cot_pred``: float32
        [Nq, out_channels] or None; ``cot_jac``: float32 [Nq, out_channels, 3] or None; ``cot_lap``: float32 [Nq, out_channels].  The
        decoder's parameters and the query coordinates are CONSTANTS here.

        Streamed as ``sample_jacobian_vjp`` is, through the same chunk loop.  Per chunk: the lists; the mixed value, first- and
        second-order planes along the three axes recomputed at fp32 (``_jet_planes``, as ``sample_laplacian`` forms them; on row
        lists with the jets of the scale weights); the cotangent of that jet through the projection (``_project_lap_vjp``: a''' of the
        erf-GELU, the elementwise middle one kernel); the scale mix's cotangent (``knn``: equal operands, ``_mix_equal_scales`` on the
        five planes; row lists with softmax weights: G_s = w_s G + sum_d w'_s,d G'_d + Lap w_s L, G'_s,d = w_s G'_d + 2 w'_s,d L and
        L_s = w_s L, the weights being functions of the query alone); then per scale ``graph.by_source`` and the adjoint of the jet
        kernel (``IntegralTransform.adjoint_jet2_knn`` / ``adjoint_jet2_rows`` along the three axes, ONE second-order cotangent plane
        shared by the three directions), and the chunk's [M, C] part added in chunk order.

        Exact fp32 in both precision modes (the same bits), outside autograd, bit-reproducible run to run for a given
        ``chunk_points``; not bit-identical across chunkings (a token's sum is split at the chunk boundaries).  Refusals are
        ``sample_laplacian``'s ('knn') / ``sample_laplacian_rows``'s ('radius', 'bidirectional'); in addition a transform that is not
        'linear' and a point-sharded model raise NotImplementedError naming it, cotangents of the wrong dtype, shape or device raise
        ValueError, and on row lists (sized by a host read) the call raises GaotError inside a stream capture before any launch."""
        return self._adjoint("sample_laplacian_vjp", 2, rndata_flat, query_pos,
                             [("cot_pred", cot_pred, (), True), ("cot_jac", cot_jac, (3,), True), ("cot_lap", cot_lap, (), False)],
                             latent_tokens_pos, chunk_points)

    @torch.no_grad()
    def sample_directional_vjp(self, rndata_flat, query_pos, dirs, cot_pred, cot_d1, cot_d2, latent_tokens_pos,
                               chunk_points: Optional[int] = None) -> torch.Tensor:
        """The ADJOINT of ``sample_directional``: -> grad_latent [M, C] (fp32)
            = sum_q cot_pred[q] . d pred[q] / d rndata_flat + sum_q,i cot_d1[q, :, i] . d d1[q, :, i] / d rndata_flat
              + sum_q,i cot_d2[q, :, i] . d d2[q, :, i] / d rndata_flat
        for the derivatives along every query's OWN directions -- the gradient of a loss on d^2 p / d n^2 (a curvature or
        second-normal-derivative term of a wall model), of a boundary-layer residual in a local frame (n, t_1, t_2), of the tangential
        Laplacian D^2_{t1} + D^2_{t2}.  ``dirs``: float32 [Nq, nd, 3] or [Nq, 3] on the queries' device, 1 <= nd <= 6, used as given
        (``sample_directional``'s rules); ``cot_pred``: float32 [Nq, out_channels] or None; ``cot_d1`` / ``cot_d2``: float32
        [Nq, out_channels, nd], each may be None, but not all three.  The decoder's parameters, the query coordinates and the
        directions are CONSTANTS here.

        Streamed through the chunk loop of ``sample_laplacian_vjp``, as its general second-order case (order 3 of ``_adjoint``): per
        chunk the mixed planes [x, x'_i, x''_i] along the chunk's directions (``_jet_planes``: the ..._qd jet kernels), the
        projection's cotangent with a second-order cotangent per direction (``_project_cot``: one ``ops.mlp2_jet2_cot_mid`` between
        the GEMMs), the scale mix's (``_mix_cot``: on row lists with the weights' derivatives along every row's own direction), then
        per scale ``graph.by_source`` and the adjoint of the jet kernel with the direction of a pass loaded per lane
        (``IntegralTransform.adjoint_jet2_knn_qd`` / ``adjoint_jet2_rows_qd``: one value chain and two per direction -- 3 at nd = 1
        where the Laplacian's adjoint runs 7).  Exactness, reproducibility, routes and refusals are ``sample_laplacian_vjp``'s; a bad
        ``dirs`` and three None cotangents raise ValueError."""
        fn = "sample_directional_vjp"
        self._sample_args(fn, chunk_points)
        dirs = self._query_dirs(fn, dirs, query_pos)
        nd = int(dirs.shape[1])
        return self._adjoint(fn, 3, rndata_flat, query_pos,
                             [("cot_pred", cot_pred, (), True), ("cot_d1", cot_d1, (nd,), True), ("cot_d2", cot_d2, (nd,), True)],
                             latent_tokens_pos, chunk_points, dirs)

    HESSIAN_VJP_WHAT = "the adjoint of the field's Hessian"

    def _polarise_cot(self, cot_jac, cot_hess):
        """The transpose of ``_polarise``: the cotangents ``cot_jac`` [n, out_channels, 3] and ``cot_hess`` [n, out_channels, 3, 3] (each
        may be None) of its results as cotangents (P, S) [n, out_channels, 6] of the jets along ``HESSIAN_DIRS``.  ``_polarise`` writes
        jac = d1[..., :3], H_aa = d2_a and H_ab = H_ba = (d2_{3+n} - d2_a - d2_b) / 2 for pair n = (a, b), so with
        Cs = (C + C^T) / 2 the loss sum_ij C_ij H_ij is sum_a C_aa d2_a + sum_n Cs_ab (d2_{3+n} - d2_a - d2_b):
            P_a = cot_jac[..., a], P_{3+n} = 0;      S_a = C_aa - sum_{b != a} Cs_ab,      S_{3+n} = Cs_ab"""
        p = s = None
        if cot_jac is not None:
            p = cot_jac.new_zeros(*cot_jac.shape[:2], 6)
            p[:, :, :3] = cot_jac
        if cot_hess is not None:
            sym = 0.5 * (cot_hess + cot_hess.transpose(2, 3))
            s = sym.new_empty(*sym.shape[:2], 6)
            for a in range(3):
                s[:, :, a] = sym[:, :, a, a]
            for n, (a, b) in enumerate(self.HESSIAN_PAIRS):
                s[:, :, 3 + n] = sym[:, :, a, b]
                s[:, :, a] -= sym[:, :, a, b]
                s[:, :, b] -= sym[:, :, a, b]
        return p, s

    @torch.no_grad()
    def sample_hessian_vjp(self, rndata_flat, query_pos, cot_pred, cot_jac, cot_hess, latent_tokens_pos,
                           chunk_points: Optional[int] = None) -> torch.Tensor:
        """The ADJOINT of ``sample_hessian`` / ``sample_hessian_rows``: -> grad_latent [M, C] (fp32)
            = sum_q cot_pred[q] . d pred[q] / d rndata_flat + sum_q cot_jac[q] . d jac[q] / d rndata_flat
              + sum_q cot_hess[q] . d hess[q] / d rndata_flat
        -- the gradient of a loss on mixed second derivatives (the divergence of a viscous stress, a strain-rate term, any
        second-order residual that is not the Laplacian).  ``cot_pred``: float32 [Nq, out_channels]; ``cot_jac``: [Nq, out_channels, 3];
        ``cot_hess``: [Nq, out_channels, 3, 3] (need not be symmetric: hess[..., i, j] and hess[..., j, i] are one value, and the two
        cotangents add); each may be None, but not all three.

        The cotangents go through the transpose of the polarisation (``_polarise_cot``) and the call runs as the general
        second-order adjoint along the six host directions ``HESSIAN_DIRS`` (order 3 of ``_adjoint``, the host-direction jet adjoint
        ``IntegralTransform.adjoint_jet2_knn`` / ``adjoint_jet2_rows`` with a second-order plane per direction: 13 chains through the
        per-edge MLP; the three first-order planes of the sum directions carry zeros and are not skipped).  Exactness, reproducibility,
        routes and refusals are ``sample_laplacian_vjp``'s."""
        fn = "sample_hessian_vjp"
        self._sample_args(fn, chunk_points)
        cots = [("cot_pred", cot_pred, (), True), ("cot_jac", cot_jac, (3,), True), ("cot_hess", cot_hess, (3, 3), True)]
        self._check_cotangents(fn, query_pos, cots)
        p, s = self._polarise_cot(cot_jac, cot_hess)
        return self._adjoint(fn, 3, rndata_flat, query_pos,
                             [("cot_pred", cot_pred, (), True), ("cot_jac", p, (6,), True), ("cot_hess", s, (6,), True)],
                             latent_tokens_pos, chunk_points, self.HESSIAN_DIRS, self.HESSIAN_VJP_WHAT)

    @torch.no_grad()
    def _laplacian_jets(self, fn, rndata_flat, query_pos, lat, chunk_points):
        """the forward of ``functional.SampleLaplacianLatentFn``: ONE jet pass along the three axes -> (pred [Nq, out_channels],
        jac [Nq, out_channels, 3], lap [Nq, out_channels]); pred and lap are ``sample_laplacian``'s / ``sample_laplacian_rows``'s and
        jac is ``sample_hessian``'s / ``sample_hessian_rows``'s bit for bit (a direction's planes depend on that direction alone)"""
        rows = self.decoder_strategy != "knn"
        rndata_flat, query_pos = rndata_flat.detach(), query_pos.detach()
        grid, chunk = self._jet2_stream(fn, rndata_flat, query_pos, lat, chunk_points, rows=rows)
        nq = int(query_pos.shape[0])
        pred, jac, lap = self._new(rndata_flat, nq), self._new(rndata_flat, nq, 3), self._new(rndata_flat, nq)
        for sl, q, lists in self._stream_chunks(grid, query_pos, chunk, "rows" if rows else "knn"):
            d1, d2 = self._jet2_chunk(rndata_flat, q, lat, lists, self.LAP_VJP_DIRS, pred[sl])
            jac[sl] = d1
            torch.add(d2[:, :, 0] + d2[:, :, 1], d2[:, :, 2], out=lap[sl])
        return pred, jac, lap

    def sample_jacobian(self, rndata_flat, query_pos, latent_tokens_pos, chunk_points: Optional[int] = None,
                        row_lists: bool = False):
        """``sample`` with the spatial derivative of the field: -> (pred [Nq, out_channels], jac [Nq, out_channels, coord_dim]) with
        jac[q, o, d] = d pred[q, o] / d query_pos[q, d], every query's neighbour list held fixed -- the derivative autograd returns
        through ``forward(query_coord_pos=...)``, where edges are built once and not differentiated.  It is valid almost everywhere
        and NOT defined across the surfaces where a query's neighbour list (its k nearest tokens, the tokens within its radius)
        changes.  ``chunk_points`` queries at a time into two preallocated results; neither ever requires grad.  Argument rules are
        ``sample``'s: 'reverse' and a non-positive ``chunk_points`` raise ValueError.

        STREAMING path -- the conditions of ``sample``'s 'knn' route (strategy 'knn', k_neighbors in ``ops.GNO_KNN_K``, tokens on the
        model's regular grid, no neighbour sampling, no decoder GeoEmbed, a transform ``_fused_plan`` accepts): forward mode.  Per chunk
        one ``knn_to_grid`` launch, one ``jacobian_knn`` launch per 32-channel pass (value and three tangent planes), the scale mix
        applied to the value and to every tangent plane with the same weights, and the projection MLP's tangent
        (``jvp_rows``).  Every scale sees the same list, so the mix is of EQUAL operands: the derivative of the softmax weights
        themselves multiplies sum_s dw_s = 0 and drops out.  No edge_index, no sorted lists, no autograd graph, no backward pass, no
        host synchronisation (capturable in a graph after one eager call, as ``sample``).  Everything on this path is exact fp32 in
        both precision modes: in bf16 mode ``pred`` is the fp32-kernel value and differs from ``sample``'s by bf16 rounding.
        ``row_lists=True`` (opt-in; without it every configuration runs the route it ran before the argument existed) streams the
        'radius' and 'bidirectional' decoders too, under exactly the conditions of ``sample``'s row-list route ('bidirectional':
        k_neighbors <= ``graph.QUERY_LIST_MAX_K``): per chunk and scale ``graph.query_lists`` writes the by-query list and
        ``jacobian_rows`` runs the tangent kernel on its ragged rows (two launches per 32-channel pass), then the scale mix WITH the
        tangent of its weights -- the scales see different lists, so sum_s (dw_s) out_s does not vanish (``_mix_scales_jet2`` at first
        order) -- and ``jvp_rows``.  Exact fp32 in both precision modes; ``pred`` is the fp32-mode result of ``sample`` with the queries
        in one piece, bit for bit.  The results do not depend on ``chunk_points``: a row that straddles two of the kernel's 32-edge
        tiles is summed from two partial sums, so every chunk's list is led by as many padding edges as put its rows against the
        tiles where the list of ALL queries would have them (``query_lists(..., lead=)``).  The lists are sized by a host read, so
        this route raises GaotError inside a stream capture, before any launch.  It differs from the autograd route by fp32
        rounding (forward against reverse mode).  The flag changes nothing for any other configuration.
        Every other configuration ('radius' / 'bidirectional' decoders without ``row_lists``) takes the AUTOGRAD route: per chunk ``forward``'s
        decoder on a detached copy of the chunk that requires grad, then one backward pass per output channel.  use_attn raises the
        NotImplementedError ``IntegralTransform`` raises for coordinate gradients; a 'statistical' decoder GeoEmbed couples all
        queries through its z-score, so a per-query Jacobian is not what that route returns: NotImplementedError."""
        chunk = self._sample_args("sample_jacobian", chunk_points)
        if self.use_geoembed and self.geoembed.method == "statistical":
            raise NotImplementedError("MAGNODecoder.sample_jacobian: a 'statistical' decoder GeoEmbed normalises over ALL query rows, "
                                      "which couples the queries; there is no per-query Jacobian")
        nq, cd = int(query_pos.shape[0]), int(query_pos.shape[1])
        lat = latent_tokens_pos
        rndata_flat = rndata_flat.detach()
        query_pos = query_pos.detach()
        pred, jac = self._new(rndata_flat, nq), self._new(rndata_flat, nq, cd)
        route = self._stream_route()
        if route == "rows" and not row_lists:
            route = None
        with torch.no_grad():               # the plan of the forward alone, as ``sample`` asks for it (four hidden layers stream in fp32 mode)
            grid = self._stream_grid(rndata_flat, query_pos, lat) if route else None
            if grid is not None:
                for sl, q, lists in self._stream_chunks(grid, query_pos, chunk, route):
                    planes = self._jet_planes(rndata_flat, q, lat, lists)
                    # the planes of the real directions only (a padded direction's plane is zero and has no column in ``jac``)
                    self.projection.jvp_rows(planes[0], planes[1:1 + cd], out=(pred[sl], jac[sl]))
                return pred, jac
        lat_bidx = torch.zeros(lat.shape[0], dtype=torch.long, device=lat.device)
        for i in range(0, nq, chunk):
            with torch.enable_grad():
                q = query_pos[i:i + chunk].clone().requires_grad_(True)
                q_bidx = torch.zeros(q.shape[0], dtype=torch.long, device=q.device)
                p = self._decode(rndata_flat, q, q_bidx, lat, lat_bidx, None, False)
                for o in range(self.out_channels):
                    (g,) = torch.autograd.grad(p[:, o].sum(), q, retain_graph=o + 1 < self.out_channels)
                    jac[i:i + chunk, o, :] = g
            pred[i:i + chunk] = p.detach()
        return pred, jac
