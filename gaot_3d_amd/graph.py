"""Neighbour-graph construction on the device: the reference's ``get_neighbor_strategy`` and friends
(src/model/layers/magno.py:116-295), which run torch_cluster knn / radius on the CPU, restated for latent tokens that
form a regular D x H x W grid (gaot_3d.py:35-46; the trainer's rescaled copy stat.py:238-252) and executed by the HIP
kernels of csrc/graph.hip through the C ABI.  Conventions kept: encoder edges are ``[phys_idx, latent_idx]``, decoder
edges ``[latent_idx, phys_idx]``; 'bidirectional' = coalesce(cat(knn, radius)); 'reverse' = flip of the *bidirectional*
encoder graph whatever the encoder strategy is (magno.py:263-273); pyg_radius keeps at most 32 neighbours per centre
(magno.py:199, 259).  Outputs are int32 ``[2, E]`` tensors on the device (the on-disk dtype, stat.py:191, 208).

The only host synchronisations are the reads of list lengths (edge counts size the outputs); graph construction sits in
the data path, outside the captured training step.  No CPU fallback: a CPU tensor or an irregular token set raises."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

from . import _lib, ops
from ._lib import GaotError, check

Tensor = torch.Tensor
RADIUS_CAP = 32   # torch_cluster / PyG default max_num_neighbors (reference leaves it at the default)


class _Grid(C.Structure):   # gaot_grid_t
    _fields_ = [("dims", C.c_int32 * 3), ("lo", C.c_float * 3), ("hi", C.c_float * 3)]


@dataclass
class LatentGrid:
    dims: Tuple[int, int, int]
    lo: Tuple[float, float, float]
    hi: Tuple[float, float, float]
    pos: Tensor   # [D*H*W, 3] fp32 on the device: the coordinates distances are measured to

    @property
    def num_tokens(self) -> int:
        return self.dims[0] * self.dims[1] * self.dims[2]

    def c_struct(self) -> _Grid:
        return _Grid((C.c_int32 * 3)(*self.dims), (C.c_float * 3)(*self.lo), (C.c_float * 3)(*self.hi))


WINDOW_SLACK = 1e-4      # the relative slack of knn_grid_select's window test (csrc/graph.hip: bound * (1 - 1e-4))
_U = 2.0 ** -24          # fp32 unit roundoff


def grid_deviation_bound(dims: Sequence[int], slack: float = WINDOW_SLACK) -> float:
    """The largest distance, in units of the grid's smallest step, a stored token coordinate may lie from its ideal node
    ``lo + i * (hi - lo) / (n - 1)`` (exact arithmetic on the stored corner coordinates) for the grid kernels' lists to be exact.

    knn_grid_select stops at a window once ``kth < (bound * (1 - slack))^2``, where ``bound`` is the kernel's fp32 value of the
    distance D from the query to the nearest excluded grid PLANE (axis a, ideal position).  A token of that plane is at least
    ``D - delta`` away (delta: its deviation along axis a), and the kernel's value is at most ``(D + 5u |f| step_a)(1 + 4u)``:
    f = (p - lo) / step carries five roundings (p - lo; hi - lo, / (n - 1) and 1 / step behind inv_step; the product), the
    subtraction of the plane index and the product with step (two roundings behind it) four more.  dist2, bound * (1 - slack) and
    its square round too: another 4u relative.  The stop is therefore sound when
        delta + 5u |f| step_a <= (slack - 8u) D.
    Inside the box |f| <= C = n - 1 cells and D >= (1.5 - 5u C) step_a at the first window (w = 1; rint puts the query within half a
    cell of the base node, the excluded plane is two nodes from it); wider windows and queries outside the box raise D by at least
    as many cells as |f|, and slack - 8u > 5u.  With step_a >= step_min:
        delta / step_min <= (1.5 - 5u C)(slack - 8u) - 5u C,       C = the largest number of cells along one axis.
    At slack = 1e-4 that is 1.30e-4 for 64 nodes, 7.3e-5 for 256 and no longer positive beyond C = 500 cells: larger grids are
    not accepted.  (radius_grid_visit floors / ceils its window outwards: a whole cell of margin, nothing to add here.)"""
    c = max(int(v) for v in dims) - 1
    return (1.5 - 5 * _U * c) * (slack - 8 * _U) - 5 * _U * c


def as_latent_grid(latent_pos: Tensor, dims: Sequence[int], rtol: float = WINDOW_SLACK) -> LatentGrid:
    """Check that ``latent_pos [D*H*W, 3]`` is the reference's ``meshgrid(linspace, indexing='ij')`` grid (possibly
    rescaled per axis) and describe it.  Raises GaotError otherwise (no tree search on this path).

    Accepted: every stored coordinate within ``grid_deviation_bound(dims, rtol) * step_min`` of its ideal node, measured in fp64
    against the exact subdivision of the stored corners (``step_min``: the smallest step of an axis with more than one node).
    ``rtol`` is the slack the deviation budget is derived from; the kernels' own is WINDOW_SLACK, so a larger value is cut to
    it -- every grid accepted here gives exact lists."""
    d, h, w = (int(v) for v in dims)
    if latent_pos.dim() != 2 or latent_pos.shape[1] != 3 or latent_pos.shape[0] != d * h * w:
        raise GaotError(f"latent tokens {tuple(latent_pos.shape)} do not form a {d}x{h}x{w} grid")
    p = latent_pos.detach().to(torch.float32).contiguous()
    g = p.view(d, h, w, 3)
    lo = [float(g[0, 0, 0, a]) for a in range(3)]
    hi = [float(g[-1, -1, -1, a]) for a in range(3)]
    bad = any((n > 1 and not hi[a] > lo[a]) for a, n in enumerate((d, h, w)))
    steps = [(hi[a] - lo[a]) / (n - 1) for a, n in enumerate((d, h, w)) if n > 1]
    step_min = min(steps) if steps and not bad else 1.0      # a one-token grid has no step: the three coordinates must just agree
    tol = grid_deviation_bound((d, h, w), min(float(rtol), WINDOW_SLACK)) * step_min
    if not bad and tol > 0.0:
        ref = torch.stack(torch.meshgrid(*[lo[a] + torch.arange(n, device=p.device, dtype=torch.float64) * ((hi[a] - lo[a]) / max(n - 1, 1))
                                           for a, n in enumerate((d, h, w))], indexing="ij"), dim=-1)
        bad = not float((g.double() - ref).abs().max()) <= tol
    if bad or not tol > 0.0:
        raise GaotError("latent tokens are not a regular ascending meshgrid(linspace) grid: device graph construction "
                        "needs the reference's regular token grid")
    return LatentGrid((d, h, w), tuple(lo), tuple(hi), p)


@dataclass
class TokenSet:
    """latent tokens that are NOT a regular grid: searched by the brute-force device kernels (every point scans all tokens)"""
    pos: Tensor   # [M, 3] fp32 on the device

    @property
    def num_tokens(self) -> int:
        return int(self.pos.shape[0])


def _need_cuda(t: Tensor, what: str):
    if not t.is_cuda:
        raise GaotError(f"{what}: device graph construction runs on the HIP device only (got a {t.device} tensor)")


def exclusive_scan(x: Tensor) -> Tensor:
    """int32 [n] -> int32 [n+1] exclusive prefix sums (last element = total)"""
    lib = _lib.load()
    n = x.numel()
    out = torch.empty(n + 1, dtype=torch.int32, device=x.device)
    ws = torch.empty(max(lib.gaot_exclusive_scan_workspace_bytes(n), 16), dtype=torch.uint8, device=x.device)
    check(lib.gaot_exclusive_scan_i32(ops._ptr(x), n, ops._ptr(out), ops._ptr(ws), ws.numel(), ops._stream()),
          "gaot_exclusive_scan_i32")
    return out


def knn_to_grid(phys_pos: Tensor, grid: LatentGrid, k: int) -> Tensor:
    """int32 [N, k]: the k nearest tokens of every point, by (distance, token index)"""
    _need_cuda(phys_pos, "knn_to_grid")
    lib = _lib.load()
    p = phys_pos.detach().to(torch.float32).contiguous()
    out = torch.empty(p.shape[0], k, dtype=torch.int32, device=p.device)
    if isinstance(grid, TokenSet):
        check(lib.gaot_knn_brute(ops._ptr(p), p.shape[0], ops._ptr(grid.pos), grid.num_tokens, k, ops._ptr(out), ops._stream()),
              "gaot_knn_brute")
        return out
    gs = grid.c_struct()
    check(lib.gaot_knn_grid(ops._ptr(p), p.shape[0], C.byref(gs), ops._ptr(grid.pos), k, ops._ptr(out), ops._stream()),
          "gaot_knn_grid")
    return out


def radius_pairs(phys_pos: Tensor, grid: LatentGrid, radius: float, cap: Optional[int]) -> Tuple[Tensor, Tensor]:
    """(point_idx, token_idx) int32 lists of all pairs with d <= radius, grouped by point (ascending), tokens ascending
    inside a point, at most ``cap`` tokens per point (None: no cap)"""
    _need_cuda(phys_pos, "radius_pairs")
    lib = _lib.load()
    p = phys_pos.detach().to(torch.float32).contiguous()
    n = p.shape[0]
    brute = isinstance(grid, TokenSet)
    gs = None if brute else grid.c_struct()
    capv = int(cap) if cap is not None else 0x7fffffff
    counts = torch.empty(n, dtype=torch.int32, device=p.device)
    if brute:
        check(lib.gaot_radius_brute_count(ops._ptr(p), n, ops._ptr(grid.pos), grid.num_tokens, float(radius), capv,
                                          ops._ptr(counts), ops._stream()), "gaot_radius_brute_count")
    else:
        check(lib.gaot_radius_grid_count(ops._ptr(p), n, C.byref(gs), ops._ptr(grid.pos), float(radius), capv, ops._ptr(counts),
                                         ops._stream()), "gaot_radius_grid_count")
    offs = exclusive_scan(counts)
    total = int(offs[-1])     # host sync: sizes the output
    pt = torch.empty(total, dtype=torch.int32, device=p.device)
    tk = torch.empty(total, dtype=torch.int32, device=p.device)
    if total and brute:
        check(lib.gaot_radius_brute_fill(ops._ptr(p), n, ops._ptr(grid.pos), grid.num_tokens, float(radius), capv, ops._ptr(offs),
                                         ops._ptr(pt), ops._ptr(tk), ops._stream()), "gaot_radius_brute_fill")
    elif total:
        check(lib.gaot_radius_grid_fill(ops._ptr(p), n, C.byref(gs), ops._ptr(grid.pos), float(radius), capv, ops._ptr(offs),
                                        ops._ptr(pt), ops._ptr(tk), ops._stream()), "gaot_radius_grid_fill")
    return pt, tk


def _compact(a: Tensor, b: Tensor, flags: Tensor) -> Tuple[Tensor, Tensor]:
    lib = _lib.load()
    offs = exclusive_scan(flags)
    total = int(offs[-1])
    oa = torch.empty(total, dtype=torch.int32, device=a.device)
    ob = torch.empty(total, dtype=torch.int32, device=a.device)
    if total:
        check(lib.gaot_compact_pairs(ops._ptr(a), ops._ptr(b), ops._ptr(flags), ops._ptr(offs), a.numel(), ops._ptr(oa),
                                     ops._ptr(ob), ops._stream()), "gaot_compact_pairs")
    return oa, ob


def cap_per_key(key: Tensor, other: Tensor, num_keys: int, cap: int) -> Tuple[Tensor, Tensor]:
    """stable-sort (key, other) by key and keep the first ``cap`` entries of every key (pyg_radius' per-centre cap)"""
    lib = _lib.load()
    if key.numel() == 0:
        return key, other
    s = ops.csr_build(torch.stack([other, key]), 1, num_keys)
    flags = torch.empty(key.numel(), dtype=torch.int32, device=key.device)
    check(lib.gaot_segment_cap_flags(ops._ptr(s.rowptr), ops._ptr(s.key), key.numel(), int(cap), ops._ptr(flags), ops._stream()),
          "gaot_segment_cap_flags")
    return _compact(s.key, s.other, flags)


def apply_neighbor_sampling(edge_index: Tensor, num_query_nodes: int, device=None, sampling_strategy: Optional[str] = None,
                            max_neighbors: Optional[int] = None, sample_ratio: Optional[float] = None,
                            training: bool = True, seed: Optional[Tensor] = None) -> Tensor:
    """reference magno.py:297-371, same arguments (+ ``seed``: one-element int64 device tensor; default = the next
    word of the device seed stream, functional.next_dropout_seed).  'max_neighbors': every query keeps at most
    ``max_neighbors`` uniformly random edges (applied in training and eval alike, as in the reference); 'ratio': every
    edge is kept with probability ``sample_ratio`` in training mode.  The result is sorted by query (the reference keeps
    the input order; the operators downstream do not depend on it)."""
    if sampling_strategy is None:
        return edge_index
    if num_query_nodes == 0 or edge_index.shape[1] == 0:
        return edge_index
    if sampling_strategy == "max_neighbors":
        if max_neighbors is None:
            raise ValueError("max_neighbors must be provided when using 'max_neighbors' sampling strategy")
    elif sampling_strategy == "ratio":
        if sample_ratio is None:
            raise ValueError("sample_ratio must be provided when using 'ratio' sampling strategy")
        if sample_ratio >= 1.0 or not training:
            return edge_index
    else:
        raise ValueError(f"Invalid sampling strategy: {sampling_strategy}")
    _need_cuda(edge_index, "edge_index")
    lib = _lib.load()
    if seed is None:
        from .functional import next_dropout_seed
        seed = next_dropout_seed(edge_index.device)
    e = edge_index.shape[1]
    flags = torch.empty(e, dtype=torch.int32, device=edge_index.device)
    s = ops.csr_build(edge_index, 1, num_query_nodes)          # key = query, other = source
    if sampling_strategy == "max_neighbors":
        check(lib.gaot_segment_random_cap_flags(ops._ptr(seed), ops._ptr(s.rowptr), ops._ptr(s.key), e, int(max_neighbors),
                                                ops._ptr(flags), ops._stream()), "gaot_segment_random_cap_flags")
    else:
        check(lib.gaot_random_keep_flags(ops._ptr(seed), e, float(sample_ratio), ops._ptr(flags), ops._stream()),
              "gaot_random_keep_flags")
    q, src = _compact(s.key, s.other, flags)
    return torch.stack([src, q]).to(edge_index.dtype)


def coalesce(row0: Tensor, row1: Tensor, num_row0: int, num_row1: int) -> Tensor:
    """sort by (row0, row1) and drop duplicates -- torch_geometric.utils.coalesce as the reference uses it for
    'bidirectional' (magno.py:219-220): stable sort by row1, stable sort by row0, adjacent-unique, compact"""
    lib = _lib.load()
    if row0.numel() == 0:
        return torch.stack([row0, row1])
    s1 = ops.csr_build(torch.stack([row0, row1]), 1, num_row1)       # key = row1, other = row0
    s0 = ops.csr_build(torch.stack([s1.other, s1.key]), 0, num_row0)  # key = row0 (stable: row1 stays ascending)
    flags = torch.empty(row0.numel(), dtype=torch.int32, device=row0.device)
    check(lib.gaot_unique_pair_flags(ops._ptr(s0.key), ops._ptr(s0.other), row0.numel(), ops._ptr(flags), ops._stream()),
          "gaot_unique_pair_flags")
    a, b = _compact(s0.key, s0.other, flags)
    return torch.stack([a, b])


def _encoder_edges(strategy: str, p: Tensor, grid: LatentGrid, radius: float, k: int) -> Tensor:
    """[phys_idx, latent_idx] for one graph (magno.py:166-222)"""
    n, m = p.shape[0], grid.num_tokens
    knn = rad = None
    if strategy in ("knn", "bidirectional"):
        idx = knn_to_grid(p, grid, k)
        src = torch.arange(n, dtype=torch.int32, device=p.device).repeat_interleave(k)
        knn = torch.stack([src, idx.reshape(-1)])
    if strategy in ("radius", "bidirectional"):
        pt, tk = radius_pairs(p, grid, radius, None)          # every pair; the cap applies per TOKEN here
        tk2, pt2 = cap_per_key(tk, pt, m, RADIUS_CAP)          # grouped by token, points ascending, <= 32 per token
        rad = torch.stack([pt2, tk2])
    if strategy == "knn":
        return knn
    if strategy == "radius":
        return rad
    if strategy == "bidirectional":
        both = torch.cat([knn, rad], dim=1)
        return coalesce(both[0].contiguous(), both[1].contiguous(), n, m)
    raise ValueError(f"Unknown encoder strategy: {strategy}")


def _decoder_edges(strategy: str, p: Tensor, grid: LatentGrid, radius: float, k: int) -> Tensor:
    """[latent_idx, phys_idx] for one graph (magno.py:224-295)"""
    n, m = p.shape[0], grid.num_tokens
    if strategy == "reverse":
        return _encoder_edges("bidirectional", p, grid, radius, k).flip(0).contiguous()
    knn = rad = None
    if strategy in ("knn", "bidirectional"):
        idx = knn_to_grid(p, grid, k)
        dst = torch.arange(n, dtype=torch.int32, device=p.device).repeat_interleave(k)
        knn = torch.stack([idx.reshape(-1), dst])
    if strategy in ("radius", "bidirectional"):
        pt, tk = radius_pairs(p, grid, radius, RADIUS_CAP)    # points are the centres: <= 32 tokens per point
        rad = torch.stack([tk, pt])
    if strategy == "knn":
        return knn
    if strategy == "radius":
        return rad
    if strategy == "bidirectional":
        both = torch.cat([knn, rad], dim=1)
        return coalesce(both[0].contiguous(), both[1].contiguous(), m, n)
    raise ValueError(f"Unknown decoder strategy: {strategy}")


QUERY_LIST_STRATEGIES = ("radius", "bidirectional")
QUERY_LIST_MAX_K = 32     # the register-list capacities gaot_nbr_union_grid_* is instantiated for


def query_lists(strategy: str, query_pos: Tensor, grid: LatentGrid, radius: float, k: int, lead: int = 0) -> ops.BipartiteGraph:
    """The by-query neighbour list of a 'radius' or 'bidirectional' DECODER graph for one regular token grid, written row by row --
    what ``ops.csr_build(_decoder_edges(strategy, ...), 1, Nq)`` holds in ``rowptr`` / ``key`` / ``other``, without the edge list,
    ``coalesce`` or a sort.  Both neighbourhoods are defined per query ('radius': the tokens within ``radius``, the ``RADIUS_CAP``
    lowest ids; 'bidirectional': those united with the ``k`` nearest tokens), and ``coalesce`` followed by the stable sort by query
    leaves every query's tokens ascending without duplicates, so a row does not depend on the other queries.

    FORWARD ONLY: ``by_dst`` is ``SortedEdges(rowptr=offsets, perm=None, key=query ids, other=token ids)`` -- the three arrays the
    fused forward (``ops.gno_forward`` / ``ops.gno_nl_forward``) reads -- and ``by_src`` is None; a backward needs ``build_graph``.
    One host read of the total (it sizes the two id lists), as in ``radius_pairs``: raises while a stream is being captured.
    ``lead`` > 0 (``ops.gno_forward_jac`` alone reads such a list): the lists begin with ``lead`` PADDING edges (query id -1, token 0)
    and ``rowptr`` starts at ``lead``, so that a piece of a longer list can lie against the kernels' 32-edge tiles as it does there
    (``lead`` = the edges before it, modulo 32); the rows are written at their shifted offsets, nothing is copied."""
    if strategy not in QUERY_LIST_STRATEGIES:
        raise ValueError(f"query_lists: strategy must be one of {QUERY_LIST_STRATEGIES}, got {strategy!r}")
    _need_cuda(query_pos, "query_lists")
    if isinstance(grid, TokenSet):
        raise GaotError("query_lists: the tokens are not a regular grid (TokenSet); build the edge list (get_neighbor_strategy)")
    if torch.cuda.is_current_stream_capturing():
        raise GaotError(f"query_lists: a '{strategy}' neighbour list is sized by a host read of its length, which is illegal while a "
                        "stream is being captured; sample eagerly")
    union = strategy == "bidirectional"
    p = query_pos.detach().to(torch.float32).contiguous()
    if p.dim() != 2 or p.shape[1] != 3:
        raise GaotError(f"query_lists: query_pos must be [Nq, 3], got {tuple(p.shape)}")
    n, k = int(p.shape[0]), int(k)
    if not float(radius) > 0.0:
        raise GaotError(f"query_lists: radius must be positive, got {radius}")
    if union and not 1 <= k <= min(QUERY_LIST_MAX_K, grid.num_tokens):
        raise GaotError(f"query_lists: k must be in [1, min({QUERY_LIST_MAX_K}, number of tokens = {grid.num_tokens})], got {k}")
    if n * ((k if union else 0) + RADIUS_CAP) > 0x7fffffff:
        raise GaotError(f"query_lists: {n} queries x up to {(k if union else 0) + RADIUS_CAP} tokens is beyond int32; take the "
                        "queries in chunks")
    lib = _lib.load()
    counts = torch.empty(n, dtype=torch.int32, device=p.device)
    gs = grid.c_struct()
    head = (ops._ptr(p), n, C.byref(gs), ops._ptr(grid.pos)) + ((k,) if union else ()) + (float(radius), RADIUS_CAP)
    count, fill = (lib.gaot_nbr_union_grid_count, lib.gaot_nbr_union_grid_fill) if union else \
        (lib.gaot_radius_grid_count, lib.gaot_radius_grid_fill)
    what = "gaot_nbr_union_grid" if union else "gaot_radius_grid"
    if n:
        check(count(*head, ops._ptr(counts), ops._stream()), what + "_count")
    offs = exclusive_scan(counts)
    total = int(offs[-1])     # host sync: sizes the lists
    lead = int(lead)
    if lead < 0:
        raise GaotError(f"query_lists: lead must not be negative, got {lead}")
    qi = torch.empty(lead + total, dtype=torch.int32, device=p.device)
    tk = torch.empty(lead + total, dtype=torch.int32, device=p.device)
    if lead:
        offs = offs + lead
        qi[:lead] = -1
        tk[:lead] = 0
    if total:
        check(fill(*head, ops._ptr(offs), ops._ptr(qi), ops._ptr(tk), ops._stream()), what + "_fill")
    return ops.BipartiteGraph(ops.SortedEdges(offs, None, qi, tk, n), None, grid.num_tokens, n)


def by_source(lists, num_src: int) -> ops.BipartiteGraph:
    """The by-SOURCE list of a chunk of queries, which the adjoint (``ops.gno_adjoint``) reduces over: ``lists`` is the regular list
    (nbr, k) of ``knn_to_grid`` (nbr int32, [n, k] or flat) or the forward-only graph of ``query_lists`` (built WITHOUT ``lead``
    padding).  Forms the int32 [2, E] (source, query) pairs in by-query order and sorts them with the stable ``ops.csr_build(..., 0,
    num_src)``, so a source's queries come in ascending order.  -> a graph with ``by_src`` set; ``by_dst`` is the list given (None for
    a regular list, whose degree is the constant k)."""
    if isinstance(lists, tuple):
        nbr, k = lists[0], int(lists[1])
        _need_cuda(nbr, "by_source")
        if nbr.dtype != torch.int32 or k < 1 or nbr.numel() % k:
            raise GaotError(f"by_source: nbr must hold int32 ids, k per query (k = {k}), got {nbr.dtype} {tuple(nbr.shape)}")
        n = nbr.numel() // k
        qi = torch.arange(n, dtype=torch.int32, device=nbr.device).repeat_interleave(k)
        tk, by_dst = nbr.reshape(-1), None
    else:
        by_dst, n = lists.by_dst, lists.num_dst
        if int(num_src) != lists.num_src:
            raise GaotError(f"by_source: the lists were built for {lists.num_src} sources, got num_src = {num_src}")
        if by_dst.num_edges and int(by_dst.rowptr[0]) != 0:
            raise GaotError("by_source: the lists begin with padding edges (query_lists(..., lead=)); build them without")
        qi, tk = by_dst.key, by_dst.other
    return ops.BipartiteGraph(by_dst, ops.csr_build(torch.stack([tk, qi]), 0, int(num_src)), int(num_src), int(n))


def get_neighbor_strategy(neighbor_strategy: str, phys_pos: Tensor, batch_idx_phys: Optional[Tensor], latent_tokens_pos: Tensor,
                          batch_idx_latent: Optional[Tensor], radius: float, k_neighbors: int = 1, is_decoder: bool = False,
                          latent_dims: Optional[Sequence[int]] = None) -> Tensor:
    """Device version of the reference function of the same name (magno.py:116-164; same arguments plus the grid shape).
    ``latent_tokens_pos`` holds the tokens of every graph of the batch back to back (gaot_3d.py:283-285: the same grid
    tiled ``num_graphs`` times); ``batch_idx_*`` are the sorted PyG batch vectors (None = one graph)."""
    _need_cuda(phys_pos, "get_neighbor_strategy")
    lat = latent_tokens_pos.detach().to(phys_pos.device, torch.float32).contiguous()
    m = int(latent_dims[0]) * int(latent_dims[1]) * int(latent_dims[2]) if latent_dims is not None else 0
    regular = m > 0 and lat.shape[0] % m == 0 and lat.shape[0] > 0
    if regular:
        nb = lat.shape[0] // m
        lptr = [b * m for b in range(nb + 1)]
    else:   # any token set: the graphs of the batch are the runs of the (sorted) token batch vector
        if batch_idx_latent is None or batch_idx_latent.numel() == 0:
            nb, lptr = 1, [0, lat.shape[0]]
        else:
            nb = int(batch_idx_latent.max().item()) + 1
            lptr = [0] + torch.cumsum(torch.bincount(batch_idx_latent, minlength=nb), 0).tolist()
    if batch_idx_phys is None or nb == 1:
        ptr = [0, phys_pos.shape[0]]
    else:
        cnt = torch.bincount(batch_idx_phys, minlength=nb)
        ptr = [0] + torch.cumsum(cnt, 0).tolist()
    outs = []
    for b in range(nb):
        toks = lat[lptr[b]:lptr[b + 1]]
        grid = None
        if regular:
            try:
                grid = as_latent_grid(toks, latent_dims)
            except GaotError:
                grid = None
        if grid is None:   # not the reference's regular grid: brute-force kernels (csrc/graph.hip: k_knn_brute, k_radius_brute)
            grid = TokenSet(toks)
        p = phys_pos[ptr[b]:ptr[b + 1]]
        e = (_decoder_edges if is_decoder else _encoder_edges)(neighbor_strategy, p, grid, radius, k_neighbors)
        if b:
            inc = torch.tensor([[lptr[b]], [ptr[b]]] if is_decoder else [[ptr[b]], [lptr[b]]], dtype=torch.int32, device=e.device)
            e = e + inc
        outs.append(e)
    return outs[0] if nb == 1 else torch.cat(outs, dim=1)
