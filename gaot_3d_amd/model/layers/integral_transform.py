"""IntegralTransform with the reference's constructor/forward signature
(src/model/layers/integral_transform.py:31-40, 80-87).

Default configuration -- transform_type='linear', no attention weights, kernel MLP 6 -> 64 (x1..4) -> 32 -- runs the
fused HIP kernels (csrc/gno.hip, gno_bf16.hip, gno_bwd3_bf16.hip: no per-edge tensor ever reaches HBM).  So do
transform_type='nonlinear' and 'nonlinear_kernelonly' (kernel MLP 6 + C_in -> 64 (x1..4) -> C): the feature columns of the
first layer act on the SOURCE node only, so t = W_0f f_y is one per-node product ([N_y, 64], fp32) and the kernels start every
edge's first-layer accumulator from b_0 + t[src]; the backward returns dt[s] = sum of dz_0 over the edges of s, from which
dW_0f = dt^T f_y and grad f_y += dt W_0f follow as per-node products (the autograd of the linear that formed t).
use_attn=True (cosine / dot_product edge scores, softmax per query, weighted SUM) runs the same kernels in their WEIGHTED
instantiation (``_fused_attn_plan``, ``functional.GnoWFn``): out_q = sum_e alpha_e k_e f_y[s_e] with alpha [E] one fp32 scalar per
edge in the dst-sorted order (``_attn_weights``); the backward returns d alpha_e = sum_c g_c k_e,c f_y[s_e]_c beside the gradients
of f_y, t and the parameters, and autograd carries it through the softmax into the scores.  The dot-product scores are a bilinear
form of the endpoints' homogeneous coordinates (``attn_bilinear_form``, csrc/gno_attn.hip): a scalar per edge, no gathered [E, 64]
projection rows.  Coordinates that require grad are refused with use_attn.
Every other variant the reference offers (other MLP shapes, MLP dropout in training, f_y=None)
runs the general path: per-edge tensors in dst-sorted order, the MLP on the GEMM kernels, gather / segment /
element-wise glue and its autograd in csrc/edgeops.hip (gaot_3d_amd/edgeops.py), with the same ``_attn_weights`` under use_attn.
``forward_knn`` is the forward alone on a regular k-neighbour list (the [n, k] ids of ``graph.knn_to_grid`` as they stand, k | 32):
the same operands, one ``gaot_gno_fwd_knn`` launch per 32-channel pass, no edge list or sorted lists, bit-identical to ``forward`` on
the graph of those lists -- what ``MAGNODecoder.sample`` streams query chunks through.  ``jacobian_knn`` is ``forward_knn`` with the
derivative of its result with respect to the query coordinates, in forward mode (``gaot_gno_fwd_knn_jac``: three tangents through the
per-edge MLP beside the value, exact fp32) -- what ``MAGNODecoder.sample_jacobian`` streams.  ``jacobian_rows`` is the same on the
ragged by-query list of any graph (``gaot_gno_fwd_jac``: the tangent kernel finished by the forward's segmented walk and one fix-up
launch) -- what ``sample_jacobian(row_lists=True)`` streams for 'radius' / 'bidirectional' decoders.  ``jet2_knn`` and ``jet2_rows``
carry directional 2-jets (value, D_v, D_v^2) on the same two kinds of list (``gaot_gno_fwd_knn_jet2`` / ``gaot_gno_fwd_jet2``) -- what
``sample_hessian`` / ``sample_laplacian`` and their ``_rows`` variants stream; ``jet2_knn_qd`` and ``jet2_rows_qd`` carry them along a
direction set of every query's own (``gaot_gno_fwd_knn_jet2_qd`` / ``gaot_gno_fwd_jet2_qd``) -- what ``sample_directional`` streams.
``adjoint_knn`` / ``adjoint_rows`` are the ADJOINT of the 'linear' forward with respect to f_y on the by-source list of a chunk
(``gaot_gno_adj``: the per-edge MLP evaluated forward once and reduced by source, exact fp32, no weight gradients) -- what
``MAGNODecoder.sample_vjp`` streams.
HIP only, no CPU fallback."""
from typing import Optional

import torch
import torch.nn as nn

from ... import edgeops as EO
from ... import functional as GF
from ... import ops
from .mlp import LinearChannelMLP, activation_name


def _is_flip_of_encoder(cache_owner, slot, dec_ei: torch.Tensor, enc_ei: torch.Tensor) -> bool:
    """Is this decoder edge list the encoder's with its two rows swapped (the shipped configuration: knn encoder, "flipped"
    decoder)?  A fact about the SAMPLE's inputs, found once per pair of tensors (object identity + in-place version) with two
    device comparisons and kept on the batch beside -- not inside -- the neighbour-list cache, so `clear_graph_cache` (a step that
    rebuilds its lists) does not repeat the host synchronisation.  Never evaluated while a hipGraph is being captured."""
    facts = cache_owner.__dict__.setdefault("_gaot_flip", {})
    ent = facts.get(slot)
    if ent is not None and ent[0] is dec_ei and ent[1] == dec_ei._version and ent[2] is enc_ei and ent[3] == enc_ei._version:
        return ent[4]
    if dec_ei.is_cuda and torch.cuda.is_current_stream_capturing():
        return False
    flip = bool(dec_ei.shape == enc_ei.shape and dec_ei.dtype == enc_ei.dtype and dec_ei.device == enc_ei.device
                and torch.equal(dec_ei[0], enc_ei[1]) and torch.equal(dec_ei[1], enc_ei[0]))
    facts[slot] = (dec_ei, dec_ei._version, enc_ei, enc_ei._version, flip)
    return flip


def graph_for(edge_index: torch.Tensor, num_src: int, num_dst: int, cache_owner=None, key=None):
    """Row-sorted neighbour lists for one edge_index; cached on the batch object so that encoder GNO, GeoEmbed and the
    backward pass share one build per sample and scale.  An entry is valid only for the very tensor it was built from
    (object identity and in-place version counter; the entry keeps the tensor alive, so its address cannot be handed to
    another edge list meanwhile): edges rebuilt or re-uploaded per forward replace the entry of their slot, they never
    hit a stale one, and the cache holds one entry per (side, scale).
    A decoder list that is the encoder's with the rows swapped needs no build of its own: sorted by query it IS the encoder's
    list sorted by source and vice versa (same edge order, same stable sort: identical arrays), so the decoder's graph shares the
    encoder's two lists -- two radix-sort builds per step instead of four (0.36 ms at E = 4 M, ~5 ms at E = 64 M)."""
    if cache_owner is not None:
        cache = cache_owner.__dict__.setdefault("_gaot_graphs", {})
        k = (key, num_src, num_dst)
        ent = cache.get(k)
        if ent is not None and ent[0] is edge_index and ent[1] == edge_index._version:
            return ent[2]
        g = None
        if isinstance(key, tuple) and len(key) == 2 and key[0] == "dec":
            enc = cache.get((("enc", key[1]), num_dst, num_src))
            if (enc is not None and enc[1] == enc[0]._version
                    and _is_flip_of_encoder(cache_owner, key[1], edge_index, enc[0])):
                ge = enc[2]
                g = ops.BipartiteGraph(ge.by_src, ge.by_dst, num_src, num_dst)
        if g is None:
            g = ops.build_graph(edge_index, num_src, num_dst)
        cache[k] = (edge_index, edge_index._version, g)
        return g
    return ops.build_graph(edge_index, num_src, num_dst)


def coords_need_grad(*pos) -> bool:
    """does autograd want a gradient with respect to any of these coordinate tensors?"""
    return torch.is_grad_enabled() and any(p is not None and p.requires_grad for p in pos)


def attn_bilinear_form(wq: torch.Tensor, bq: torch.Tensor, wk: torch.Tensor, bk: torch.Tensor) -> torch.Tensor:
    """M [4, 4] with (W_q x + b_q) . (W_k y + b_k) = [x, 1]^T M [y, 1] for the reference's query_proj / key_proj
    (Linear(coord_dim -> 64) each, integral_transform.py:128-130): M = A_q^T A_k with A = [W | 0.. | b] ([64, 4]: the columns of
    the coordinates a coord_dim below 3 does not have are exact zeros, column 3 belongs to the homogeneous 1).  Pure torch, any
    device; the 64 products of an entry are added in fp64, and autograd carries dM into the four parameters."""
    cd = wq.shape[1]
    if not (1 <= cd <= 3 and wk.shape[1] == cd and wq.shape[0] == wk.shape[0]):
        raise ValueError(f"query_proj / key_proj weights {tuple(wq.shape)} / {tuple(wk.shape)}: [n, 1..3] each expected")
    hom = lambda w, b: torch.cat([w, w.new_zeros(w.shape[0], 3 - cd), b.unsqueeze(1)], dim=1)
    aq, ak = hom(wq, bq).double(), hom(wk, bk).double()
    return (aq.unsqueeze(2) * ak.unsqueeze(1)).sum(0).to(wq.dtype)


class IntegralTransform(nn.Module):
    def __init__(self, channel_mlp=None, channel_mlp_layers=None, channel_mlp_non_linearity="gelu",
                 transform_type="linear", use_attn=None, coord_dim=None, attention_type="cosine"):
        """``channel_mlp_non_linearity``: the reference's callable (F.gelu, integral_transform.py:35) or its name"""
        super().__init__()
        self.transform_type = transform_type
        self.use_attn = use_attn
        self.coord_dim = coord_dim
        self.attention_type = attention_type
        if channel_mlp is None:
            if channel_mlp_layers is None:
                raise ValueError("Need channel_mlp or layers")
            self.channel_mlp = LinearChannelMLP(layers=channel_mlp_layers, non_linearity=channel_mlp_non_linearity)
        else:
            self.channel_mlp = channel_mlp
        if self.use_attn:
            if coord_dim is None:
                raise ValueError("coord_dim must be specified when use_attn is True")
            if attention_type == "dot_product":
                self.query_proj = nn.Linear(coord_dim, 64)
                self.key_proj = nn.Linear(coord_dim, 64)
                self.scaling_factor = 1.0 / (64 ** 0.5)
            elif attention_type != "cosine":
                raise ValueError(f"Invalid attention_type: {attention_type}. Must be 'cosine' or 'dot_product'.")

    def forward(self, y_pos, x_pos, edge_index, f_y: Optional[torch.Tensor] = None, weights=None, batch_y=None,
                batch_x=None, graph=None):
        """y_pos [N_y,3] source coords, x_pos [N_x,3] query coords, edge_index [2,E] (row 0 -> y, row 1 -> x),
        f_y [N_y,C].  ``graph`` (optional) = prebuilt neighbour lists for edge_index."""
        if self.transform_type not in ("linear", "nonlinear", "nonlinear_kernelonly"):
            raise ValueError(f"Invalid transform_type: {self.transform_type}")
        fcs = list(self.channel_mlp.fcs)
        if edge_index is not None and edge_index.shape[1] == 0 and graph is None:   # integral_transform.py:106-112
            return torch.zeros(x_pos.shape[0], fcs[-1].weight.shape[0], dtype=x_pos.dtype, device=x_pos.device)
        if self.use_attn and coords_need_grad(y_pos, x_pos):
            raise NotImplementedError("IntegralTransform: gradients with respect to the coordinates are not supported with "
                                      "use_attn=True (cosine / dot-product edge scores); detach y_pos / x_pos")
        if graph is None:
            graph = graph_for(edge_index.to(x_pos.device), y_pos.shape[0], x_pos.shape[0])
        plan = self._fused_plan(fcs, f_y, y_pos, x_pos)
        if plan is not None:
            return self._forward_fused(fcs, y_pos, x_pos, f_y, graph, *plan)
        if self.use_attn:
            plan = self._fused_attn_plan(fcs, f_y, y_pos, x_pos)
            if plan is not None:
                y3, x3 = self._pad3(y_pos), self._pad3(x_pos)
                return self._forward_fused(fcs, y_pos, x_pos, f_y, graph, *plan,
                                           edge_w=self._attn_weights(y_pos, x_pos, y3, x3, graph))
        return self._forward_general(fcs, y_pos, x_pos, f_y, graph)

    def forward_knn(self, y_pos, x_pos, nbr, k: int, f_y: Optional[torch.Tensor] = None):
        """The transform's forward on a REGULAR neighbour list, without an edge list: ``nbr`` int32 [N_x * k] with nbr[q*k + j] = the
        j-th source of query q (``graph.knn_to_grid`` / ``ops.knn_grid`` output as it stands), k in ``ops.GNO_KNN_K``.  The operands
        are prepared exactly as in ``forward`` (``_fused_passes``: zero padding of coordinates / hidden widths / channel blocks,
        t = W_0f f_y of the nonlinear types) and every 32-channel pass is one ``ops.gno_forward_knn`` launch: bit-identical to
        ``forward`` on the graph of the same lists.  Forward only (nothing is recorded for autograd); runs exactly when ``_fused_plan``
        is not None and raises otherwise -- there is no general path on these lists."""
        return self._on_lists("forward_knn", y_pos, x_pos, f_y, (nbr, k), 0)[0]

    def jacobian_knn(self, y_pos, x_pos, nbr, k: int, f_y: Optional[torch.Tensor] = None):
        """``forward_knn`` with the spatial derivative of its result: -> (out [N_x, C], jac [3, N_x, C]) with
        jac[d, q, c] = d out[q, c] / d x_pos[q, d], every query's neighbour list held fixed -- the derivative autograd returns through
        ``forward`` on the graph of these lists (edges are built once and not differentiated).  It is valid almost everywhere and NOT
        defined across the surfaces where a query's k nearest sources change.  Forward mode, one ``ops.gno_forward_knn_jac`` launch per
        32-channel pass (three tangents carried through the per-edge MLP beside the value), exact fp32 in both precision modes: ``out``
        is ``forward_knn``'s fp32-mode result bit for bit.  The operands are prepared exactly as in ``forward_knn``; the planes of the
        directions a coordinate dimension of 1 / 2 is padded with are exact zeros.  Runs exactly when ``_fused_plan`` is not None and
        k is in ``ops.GNO_KNN_K`` and raises NotImplementedError otherwise.  Nothing is recorded for autograd."""
        return self._on_lists("jacobian_knn", y_pos, x_pos, f_y, (nbr, k), 1)

    def jet2_knn(self, y_pos, x_pos, nbr, k: int, f_y: Optional[torch.Tensor] = None, dirs=((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))):
        """``forward_knn`` with a directional 2-jet of its result: -> (out [N_x, C], d1 [nd, N_x, C], d2 [nd, N_x, C]), the first and
        second directional derivative of out with respect to x_pos along each of the 1..6 directions ``dirs`` (host values [nd][3];
        components beyond the coordinate dimension meet zero weight columns), every query's neighbour list held fixed as in
        ``jacobian_knn``.  One ``ops.gno_forward_knn_jet2`` launch per 32-channel pass, exact fp32 in both precision modes: ``out`` is
        ``forward_knn``'s fp32-mode result and, for an axis direction, d1 is ``jacobian_knn``'s plane, bit for bit.  The operands are
        prepared exactly as in ``jacobian_knn``.  Runs exactly when ``_fused_plan`` is not None and k is in ``ops.GNO_KNN_K`` and raises
        NotImplementedError otherwise.  Nothing is recorded for autograd."""
        return self._on_lists("jet2_knn", y_pos, x_pos, f_y, (nbr, k), 2, dirs)

    def jacobian_rows(self, y_pos, x_pos, f_y: Optional[torch.Tensor], graph):
        """``jacobian_knn`` on RAGGED rows: ``graph`` holds the by-query list of any graph (``graph.by_dst``; ``by_src`` may be None, as
        ``graph.query_lists`` leaves it) -> (out [N_x, C], jac [3, N_x, C]), every query's list held fixed, empty rows exact zeros.
        Forward mode, one ``ops.gno_forward_jac`` call (the tangent kernel and its fix-up) per 32-channel pass, exact fp32 in both
        precision modes: ``out`` is ``forward``'s fp32-mode result on the same graph bit for bit.  The operands are prepared exactly
        as in ``forward``; the planes of the directions a coordinate dimension of 1 / 2 is padded with are exact zeros.  Runs exactly
        when ``_fused_plan`` is not None and raises NotImplementedError otherwise.  Nothing is recorded for autograd."""
        return self._on_lists("jacobian_rows", y_pos, x_pos, f_y, graph, 1)

    def jet2_rows(self, y_pos, x_pos, f_y: Optional[torch.Tensor], graph, dirs):
        """``jet2_knn`` on RAGGED rows: ``graph`` holds the by-query list of any graph (``graph.by_dst``; ``by_src`` may be None, as
        ``graph.query_lists`` leaves it) -> (out [N_x, C], d1 [nd, N_x, C], d2 [nd, N_x, C]) along the 1..6 directions ``dirs`` (host
        values [nd][3]), every query's list held fixed, empty rows exact zeros in every plane.  One ``ops.gno_forward_jet2`` call (the
        jet kernel and its fix-up) per 32-channel pass, exact fp32 in both precision modes: ``out`` is ``jacobian_rows``'s and, for an
        axis direction, d1 is its Jacobian plane, bit for bit.  The operands are prepared exactly as in ``jacobian_rows``.  Runs
        exactly when ``_fused_plan`` is not None and raises NotImplementedError otherwise.  Nothing is recorded for autograd."""
        return self._on_lists("jet2_rows", y_pos, x_pos, f_y, graph, 2, dirs)

    def jet2_knn_qd(self, y_pos, x_pos, nbr, k: int, f_y: Optional[torch.Tensor], qdirs: torch.Tensor):
        """``jet2_knn`` along PER-QUERY directions: ``qdirs`` is a fp32 device tensor [N_x, nd, 3] (1..6 directions per query, used as
        given) -> (out [N_x, C], d1 [nd, N_x, C], d2 [nd, N_x, C]) with d1[i, q] / d2[i, q] along qdirs[q, i].  One
        ``ops.gno_forward_knn_jet2_qd`` launch per 32-channel pass, the operands prepared exactly as in ``jet2_knn``; the rows of
        query q are ``jet2_knn``'s with q's directions, bit for bit."""
        return self._on_lists("jet2_knn_qd", y_pos, x_pos, f_y, (nbr, k), 2, qdirs, qd=True)

    def jet2_rows_qd(self, y_pos, x_pos, f_y: Optional[torch.Tensor], graph, qdirs: torch.Tensor):
        """``jet2_rows`` along PER-QUERY directions ``qdirs`` [N_x, nd, 3] (``jet2_knn_qd``): one ``ops.gno_forward_jet2_qd`` call (the
        jet kernel and its fix-up) per 32-channel pass, the operands prepared exactly as in ``jet2_rows``."""
        return self._on_lists("jet2_rows_qd", y_pos, x_pos, f_y, graph, 2, qdirs, qd=True)

    def adjoint_knn(self, y_pos, x_pos, nbr, k: int, grad_out, graph=None):
        """The ADJOINT of ``forward_knn`` with respect to f_y: -> grad_f_y [N_y, C] = the vector-Jacobian product of the cotangent
        ``grad_out`` [N_x, C] (fp32) with d forward_knn / d f_y, on the regular list ``nbr`` / ``k`` (1/deg = 1/k).  ``graph``: the
        by-source list of these lists (``graph.by_source((nbr, k), N_y)``, built here when None).  The 'linear' transform is linear in
        f_y, so this is one forward evaluation of the per-edge kernel MLP reduced by source (``ops.gno_adjoint``: two launches per
        32-channel pass) -- no MLP backward, no weight gradients.  The operands are prepared exactly as in ``forward_knn``
        (``_fused_passes``); exact fp32 in both precision modes; nothing is recorded for autograd.  Runs exactly when ``_fused_plan``
        is not None, the transform is 'linear' and k is in ``ops.GNO_KNN_K``; raises NotImplementedError otherwise."""
        return self._adjoint(y_pos, x_pos, [grad_out], graph, (nbr, k))

    def adjoint_rows(self, y_pos, x_pos, grad_out, graph):
        """``adjoint_knn`` on RAGGED rows: ``graph`` holds both lists of the chunk -- ``by_dst`` as ``graph.query_lists`` wrote it
        (its offsets give 1/deg; a query without neighbours contributes nothing) and ``by_src`` from ``graph.by_source``."""
        return self._adjoint(y_pos, x_pos, [grad_out], graph)

    def adjoint_jac_knn(self, y_pos, x_pos, nbr, k: int, grad_out, grad_jac, graph=None):
        """The ADJOINT of ``jacobian_knn`` with respect to f_y: -> grad_f_y [N_y, C] for the cotangents ``grad_out`` [N_x, C] on the
        value and ``grad_jac`` [3, N_x, C] on the Jacobian planes (fp32, ``jacobian_knn``'s layout), on the regular list ``nbr`` /
        ``k``.  Value and tangent planes of the 'linear' transform are linear in f_y, so this is the tangent kernel's per-edge work
        contracted with the cotangents and reduced by source (``ops.gno_adjoint_jac``: two launches per 32-channel pass).  ``graph``,
        the preparation of the operands (the cotangent planes ride where ``grad_out`` does), exactness and refusals are
        ``adjoint_knn``'s."""
        return self._adjoint(y_pos, x_pos, [grad_out, grad_jac], graph, (nbr, k))

    def adjoint_jac_rows(self, y_pos, x_pos, grad_out, grad_jac, graph):
        """``adjoint_jac_knn`` on RAGGED rows: ``graph`` holds both lists of the chunk, as for ``adjoint_rows``."""
        return self._adjoint(y_pos, x_pos, [grad_out, grad_jac], graph)

    def adjoint_jet2_knn(self, y_pos, x_pos, nbr, k: int, dirs, grad_out, grad_d1, grad_d2, graph=None):
        """The ADJOINT of ``jet2_knn`` with respect to f_y: -> grad_f_y [N_y, C] for the directions ``dirs`` (host values [nd][3],
        1..6) and the cotangents ``grad_out`` [N_x, C] on the value, ``grad_d1`` [nd, N_x, C] on the first and ``grad_d2``
        [nd, N_x, C] on the second directional derivatives (fp32, ``jet2_knn``'s layout), on the regular list ``nbr`` / ``k``.
        ``grad_d2`` may be [1, N_x, C]: ONE plane every direction contracts with (the Laplacian's cotangent along the three axes).
        All 1 + 2 nd planes of the 'linear' transform are linear in f_y, so this is the jet kernel's per-edge work contracted with the
        cotangents and reduced by source (``ops.gno_adjoint_jet2``: two launches per 32-channel pass).  ``graph``, the preparation of
        the operands, exactness and refusals are ``adjoint_knn``'s."""
        return self._adjoint(y_pos, x_pos, [grad_out, grad_d1, grad_d2], graph, (nbr, k), dirs)

    def adjoint_jet2_rows(self, y_pos, x_pos, dirs, grad_out, grad_d1, grad_d2, graph):
        """``adjoint_jet2_knn`` on RAGGED rows: ``graph`` holds both lists of the chunk, as for ``adjoint_rows``."""
        return self._adjoint(y_pos, x_pos, [grad_out, grad_d1, grad_d2], graph, None, dirs)

    def adjoint_jet2_knn_qd(self, y_pos, x_pos, nbr, k: int, qdirs, grad_out, grad_d1, grad_d2, graph=None):
        """``adjoint_jet2_knn`` along PER-QUERY directions: ``qdirs`` is a fp32 device tensor [N_x, nd, 3] (``jet2_knn_qd``'s); one
        ``ops.gno_adjoint_jet2_qd`` call per 32-channel pass -- the ADJOINT of ``jet2_knn_qd`` with respect to f_y."""
        return self._adjoint(y_pos, x_pos, [grad_out, grad_d1, grad_d2], graph, (nbr, k), qdirs, qd=True)

    def adjoint_jet2_rows_qd(self, y_pos, x_pos, qdirs, grad_out, grad_d1, grad_d2, graph):
        """``adjoint_jet2_knn_qd`` on RAGGED rows: ``graph`` holds both lists of the chunk, as for ``adjoint_rows``."""
        return self._adjoint(y_pos, x_pos, [grad_out, grad_d1, grad_d2], graph, None, qdirs, qd=True)

    def _adjoint(self, y_pos, x_pos, cots, graph, lists=None, dirs=None, qd: bool = False):
        """The eight adjoint methods.  ``cots``: the cotangent planes [grad_out [N_x, C]], [grad_out, grad_jac [3, N_x, C]] or, with the
        host directions ``dirs`` [nd][3] (``qd``: the per-query directions, a device tensor [N_x, nd, 3]), [grad_out, grad_d1 [nd, N_x, C], grad_d2 [nd or 1, N_x, C]]; ``lists``: the regular list
        (nbr, k), whose by-source list is built here when ``graph`` is None, or None for the two lists of ``graph``.  Every pass of
        ``_fused_passes`` (its f_y block is grad_out's) is one ``ops.gno_adjoint`` / ``gno_adjoint_jac`` / ``gno_adjoint_jet2`` call on
        the same 32 channels of every plane, zero-padded in the last block."""
        fn = "adjoint" + ("", "_jac", "_jet2")[len(cots) - 1] + ("_rows" if lists is None else "_knn") + ("_qd" if qd else "")
        k = None
        if lists is not None:
            nbr, k = lists[0], int(lists[1])
            if k not in ops.GNO_KNN_K:
                raise NotImplementedError(f"IntegralTransform.{fn}: lists of k in {ops.GNO_KNN_K} neighbours per query, got k = {lists[1]}")
            if graph is None:
                from ... import graph as device_graph
                graph = device_graph.by_source((nbr, k), y_pos.shape[0])
        grad_out, *planes = cots
        fcs = list(self.channel_mlp.fcs)
        with torch.no_grad():
            plan = self._fused_plan(fcs, grad_out, y_pos, x_pos) if self.transform_type == "linear" else None
            if plan is None:
                raise NotImplementedError(f"IntegralTransform.{fn}: only the 'linear' transforms the fused kernels evaluate (_fused_plan); "
                                          f"transform_type = {self.transform_type!r}, use_attn = {bool(self.use_attn)}")
            if qd and not (isinstance(dirs, torch.Tensor) and dirs.dim() == 3):
                raise ValueError(f"IntegralTransform.{fn}: qdirs must be a tensor [{grad_out.shape[0]}, nd, 3]")
            nd = 0 if dirs is None else int(dirs.shape[1]) if qd else len(dirs)
            leads = [(3,)] if dirs is None else [(nd,), (nd, 1)]
            for name, t, lead in zip(("grad_jac",) if dirs is None else ("grad_d1", "grad_d2"), planes, leads):
                if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[0] not in lead or t.shape[1:] != grad_out.shape:
                    raise ValueError(f"IntegralTransform.{fn}: {name} must be [{' or '.join(str(n) for n in lead)}, "
                                     f"{grad_out.shape[0]}, {grad_out.shape[1]}], got "
                                     f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
            run = ops.gno_adjoint_jet2_qd if qd else (ops.gno_adjoint, ops.gno_adjoint_jac, ops.gno_adjoint_jet2)[len(planes)]
            y3, x3, _, (w0, b0, *mid), blocks = self._fused_passes(fcs, y_pos, x_pos, grad_out, *plan)
            outs = []
            for i, (wb, bb, gb, n) in enumerate(blocks):
                ws, bs = [w0.contiguous(), *mid[0::2], wb.contiguous()], [b0, *mid[1::2], bb.contiguous()]
                pb = [t if t.shape[2] == 32 else torch.nn.functional.pad(t[:, :, 32 * i:32 * i + n], (0, 32 - n)) for t in planes]
                o = run(ws, bs, y3, x3, *(() if dirs is None else (dirs,)), gb.contiguous(), *(p.contiguous() for p in pb), graph, k)
                outs.append(o if n == 32 else o[:, :n])
            return outs[0].contiguous() if len(outs) == 1 else torch.cat(outs, dim=1)

    def _param_adjoint(self, y_pos, x_pos, f_y, grad_out, graph, add):
        """The backward of the 'linear' transform on the lists of ``graph`` (``by_dst``: the by-query offsets, ``by_src``: the
        by-source list) with respect to f_y AND the kernel MLP: -> grad_f_y [N_y, C]; the parameters' gradients go to
        ``add(parameter, gradient)``.  Every pass of ``_fused_passes`` is ONE exact-fp32 ``ops.gno_backward`` launch (precision 0) on
        the operands ``GnoFn`` sees in that pass: the padded weights' gradients are cut back to the parameters' shapes (the transpose
        of the zero padding), the layers before the last receive every pass's part in pass order, the last layer and f_y their
        32-channel block.  Outside autograd; raises NotImplementedError unless ``_fused_plan`` takes the 'linear' transform with at
        most three hidden layers."""
        fcs = list(self.channel_mlp.fcs)
        with torch.no_grad():
            plan = self._fused_plan(fcs, f_y, y_pos, x_pos) if self.transform_type == "linear" and len(fcs) <= 4 else None
            if plan is None:
                raise NotImplementedError("IntegralTransform._param_adjoint: only the 'linear' transforms the fused kernels evaluate "
                                          f"(_fused_plan) with at most three hidden layers; transform_type = {self.transform_type!r}, "
                                          f"use_attn = {bool(self.use_attn)}, {len(fcs) - 1} hidden layers")
            cd = plan[0]
            y3, x3, _, (w0, b0, *mid), blocks = self._fused_passes(fcs, y_pos, x_pos, f_y, *plan)
            dims = [(fc.weight.shape[0], fc.weight.shape[1]) for fc in fcs]
            outs = []
            for i, (wb, bb, fb, n) in enumerate(blocks):
                ws, bs = [w0.contiguous(), *mid[0::2], wb.contiguous()], [b0, *mid[1::2], bb.contiguous()]
                gb = grad_out if (n == 32 and grad_out.shape[1] == 32) else torch.nn.functional.pad(grad_out[:, 32 * i:32 * i + n], (0, 32 - n))
                gf, gw, gbias = ops.gno_backward(ws, bs, y3, x3, fb.contiguous(), gb.contiguous(), graph, precision=0)
                outs.append(gf if n == 32 else gf[:, :n])
                g0 = gw[0][:dims[0][0]]
                add(fcs[0].weight, g0 if cd == 3 else torch.cat([g0[:, :cd], g0[:, 3:3 + cd]], dim=1))
                add(fcs[0].bias, gbias[0][:dims[0][0]])
                for l in range(1, len(fcs) - 1):
                    add(fcs[l].weight, gw[l][:dims[l][0], :dims[l][1]])
                    add(fcs[l].bias, gbias[l][:dims[l][0]])
                last = torch.zeros(dims[-1], dtype=torch.float32, device=gf.device)
                last[32 * i:32 * i + n] = gw[-1][:n, :dims[-1][1]]
                add(fcs[-1].weight, last)
                lastb = torch.zeros(dims[-1][0], dtype=torch.float32, device=gf.device)
                lastb[32 * i:32 * i + n] = gbias[-1][:n]
                add(fcs[-1].bias, lastb)
            return outs[0].contiguous() if len(outs) == 1 else torch.cat(outs, dim=1)

    def _on_lists(self, fn, y_pos, x_pos, f_y, lists, order: int, dirs=None, qd: bool = False):
        """The seven list methods: the forward-mode routes on the regular list ``lists`` = (nbr, k) or on the by-query list of the graph
        ``lists``, at ``order`` 0 (value), 1 (and Jacobian) or 2 (and 2-jets along ``dirs``: host values [nd][3], or with ``qd`` a
        device tensor [N_x, nd, 3] of per-query directions) -> the tuple of planes, channels last:
        (out [N_x, c],), (out, jac [3, N_x, c]) or (out, d1 [nd, N_x, c], d2 [nd, N_x, c]).  Every pass of ``_fused_passes`` is one call
        of the route's ``ops.gno_forward_*`` function; a pass is cut to its channels and the passes are concatenated.  Nothing is
        recorded for autograd; ``fn`` names the public method in the refusal."""
        if self.transform_type not in ("linear", "nonlinear", "nonlinear_kernelonly"):
            raise ValueError(f"Invalid transform_type: {self.transform_type}")
        fcs = list(self.channel_mlp.fcs)
        knn = isinstance(lists, tuple)
        with torch.no_grad():
            plan = self._fused_plan(fcs, f_y, y_pos, x_pos)
            if plan is None or (knn and int(lists[1]) not in ops.GNO_KNN_K):
                raise NotImplementedError(f"IntegralTransform.{fn}: only the transforms the fused kernels evaluate (_fused_plan)"
                                          + (f" on lists of k in {ops.GNO_KNN_K} neighbours per query" if knn else "")
                                          + ("; use forward() with an edge_index" if order == 0 else ""))
            run = {(True, 0): ops.gno_forward_knn, (True, 1): ops.gno_forward_knn_jac, (True, 2): ops.gno_forward_knn_jet2,
                   (False, 1): ops.gno_forward_jac, (False, 2): ops.gno_forward_jet2}[knn, order]
            if qd:                                 # order 2 along per-query directions: ``dirs`` is the device tensor [N_x, nd, 3]
                run = ops.gno_forward_knn_jet2_qd if knn else ops.gno_forward_jet2_qd
            tail = ((lists[0], int(lists[1])) if knn else (lists,)) + ((dirs,) if order == 2 else ())
            y3, x3, t, (w0, b0, *mid), blocks = self._fused_passes(fcs, y_pos, x_pos, f_y, *plan)
            outs = []
            for wb, bb, fb, n in blocks:
                o = run(self.transform_type, [w0.contiguous(), *mid[0::2], wb.contiguous()], [b0, *mid[1::2], bb.contiguous()], y3, x3,
                        None if fb is None else fb.contiguous(), t, *tail)
                o = o if order else (o,)
                outs.append(o if n == 32 else tuple(p[..., :n] for p in o))
            if len(outs) > 1:
                return tuple(torch.cat(ps, dim=-1) for ps in zip(*outs))
            return tuple(p.contiguous() for p in outs[0]) if order else outs[0]

    @staticmethod
    def _pad3(pos):
        """coordinates of dimension 1 / 2 padded with zeros to the kernels' 3-D rows"""
        return pos if pos.shape[1] >= 3 else torch.nn.functional.pad(pos, (0, 3 - pos.shape[1]))

    def _fused_plan(self, fcs, f_y, y_pos, x_pos=None):
        """(coord_dim, channels) when the fused kernels (csrc/gno*.hip: coordinates of dimension 3, hidden width 64, 32
        channels per pass) can evaluate this transform EXACTLY, possibly through zero padding; None -> general path.
        Kernel MLP coord-pair -> 64 (x 1..4; with gradients in fp32 mode: 1..3) -> C with GELU, mean reduction; 'linear' transform, or
        'nonlinear' / 'nonlinear_kernelonly' with the kernel MLP's input widened by f_y's channels (their term of the first layer is
        the per-node product t = W_0f f_y, see ``_fused_passes``; 'nonlinear' needs as many input as output channels):
          * coord_dim 1 / 2 (the reference's default is 2, magno.py:28): coordinates padded with zeros to 3-D and the first
            layer's weight given zero columns for them -- the products that are added are exactly 0;
          * C != 32 (the reference's default is 16, magno.py:25): the last layer / f_y / the output are cut into blocks of 32
            channels (the last one zero-padded); every block is one pass of the 32-channel kernels, so C = 16 costs what
            C = 32 costs and C = 64 two passes (the hidden layers are recomputed), still without a per-edge tensor in HBM."""
        if self.use_attn:
            return None
        return self._fused_shape_plan(fcs, f_y, y_pos, x_pos)

    def _fused_attn_plan(self, fcs, f_y, y_pos, x_pos=None):
        """``_fused_plan`` for use_attn=True: the same shape rules (``_fused_shape_plan``) decide whether the WEIGHTED instantiations of
        the fused kernels (``functional.GnoWFn``: a softmax weight per edge, rows summed) evaluate this transform; None -> general
        path.  The scores' own parameters (query_proj / key_proj) count among the tensors that may need a gradient."""
        if not self.use_attn or self.attention_type not in ("cosine", "dot_product"):
            return None
        cdp = y_pos.shape[1]
        cd = int(self.coord_dim) if self.coord_dim is not None else cdp
        if not (1 <= cd <= min(3, cdp)) or (x_pos is not None and x_pos.shape[1] != cdp):
            return None                                   # the general path raises for these
        also = []
        if self.attention_type == "dot_product":
            also = list(self.query_proj.parameters()) + list(self.key_proj.parameters())
        return self._fused_shape_plan(fcs, f_y, y_pos, x_pos, also)

    def _fused_shape_plan(self, fcs, f_y, y_pos, x_pos=None, also=()):
        """the shape rules shared by ``_fused_plan`` and ``_fused_attn_plan`` (see ``_fused_plan``); ``also``: further tensors whose
        ``requires_grad`` makes the transform need its backward"""
        if self.transform_type not in ("linear", "nonlinear", "nonlinear_kernelonly") or f_y is None:
            return None
        cin = 0 if self.transform_type == "linear" else f_y.shape[1]      # feature columns of the first layer
        # the exact-fp32 backward keeps the hidden activations of 128 edges in LDS: three hidden layers at most when gradients
        # are needed in fp32 mode; the bf16 backward takes four (its operand fragments then come from L2, gno_bwd3_bf16.hip)
        need_grad = torch.is_grad_enabled() and (f_y.requires_grad or any(fc.weight.requires_grad for fc in fcs)
                                                 or y_pos.requires_grad or (x_pos is not None and x_pos.requires_grad)
                                                 or any(p.requires_grad for p in also))
        from ... import ops as _ops
        max_fcs = 4 if (need_grad and _ops.get_precision() != "bf16") else 5
        if activation_name(getattr(self.channel_mlp, "non_linearity", "gelu")) != "gelu" or not (2 <= len(fcs) <= max_fcs):
            return None
        if self.training and getattr(self.channel_mlp, "dropout_p", 0.0) > 0.0:
            return None
        dims = [(fc.weight.shape[0], fc.weight.shape[1]) for fc in fcs]
        cd = y_pos.shape[1]
        c = dims[-1][0]
        # hidden widths: the kernels are written for 64; any width <= 64 (the lists in_/out_gno_channel_mlp_hidden_layers are free,
        # magno.py:32,36) is zero-padded to it -- gelu(0) = 0 and the padded rows / columns of the neighbouring weights are 0,
        # so every added product is exactly 0 (a width of 32 then costs what 64 costs; wider layers take the general path)
        chain = all(dims[i][1] == dims[i - 1][0] for i in range(1, len(dims)))
        ok = (cd in (1, 2, 3) and dims[0][1] == 2 * cd + cin and chain and all(1 <= d[0] <= 64 for d in dims[:-1])
              and 1 <= c <= 256 and (f_y.shape[1] == c or self.transform_type == "nonlinear_kernelonly")
              and all(fc.bias is not None for fc in fcs))
        return (cd, c) if ok else None

    def _fused_eligible(self, fcs, f_y) -> bool:
        """the transform runs on the fused kernels as it is (the shipped configuration): no padding, one pass"""
        dims = [(fc.weight.shape[0], fc.weight.shape[1]) for fc in fcs]
        return (not self.use_attn and self.transform_type == "linear" and f_y is not None and dims[0] == (64, 6)
                and dims[-1] == (32, 64) and f_y.shape[1] == 32)

    def _fused_passes(self, fcs, y_pos, x_pos, f_y, cd: int, c: int, straight: bool = True):
        """The operands of the fused kernels for a transform ``_fused_plan`` accepts -> (y3, x3, t, [w0, b0, *mid], blocks): the 3-D
        coordinates, the source table t = f_y W_0f^T of the nonlinear types (None for 'linear'), the parameters of every layer but the
        last as the autograd Functions take them, and per 32-channel pass one (wb, bb, fb, n): the last layer's block, f_y's block
        (None for 'nonlinear_kernelonly') and the channels that count -- a last block with n < 32 is zero-padded.  ``blocks`` is cut
        pass by pass as it is iterated, so that autograd records every pass's slices right before its Function.  The shipped shape
        (``straight``: 'linear', 3-D, C = 32, hidden widths 64) is the degenerate case: one pass of the operands as they stand."""
        w2 = lambda fc: fc.weight[:, :, 0] if fc.weight.dim() == 3 else fc.weight    # Conv1d(k=1) storage of mlp_type='channel'
        tt = self.transform_type
        if straight and self._straight_through(fcs, cd, c):
            head = []
            for fc in fcs[:-1]:
                head += [w2(fc), fc.bias]
            return y_pos, x_pos, None, head, [(w2(fcs[-1]), fcs[-1].bias, f_y, 32)]
        y3, x3, w0 = y_pos, x_pos, w2(fcs[0])
        t = None
        if tt != "linear":
            # W_0 = [W_0c | W_0f]: the feature term of the first layer, t = f_y W_0f^T [N_y, 64] (rows of W_0f zero-padded to the
            # kernels' hidden width), is formed ONCE in fp32 (layer 0 is fp32 in both precision modes) and shared by the passes;
            # its autograd turns the passes' summed dt into dW_0f = dt^T f_y and grad f_y += dt W_0f
            w0f = w0[:, 2 * cd:]
            if w0f.shape[0] != 64:
                w0f = torch.nn.functional.pad(w0f, (0, 0, 0, 64 - w0f.shape[0]))
            t = GF.linear(f_y, w0f.contiguous(), None, precision=0)
            w0 = w0[:, :2 * cd]
        if cd < 3:
            y3 = torch.nn.functional.pad(y_pos, (0, 3 - cd))
            x3 = torch.nn.functional.pad(x_pos, (0, 3 - cd))
            # [src coords | 0.. | query coords | 0..] by concatenation: no index tensor built on the host (a pageable
            # host-to-device copy per forward is a synchronisation and is illegal inside a hipGraph capture)
            z = w0.new_zeros(w0.shape[0], 3 - cd)
            w0 = torch.cat([w0[:, :cd], z, w0[:, cd:2 * cd], z], dim=1)
        pad2 = lambda w, rows, cols: w if (w.shape[0] == rows and w.shape[1] == cols) else torch.nn.functional.pad(
            w, (0, cols - w.shape[1], 0, rows - w.shape[0]))
        pad1 = lambda v, n: v if v.shape[0] == n else torch.nn.functional.pad(v, (0, n - v.shape[0]))
        head = [pad2(w0, 64, 6), pad1(fcs[0].bias, 64)]
        for fc in fcs[1:-1]:
            head += [pad2(w2(fc), 64, 64), pad1(fc.bias, 64)]
        wl, bl = w2(fcs[-1]), fcs[-1].bias
        wl = pad2(wl, wl.shape[0], 64)

        def blocks():
            for c0 in range(0, c, 32):
                n = min(32, c - c0)
                wb, bb = wl[c0:c0 + n], bl[c0:c0 + n]
                fb = None if tt == "nonlinear_kernelonly" else f_y[:, c0:c0 + n]
                if n < 32:
                    wb = torch.nn.functional.pad(wb, (0, 0, 0, 32 - n))
                    bb = torch.nn.functional.pad(bb, (0, 32 - n))
                    fb = None if fb is None else torch.nn.functional.pad(fb, (0, 32 - n))
                yield wb, bb, fb, n
        return y3, x3, t, head, blocks()

    def _straight_through(self, fcs, cd: int, c: int) -> bool:
        """the shipped shape: the kernels take the operands as they stand, in one pass"""
        return self.transform_type == "linear" and cd == 3 and c == 32 and all(fc.weight.shape[0] == 64 for fc in fcs[:-1])

    def _forward_fused(self, fcs, y_pos, x_pos, f_y, graph, cd: int, c: int, edge_w=None):
        """``forward`` on the fused kernels, through the autograd Functions: one per pass of ``_fused_passes``.  ``edge_w`` [E]
        (dst-sorted order): the weighted transform of use_attn -- every pass runs ``GnoWFn`` with the same weights and autograd adds
        the passes' gradients with respect to them (padded channels carry zero grad_out and zero f: exact zeros)."""
        tt = self.transform_type
        if edge_w is None and self._straight_through(fcs, cd, c):   # the shipped shape: the parameters themselves
            params = []
            for fc in fcs:
                params += [fc.weight, fc.bias]
            return GF.GnoFn.apply(f_y, y_pos, x_pos, graph, *params)
        y3, x3, t, (w0, b0, *mid), blocks = self._fused_passes(fcs, y_pos, x_pos, f_y, cd, c, straight=False)
        outs = []
        for wb, bb, fb, n in blocks:
            if edge_w is not None:
                o = GF.GnoWFn.apply(tt, None if fb is None else fb.contiguous(), t, edge_w, y3, x3, graph, w0.contiguous(), b0, *mid,
                                    wb.contiguous(), bb.contiguous())
            elif tt == "linear":
                o = GF.GnoFn.apply(fb.contiguous(), y3, x3, graph, w0, b0, *mid, wb.contiguous(), bb.contiguous())
            else:
                o = GF.GnoNlFn.apply(tt, None if fb is None else fb.contiguous(), t, y3, x3, graph, w0.contiguous(), b0, *mid,
                                     wb.contiguous(), bb.contiguous())
            outs.append(o[:, :n] if n < 32 else o)
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)

    def _forward_general(self, fcs, y_pos, x_pos, f_y, g):
        """integral_transform.py:114-171 on per-edge tensors (dst-sorted order).  Coordinates of dimension 1 / 2 (the
        reference's default is ``gno_coord_dim: 2``, magno.py:28) are padded with zeros to the kernels' 3-D rows and the first
        layer's weight gets zero columns for the padding: every added product is exactly 0, as in ``_fused_plan``."""
        tt = self.transform_type
        act = activation_name(getattr(self.channel_mlp, "non_linearity", "gelu"))
        pdrop = getattr(self.channel_mlp, "dropout_p", 0.0)
        cdp = y_pos.shape[1]
        if cdp > 3 or x_pos.shape[1] != cdp:
            raise NotImplementedError(f"coordinates of dimension {tuple(y_pos.shape[1:])} / {tuple(x_pos.shape[1:])}: 1..3 supported")
        y3, x3 = y_pos, x_pos
        if cdp < 3:
            y3 = torch.nn.functional.pad(y_pos, (0, 3 - cdp))
            x3 = torch.nn.functional.pad(x_pos, (0, 3 - cdp))
        with_f = f_y is not None and tt != "linear"
        k = EO.EdgeInputFn.apply(y3, x3, f_y if with_f else None, g)                                        # :146-152
        for i, fc in enumerate(fcs):                                                                        # :154
            w = fc.weight[:, :, 0] if fc.weight.dim() == 3 else fc.weight
            if i == 0 and cdp < 3:      # [src coords | query coords | features] -> [src, 0.. | query, 0.. | features]
                z = w.new_zeros(w.shape[0], 3 - cdp)
                w = torch.cat([w[:, :cdp], z, w[:, cdp:2 * cdp], z, w[:, 2 * cdp:]], dim=1)
            k = GF.linear(k, w, fc.bias, act=act if i < len(fcs) - 1 else None)
            k = GF.dropout(k, pdrop, self.training)
        if f_y is not None and tt != "nonlinear_kernelonly":                                                # :156-157
            k = EO.MulFn.apply(k, EO.GatherFn.apply(f_y, g, 0))
        mode = EO.MEAN
        if self.use_attn:                                                                                   # :126-142
            k = EO.RowScaleFn.apply(k, self._attn_weights(y_pos, x_pos, y3, x3, g))                         # :159-160
            mode = EO.SUM                                                                                   # :163
        return EO.SegmentReduceFn.apply(k, g, mode)

    def _attn_weights(self, y_pos, x_pos, y3, x3, g):
        """alpha [E] in the dst-sorted edge order: the edge scores (cosine or dot product of the endpoints' first coord_dim
        coordinates, integral_transform.py:126-137) under the softmax over every query's edges (:139-142).  ``y3`` / ``x3``: the
        coordinates as the kernels' 3-D rows.  Shared by the fused weighted path and the general path."""
        cdp = y_pos.shape[1]
        # the scores see the first coord_dim coordinates only (integral_transform.py:128-129: `[:, :self.coord_dim]`)
        cd = int(self.coord_dim) if self.coord_dim is not None else cdp
        if not 1 <= cd <= min(3, cdp):
            raise ValueError(f"coord_dim {cd} with {cdp}-dimensional coordinates")
        xa, ya = x3, y3
        if cd < cdp:             # drop the coordinates the scores do not see, keep the kernels' 3-D rows
            xa = torch.nn.functional.pad(x_pos[:, :cd], (0, 3 - cd))
            ya = torch.nn.functional.pad(y_pos[:, :cd], (0, 3 - cd))
        if self.attention_type == "dot_product":
            # (W_q x + b_q) . (W_k y + b_k) / 8 as scale * [x, 1]^T M [y, 1] with the 4 x 4 M = [W_q | b_q]^T [W_k | b_k]: one scalar
            # per edge from the two 12-byte coordinate rows instead of two gathered [E, 64] rows kept for the backward; the
            # gradient comes back as dM (16 numbers, fixed summation order) and autograd carries it into the projections
            m = attn_bilinear_form(self.query_proj.weight, self.query_proj.bias, self.key_proj.weight, self.key_proj.bias)
            sc = EO.EdgeBilinearFn.apply(xa.contiguous(), ya.contiguous(), g, m, self.scaling_factor)
        else:
            sc = EO.edge_coords(ya.contiguous(), xa.contiguous(), g, 2)   # cosine of the raw coordinates: no parameters
        return EO.SegmentSoftmaxFn.apply(sc, g)
