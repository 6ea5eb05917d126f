"""GAOT3D: encode (MAGNO) -> process (patchify, U-ViT) -> decode (MAGNO), with the reference's
constructor, buffers, parameter names and forward signature (src/model/gaot_3d.py:19-51, 248-332) so
that it drops into the reference-style trainer (`model(batch=batch, tokens_pos=...)`,
src/trainer/stat.py:544-547) and loads its checkpoints with strict=True."""
from typing import Optional

import torch
import torch.nn as nn

from .. import functional as GF
from .layers.attn import Transformer, TransformerConfig
from .layers.magno import MAGNOConfig, MAGNODecoder, MAGNOEncoder


class GAOT3D(nn.Module):
    def __init__(self, input_size: int, output_size: int, magno_config: MAGNOConfig = None,
                 attn_config: TransformerConfig = None, latent_tokens: tuple = (32, 32, 32),
                 norm_domin: list = [(-1, -1, -1), (1, 1, 1)]):
        super().__init__()
        magno_config = magno_config if magno_config is not None else MAGNOConfig()
        attn_config = attn_config if attn_config is not None else TransformerConfig()
        self.input_size = input_size
        self.output_size = output_size
        self.node_latent_size = magno_config.lifting_channels
        self.patch_size = attn_config.patch_size
        self.D, self.H, self.W = latent_tokens
        self.num_latent_tokens = self.D * self.H * self.W
        self.coord_dim = magno_config.gno_coord_dim
        lo, hi = norm_domin
        mg = torch.meshgrid(torch.linspace(lo[0], hi[0], self.D), torch.linspace(lo[1], hi[1], self.H),
                            torch.linspace(lo[2], hi[2], self.W), indexing="ij")
        self.register_buffer("latent_tokens", torch.stack(mg, dim=-1).reshape(-1, self.coord_dim))
        self.encoder = MAGNOEncoder(in_channels=input_size, out_channels=self.node_latent_size, gno_config=magno_config)
        self.processor = self.init_processor(self.node_latent_size, attn_config)
        self.decoder = MAGNODecoder(in_channels=self.node_latent_size, out_channels=output_size, gno_config=magno_config)
        # precompute_edges=False: the graphs are built on the device against the regular D x H x W token grid
        self.encoder.latent_dims = self.decoder.latent_dims = (self.D, self.H, self.W)

    def init_processor(self, node_latent_size, config):
        tok = self.patch_size ** 3 * node_latent_size
        self.patch_linear = nn.Linear(tok, tok)
        self.positional_embedding_name = config.positional_embedding
        for k, v in (("D", self.D), ("H", self.H), ("W", self.W)):
            setattr(config.attn_config, k, v)
        self._pe_cache = {}
        return Transformer(input_size=tok, output_size=tok, config=config)

    # -- constant tables -----------------------------------------------------------------------------
    def _patch_positions(self):
        p = self.patch_size
        return torch.stack(torch.meshgrid(torch.arange(self.D // p, dtype=torch.float32),
                                          torch.arange(self.H // p, dtype=torch.float32),
                                          torch.arange(self.W // p, dtype=torch.float32), indexing="ij"),
                           dim=-1).reshape(-1, 3)

    def _absolute_pe(self, device):
        """sum over the 3 patch coordinates of sin (even cols) / cos (odd cols), omega_k = 10000^(-2k/dim)
        (reference gaot_3d.py:102-144) -- a constant of the model, built once on the host."""
        key = str(device)
        if key not in self._pe_cache:
            dim = self.patch_size ** 3 * self.node_latent_size
            pos = self._patch_positions()
            freq = 1 / 10000 ** (2 * torch.arange(0, dim // 2, dtype=torch.float32) / dim)
            ang = pos[:, :, None] * freq[None, None, :]
            pe = torch.zeros(pos.shape[0], dim)
            pe[:, 0::2] = torch.sin(ang).sum(dim=1)
            pe[:, 1::2] = torch.cos(ang).sum(dim=1)
            self._pe_cache[key] = pe.to(device)
        return self._pe_cache[key]

    # -- stages ----------------------------------------------------------------------------------------
    def process(self, rndata: Optional[torch.Tensor] = None, condition: Optional[float] = None) -> torch.Tensor:
        b, m, c = rndata.shape
        d, h, w, p = self.D, self.H, self.W, self.patch_size
        assert m == d * h * w, f"n_regional_nodes ({m}) is not equal to D*H*W ({d * h * w})"
        assert d % p == 0 and h % p == 0 and w % p == 0, "Dimensions must be divisible by patch size"
        s = (d // p) * (h // p) * (w // p)
        tok = p * p * p * c
        x = GF.PatchifyFn.apply(rndata, b, d, h, w, p, c, True).view(b * s, tok)
        seq_group = getattr(self, "_seq_group", None)
        s_loc, pe = s, None
        if self.positional_embedding_name == "absolute":
            pe = self._absolute_pe(x.device)
        if seq_group is not None:
            # sequence-parallel Transformer of a point-sharded sample (gaot_3d_amd/sharding.py): every row-wise operator
            # from here to the un-patchify runs on this rank's S/G token rows
            import torch.distributed as dist
            from ..sharding import AllGatherRowsFn, SliceRowsFn
            assert b == 1, "sequence-parallel processing splits ONE sample"
            x = SliceRowsFn.apply(x, seq_group)
            s_loc = x.shape[0]
            if pe is not None:
                r0 = dist.get_rank(seq_group) * s_loc
                pe = pe[r0:r0 + s_loc].contiguous()
        x = GF.linear(x, self.patch_linear.weight, self.patch_linear.bias)
        relative_positions = None
        if pe is not None:
            x = GF.AddFn.apply(x, pe, s_loc * tok)
        elif self.positional_embedding_name == "rope":
            relative_positions = True  # the reference passes the 3-D positions only as an on/off flag
        x = self.processor(x.view(b, s_loc, tok), condition=condition, relative_positions=relative_positions)
        x = x.reshape(b * s_loc, tok)
        if seq_group is not None:
            x = AllGatherRowsFn.apply(x, seq_group)
        x = GF.PatchifyFn.apply(x, b, d, h, w, p, c, False)
        return x.view(b, d * h * w, c)

    def _tokens(self, num_graphs: int, device, tokens_pos: Optional[torch.Tensor], tokens_batch_idx: Optional[torch.Tensor]):
        """the token coordinates of every graph of the batch back to back, and their batch vector"""
        if tokens_pos is None:
            assert tokens_batch_idx is None, "tokens_batch_idx should be None if tokens_pos is None"
            tokens_pos = self.latent_tokens
        if tokens_batch_idx is None:
            lat = tokens_pos.to(device)
            lat = lat if num_graphs == 1 else lat.repeat(num_graphs, 1)
            # a per-(batch size, device) constant: built once (arange + repeat_interleave are ATen launches on the replayed step otherwise)
            cache = self.__dict__.setdefault("_lat_bidx_cache", {})
            lat_bidx = cache.get((num_graphs, device))
            if lat_bidx is None:
                lat_bidx = torch.arange(num_graphs, device=device).repeat_interleave(self.num_latent_tokens)
                cache[(num_graphs, device)] = lat_bidx
        else:
            assert tokens_pos.shape[0] == tokens_batch_idx.shape[0], "tokens_pos and tokens_batch_idx must have same length"
            lat, lat_bidx = tokens_pos.to(device), tokens_batch_idx.to(device)
        return lat.contiguous(), lat_bidx

    def _latent(self, batch, lat, lat_bidx, condition):
        rndata = self.encoder(batch=batch, latent_tokens_pos=lat, latent_tokens_batch_idx=lat_bidx)
        rndata = self.process(rndata=rndata, condition=condition)
        return rndata.view(-1, self.node_latent_size)

    def latent(self, batch, tokens_pos: Optional[torch.Tensor] = None, tokens_batch_idx: Optional[torch.Tensor] = None,
               condition: Optional[float] = None) -> torch.Tensor:
        """The first half of ``forward``: encoder and Transformer, the processed token features of every graph as rows
        [B * D*H*W, lifting_channels].  Ordinary autograd semantics.  With ``sample`` it makes the neural-field use of a trained model
        (reference trainer test loop, src/trainer/stat.py:604-620): encode a sample once, read the field wherever it is wanted."""
        lat, lat_bidx = self._tokens(batch.num_graphs, batch.pos.device, tokens_pos, tokens_batch_idx)
        return self._latent(batch, lat, lat_bidx, condition)

    def sample(self, latent: torch.Tensor, query_pos: torch.Tensor, tokens_pos: Optional[torch.Tensor] = None,
               chunk_points: Optional[int] = None) -> torch.Tensor:
        """Predictions [Nq, output_size] of ONE encoded sample (``latent`` [D*H*W, lifting_channels] from ``latent``) at any query
        coordinates, forward only (no autograd graph): ``MAGNODecoder.sample``.  ``tokens_pos``: the tokens ``latent`` was computed
        with (default: the model's grid); ``chunk_points``: queries per pass (None: one pass of at most 2^20 points)."""
        lat = self._one_sample("sample", latent, tokens_pos)
        return self.decoder.sample(latent, query_pos.to(latent.device), lat, chunk_points=chunk_points)

    def sample_jacobian(self, latent: torch.Tensor, query_pos: torch.Tensor, tokens_pos: Optional[torch.Tensor] = None,
                        chunk_points: Optional[int] = None, row_lists: bool = False):
        """``sample`` with the field's spatial derivative: -> (pred [Nq, output_size], jac [Nq, output_size, coord_dim]) with
        jac[q, o, d] = d pred[q, o] / d query_pos[q, d] (pressure gradient, wall-normal derivative, velocity Jacobian), every query's
        neighbour list held fixed: the derivative autograd returns through ``forward(query_coord_pos=...)``, valid almost everywhere
        and not defined across the surfaces where a query's nearest tokens change.  ``MAGNODecoder.sample_jacobian``: the shipped 'knn'
        decoder streams it in forward mode (no edge list, no autograd graph, no backward); neither result requires grad.  That path
        is exact fp32 in both precision modes, so in bf16 mode ``pred`` differs from ``sample``'s by bf16 rounding.
        ``row_lists=True`` streams 'radius' / 'bidirectional' decoders in the same way on row lists (``graph.query_lists`` and the
        tangent kernel on ragged rows) instead of the autograd route; it changes nothing for other decoders."""
        lat = self._one_sample("sample_jacobian", latent, tokens_pos)
        return self.decoder.sample_jacobian(latent, query_pos.to(latent.device), lat, chunk_points=chunk_points,
                                            row_lists=row_lists)

    def _one_sample(self, fn, latent, tokens_pos):
        if latent.dim() != 2 or latent.shape[0] != self.num_latent_tokens:
            raise ValueError(f"{fn}: latent {tuple(latent.shape)} is not ONE sample's [{self.num_latent_tokens}, "
                             f"{self.node_latent_size}] token rows (sample the graphs of a batch one by one)")
        return self._tokens(1, latent.device, tokens_pos, None)[0]

    def sample_hessian(self, latent: torch.Tensor, query_pos: torch.Tensor, tokens_pos: Optional[torch.Tensor] = None,
                       chunk_points: Optional[int] = None):
        """``sample_jacobian`` with the field's SECOND spatial derivatives: -> (pred [Nq, output_size], jac [Nq, output_size, 3],
        hess [Nq, output_size, 3, 3]) with hess[q, o, i, j] = d^2 pred[q, o] / d query_pos[q, i] d query_pos[q, j] (curvature and
        smoothness of the decoded field, the derivative of a wall-shear component), every query's neighbour list held fixed: valid
        almost everywhere, not defined across the surfaces where a query's nearest tokens change.  ``MAGNODecoder.sample_hessian``:
        forward-mode directional 2-jets on the shipped 'knn' decoder, exact fp32 in both precision modes, no autograd graph;
        ``pred`` and ``jac`` are ``sample_jacobian``'s bit for bit.  Configurations that do not stream raise NotImplementedError."""
        lat = self._one_sample("sample_hessian", latent, tokens_pos)
        return self.decoder.sample_hessian(latent, query_pos.to(latent.device), lat, chunk_points=chunk_points)

    def sample_laplacian(self, latent: torch.Tensor, query_pos: torch.Tensor, tokens_pos: Optional[torch.Tensor] = None,
                         chunk_points: Optional[int] = None):
        """-> (pred [Nq, output_size], lap [Nq, output_size]): the Laplacian of the field at the query points (a Poisson or momentum
        residual), the trace of ``sample_hessian``'s result bit for bit from three directions instead of six.
        ``MAGNODecoder.sample_laplacian``; conditions as for ``sample_hessian``."""
        lat = self._one_sample("sample_laplacian", latent, tokens_pos)
        return self.decoder.sample_laplacian(latent, query_pos.to(latent.device), lat, chunk_points=chunk_points)

    def sample_hessian_rows(self, latent: torch.Tensor, query_pos: torch.Tensor, tokens_pos: Optional[torch.Tensor] = None,
                            chunk_points: Optional[int] = None):
        """``sample_hessian`` for 'radius' / 'bidirectional' decoders (the reference's shipped configuration is 'bidirectional'): the
        same results on ROW lists -- ``graph.query_lists``, the jet kernel on ragged rows and a scale mix that carries the first and
        second derivative of its weights.  ``pred`` and ``jac`` are ``sample_jacobian(row_lists=True)``'s bit for bit.
        ``MAGNODecoder.sample_hessian_rows``; on a 'knn' decoder the call is ``sample_hessian``."""
        lat = self._one_sample("sample_hessian_rows", latent, tokens_pos)
        return self.decoder.sample_hessian_rows(latent, query_pos.to(latent.device), lat, chunk_points=chunk_points)

    def sample_laplacian_rows(self, latent: torch.Tensor, query_pos: torch.Tensor, tokens_pos: Optional[torch.Tensor] = None,
                              chunk_points: Optional[int] = None):
        """``sample_laplacian`` for 'radius' / 'bidirectional' decoders: -> (pred, lap), the trace of ``sample_hessian_rows``'s result
        bit for bit from three directions.  ``MAGNODecoder.sample_laplacian_rows``; on a 'knn' decoder the call is
        ``sample_laplacian``."""
        lat = self._one_sample("sample_laplacian_rows", latent, tokens_pos)
        return self.decoder.sample_laplacian_rows(latent, query_pos.to(latent.device), lat, chunk_points=chunk_points)

    def sample_directional(self, latent: torch.Tensor, query_pos: torch.Tensor, dirs: torch.Tensor,
                           tokens_pos: Optional[torch.Tensor] = None, chunk_points: Optional[int] = None):
        """Derivatives of the field along PER-QUERY directions: -> (pred [Nq, output_size], d1 [Nq, output_size, nd],
        d2 [Nq, output_size, nd]) with d1[q, o, i] = v . grad pred[q, o] and d2[q, o, i] = v^T (Hessian of pred[q, o]) v for
        v = dirs[q, i] -- the wall-normal derivative d p / d n and d^2 p / d n^2 of a surface field from the query points' normals, the
        tangential gradient and the tangential part D^2_{t1} + D^2_{t2} of the Laplacian in a local frame (n, t1, t2).  ``dirs``:
        float32 [Nq, nd, 3] on the queries' device, 1 <= nd <= 6 ([Nq, 3]: one direction), used as given (no normalisation).  Three
        chains through the per-edge MLP for one direction where ``sample_hessian`` runs 13.  ``MAGNODecoder.sample_directional``:
        'knn' decoders on the regular lists (capturable), 'radius' / 'bidirectional' on row lists; exact fp32 in both precision
        modes, outside autograd; configurations that do not stream raise NotImplementedError, a bad ``dirs`` ValueError."""
        lat = self._one_sample("sample_directional", latent, tokens_pos)
        return self.decoder.sample_directional(latent, query_pos.to(latent.device), dirs, lat, chunk_points=chunk_points)

    def _adjoint_args(self, fn, latent, query_pos, tokens_pos, autograd_order=None, chunk_points=None, what=None):
        """what the ten adjoint methods share -> (the tokens, the queries on the latent's device): ONE sample's latent and no
        point-sharded model; for the autograd forms (``autograd_order``: the adjoint's order 0 .. 3, ``what``: its name in the
        refusals where the order's own does not fit) also a ``query_pos`` that does
        not require grad and the refusals of the decoder's adjoint (``MAGNODecoder._adjoint_stream``), before the forward runs"""
        lat = self._one_sample(fn, latent, tokens_pos)
        if autograd_order is not None and query_pos.requires_grad:
            raise ValueError(f"GAOT3D.{fn}: query_pos requires grad, but gradients flow to the latent only (no derivative in the query "
                             "coordinates is formed: the first is sample_jacobian's); detach it")
        if getattr(self, "_shard_group", None) is not None:
            raise NotImplementedError(f"GAOT3D.{fn}: a point-sharded model is not supported")
        q = query_pos.to(latent.device)
        if autograd_order is not None:
            self.decoder._adjoint_stream(fn, autograd_order, latent, q, lat, chunk_points, what)
        return lat, q

    def sample_vjp(self, latent: torch.Tensor, query_pos: torch.Tensor, cotangent: torch.Tensor,
                   tokens_pos: Optional[torch.Tensor] = None, chunk_points: Optional[int] = None) -> torch.Tensor:
        """The ADJOINT of ``sample``: -> grad_latent [D*H*W, lifting_channels] (fp32) = sum_q cotangent[q] . d pred[q] / d latent for a
        cotangent [Nq, output_size] (float32, on the queries' device) -- the gradient of a number computed from sampled values (an
        integrated surface load, a misfit at sensor points) with respect to the latent, streamed in chunks of queries with no
        edge_index, no decoder autograd graph and no weight gradients.  ``MAGNODecoder.sample_vjp``: exact fp32 in both precision
        modes, outside autograd, bit-reproducible for a given ``chunk_points`` (not bit-identical across chunkings: a token's sum is
        split at chunk boundaries).  The decoder's parameters and the query coordinates are constants.  Routes and refusals are
        ``sample_hessian``'s / ``sample_hessian_rows``'s; a point-sharded model raises NotImplementedError."""
        lat, q = self._adjoint_args("sample_vjp", latent, query_pos, tokens_pos)
        return self.decoder.sample_vjp(latent, q, cotangent, lat, chunk_points=chunk_points)

    def sample_vjp_params(self, latent: torch.Tensor, query_pos: torch.Tensor, cotangent: torch.Tensor,
                          tokens_pos: Optional[torch.Tensor] = None, chunk_points: Optional[int] = None):
        """``sample_vjp`` WITH the decoder's parameters: -> (grad_latent [D*H*W, lifting_channels] (fp32), grads), ``grads`` a dict
        keyed as ``self.decoder.named_parameters()`` keys them with the fp32 gradient of EVERY decoder parameter -- one call trains
        the decoder through the streamed field at the memory of one chunk, where ``forward(query_coord_pos=...)`` carries its edge
        list and the decoder's autograd graph.  ``MAGNODecoder.sample_vjp_params``: the projection's backward is one exact-fp32
        launch (``gaot_mlp2_bwd_f32``), the kernel MLP's gradients and the latent's come from the exact-fp32 ``gaot_gno_bwd``; the
        same bits in both precision modes, outside autograd, bit-reproducible for a given ``chunk_points``.  The scale-weighting
        MLP's gradients are exact zeros on a 'knn' decoder (its mix is of equal operands).  Refusals are ``sample_vjp``'s, plus a
        kernel MLP with four hidden layers."""
        lat, q = self._adjoint_args("sample_vjp_params", latent, query_pos, tokens_pos)
        return self.decoder.sample_vjp_params(latent, q, cotangent, lat, chunk_points=chunk_points)

    def sample_autograd(self, latent: torch.Tensor, query_pos: torch.Tensor, tokens_pos: Optional[torch.Tensor] = None,
                        chunk_points: Optional[int] = None) -> torch.Tensor:
        """``sample`` as a differentiable function of the latent: -> pred [Nq, output_size] whose backward is ``sample_vjp``
        (``functional.SampleLatentFn``), so that a loss on sampled values reaches the encoder, the processor and ``batch.pos`` through
        the ordinary autograd of ``latent`` -- at the memory of one chunk, without ``forward(query_coord_pos=...)``'s edge list and
        decoder graph.  The forward is the streamed value at fp32 arithmetic in BOTH precision modes (``torch.equal`` to ``sample``
        called in fp32 mode); only the latent, the queries and the token tensor are kept for the backward.  Gradients flow to
        ``latent`` ONLY: the decoder's parameters are constants here (train them through ``sample_autograd_params``, or through
        ``forward``), and a ``query_pos`` that requires grad raises ValueError -- the derivative with respect to the query is
        ``sample_jacobian``'s.  Configurations ``sample_vjp`` refuses are refused here, before the forward runs."""
        lat, q = self._adjoint_args("sample_autograd", latent, query_pos, tokens_pos, 0, chunk_points)
        return GF.SampleLatentFn.apply(latent, self.decoder, q, lat, chunk_points)

    def sample_autograd_params(self, latent: torch.Tensor, query_pos: torch.Tensor, tokens_pos: Optional[torch.Tensor] = None,
                               chunk_points: Optional[int] = None) -> torch.Tensor:
        """``sample_autograd`` as a complete training route: -> pred [Nq, output_size], ``torch.equal`` to ``sample_autograd``'s, whose
        backward runs ``sample_vjp_params`` once (``functional.SampleTrainFn``) and hands autograd the latent's gradient (when it is
        needed) AND the gradient of every decoder parameter that requires grad; a parameter with ``requires_grad=False`` keeps
        ``.grad`` None.  Only the latent, the queries and the token tensor are kept for the backward.  With no decoder parameter
        requiring grad (or with grad disabled) the node, the launches and the bits are ``sample_autograd``'s.  A ``query_pos`` that
        requires grad raises ValueError.  Refusals are ``sample_autograd``'s, plus a kernel MLP with four hidden layers
        (``MAGNODecoder.sample_vjp_params``), all before the forward runs."""
        lat, q = self._adjoint_args("sample_autograd_params", latent, query_pos, tokens_pos, 0, chunk_points)
        params = [p for _, p in self.decoder.named_parameters()]
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            self.decoder._param_adjoint_layers("sample_autograd_params")
            return GF.SampleTrainFn.apply(latent, self.decoder, q, lat, chunk_points, *params)
        return GF.SampleLatentFn.apply(latent, self.decoder, q, lat, chunk_points)

    def sample_jacobian_vjp(self, latent: torch.Tensor, query_pos: torch.Tensor, cot_pred: Optional[torch.Tensor],
                            cot_jac: torch.Tensor, tokens_pos: Optional[torch.Tensor] = None,
                            chunk_points: Optional[int] = None) -> torch.Tensor:
        """The ADJOINT of ``sample_jacobian``: -> grad_latent [D*H*W, lifting_channels] (fp32)
        = sum_q cot_pred[q] . d pred[q] / d latent + sum_q cot_jac[q] . d jac[q] / d latent for cotangents ``cot_pred``
        [Nq, output_size] (float32, or None for a loss on the derivative alone) and ``cot_jac`` [Nq, output_size, 3] -- the gradient
        of a loss on the field's SPATIAL DERIVATIVE (a wall-normal gradient misfit, a Sobolev term, a first-order PDE or boundary
        residual) with respect to the latent, streamed in chunks of queries with no edge_index, no decoder autograd graph and no
        weight gradients.  ``MAGNODecoder.sample_jacobian_vjp``: exact fp32 in both precision modes, outside autograd,
        bit-reproducible for a given ``chunk_points``.  The decoder's parameters and the query coordinates are constants.  Routes and
        refusals are ``sample_vjp``'s."""
        lat, q = self._adjoint_args("sample_jacobian_vjp", latent, query_pos, tokens_pos)
        return self.decoder.sample_jacobian_vjp(latent, q, cot_pred, cot_jac, lat, chunk_points=chunk_points)

    def sample_jacobian_autograd(self, latent: torch.Tensor, query_pos: torch.Tensor, tokens_pos: Optional[torch.Tensor] = None,
                                 chunk_points: Optional[int] = None):
        """``sample_jacobian`` as a differentiable function of the latent: -> (pred [Nq, output_size], jac [Nq, output_size, 3]) whose
        backward is ``sample_jacobian_vjp`` (``functional.SampleJacobianLatentFn``), so that a loss on the field's derivative reaches
        the encoder, the processor and ``batch.pos`` through the ordinary autograd of ``latent``.  The forward is
        ``sample_jacobian(..., row_lists=True)``'s result bit for bit (the flag changes nothing on a 'knn' decoder); an output that
        received no gradient contributes a zero cotangent.  A normal derivative needs no API of its own:
        ``(jac * n[:, None, :]).sum(-1)`` in ordinary autograd hands the backward cot_jac = g (x) n.  Gradients flow to ``latent``
        ONLY: the decoder's parameters are constants here (``sample_autograd_params`` trains them through the value), and a ``query_pos`` that requires grad raises ValueError (no second
        derivative in the query is formed).  Configurations ``sample_jacobian_vjp`` refuses are refused here, before the forward
        runs."""
        lat, q = self._adjoint_args("sample_jacobian_autograd", latent, query_pos, tokens_pos, 1, chunk_points)
        return GF.SampleJacobianLatentFn.apply(latent, self.decoder, q, lat, chunk_points)

    def sample_laplacian_vjp(self, latent: torch.Tensor, query_pos: torch.Tensor, cot_pred: Optional[torch.Tensor],
                             cot_jac: Optional[torch.Tensor], cot_lap: torch.Tensor, tokens_pos: Optional[torch.Tensor] = None,
                             chunk_points: Optional[int] = None) -> torch.Tensor:
        """The ADJOINT of ``sample_laplacian`` (and of the derivative ``sample_hessian`` returns beside it): -> grad_latent
        [D*H*W, lifting_channels] (fp32) = sum_q cot_pred[q] . d pred[q] / d latent + sum_q cot_jac[q] . d jac[q] / d latent
        + sum_q cot_lap[q] . d lap[q] / d latent for cotangents ``cot_pred`` [Nq, output_size] and ``cot_jac`` [Nq, output_size, 3]
        (float32, each may be None) and ``cot_lap`` [Nq, output_size] -- the gradient of a loss on a PDE RESIDUAL (a Poisson residual
        Lap p - s, a diffusion term nu Lap u, a convection-diffusion residual at collocation points) with respect to the latent,
        streamed in chunks of queries with no edge_index, no decoder autograd graph and no weight gradients.
        ``MAGNODecoder.sample_laplacian_vjp``: exact fp32 in both precision modes, outside autograd, bit-reproducible for a given
        ``chunk_points``.  The decoder's parameters and the query coordinates are constants.  Routes and refusals are
        ``sample_laplacian``'s on a 'knn' decoder and ``sample_laplacian_rows``'s on 'radius' / 'bidirectional'; a transform that is
        not 'linear' and a point-sharded model raise NotImplementedError."""
        lat, q = self._adjoint_args("sample_laplacian_vjp", latent, query_pos, tokens_pos)
        return self.decoder.sample_laplacian_vjp(latent, q, cot_pred, cot_jac, cot_lap, lat, chunk_points=chunk_points)

    def sample_laplacian_autograd(self, latent: torch.Tensor, query_pos: torch.Tensor, tokens_pos: Optional[torch.Tensor] = None,
                                  chunk_points: Optional[int] = None):
        """``sample_laplacian`` as a differentiable function of the latent: -> (pred [Nq, output_size], jac [Nq, output_size, 3],
        lap [Nq, output_size]) whose backward is ``sample_laplacian_vjp`` (``functional.SampleLaplacianLatentFn``), so that a loss on
        a PDE residual reaches the encoder, the processor and ``batch.pos`` through the ordinary autograd of ``latent``.  The forward
        is ONE jet pass along the three axes: on a 'knn' decoder ``pred`` and ``lap`` are ``sample_laplacian``'s and ``jac`` is
        ``sample_hessian``'s, on 'radius' / 'bidirectional' they are ``sample_laplacian_rows``'s and ``sample_hessian_rows``'s, bit for
        bit.  An output that received no gradient contributes no cotangent.  Gradients flow to ``latent`` ONLY: the decoder's
        parameters are constants here, and a ``query_pos`` that requires grad raises ValueError (no third derivative in the query is
        formed).  Configurations ``sample_laplacian_vjp`` refuses are refused here, before the forward runs."""
        lat, q = self._adjoint_args("sample_laplacian_autograd", latent, query_pos, tokens_pos, 2, chunk_points)
        return GF.SampleLaplacianLatentFn.apply(latent, self.decoder, q, lat, chunk_points)

    def sample_directional_vjp(self, latent: torch.Tensor, query_pos: torch.Tensor, dirs: torch.Tensor,
                               cot_pred: Optional[torch.Tensor], cot_d1: Optional[torch.Tensor], cot_d2: Optional[torch.Tensor],
                               tokens_pos: Optional[torch.Tensor] = None, chunk_points: Optional[int] = None) -> torch.Tensor:
        """The ADJOINT of ``sample_directional``: -> grad_latent [D*H*W, lifting_channels] (fp32) for cotangents ``cot_pred``
        [Nq, output_size] on the value and ``cot_d1`` / ``cot_d2`` [Nq, output_size, nd] on the first and second derivatives along
        every query's own directions ``dirs`` (float32 [Nq, nd, 3] or [Nq, 3], 1 <= nd <= 6, as ``sample_directional`` takes them);
        each cotangent may be None, but not all three -- the gradient of a loss on d^2 p / d n^2, of a boundary-layer residual in a
        local frame (n, t1, t2), of the tangential Laplacian, with respect to the latent.  One value chain and two per direction
        through the per-edge MLP (3 at nd = 1; the Laplacian's adjoint runs 7, the Hessian's 13).
        ``MAGNODecoder.sample_directional_vjp``: exact fp32 in both precision modes, outside autograd, bit-reproducible for a given
        ``chunk_points``.  The decoder's parameters, the query coordinates and the directions are constants.  Routes and refusals are
        ``sample_laplacian_vjp``'s."""
        lat, q = self._adjoint_args("sample_directional_vjp", latent, query_pos, tokens_pos)
        return self.decoder.sample_directional_vjp(latent, q, dirs, cot_pred, cot_d1, cot_d2, lat, chunk_points=chunk_points)

    def sample_directional_autograd(self, latent: torch.Tensor, query_pos: torch.Tensor, dirs: torch.Tensor,
                                    tokens_pos: Optional[torch.Tensor] = None, chunk_points: Optional[int] = None):
        """``sample_directional`` as a differentiable function of the latent: -> (pred [Nq, output_size], d1 [Nq, output_size, nd],
        d2 [Nq, output_size, nd]) whose backward is ``sample_directional_vjp`` (``functional.SampleDirectionalLatentFn``), so that a
        loss such as ``((d2[..., 0] - target) ** 2).mean()`` with the wall normals as directions reaches the encoder, the processor
        and ``batch.pos`` through the ordinary autograd of ``latent``.  The forward is ``sample_directional``'s result bit for bit; an
        output that received no gradient contributes no cotangent.  Gradients flow to ``latent`` ONLY: a ``query_pos`` or a ``dirs``
        that requires grad raises ValueError.  Configurations ``sample_directional_vjp`` refuses are refused here, before the forward
        runs."""
        fn = "sample_directional_autograd"
        if isinstance(dirs, torch.Tensor) and dirs.requires_grad:
            raise ValueError(f"GAOT3D.{fn}: dirs requires grad, but gradients flow to the latent only (the directions are constants "
                             "of this node); detach it")
        dirs = self.decoder._query_dirs(fn, dirs, query_pos.to(latent.device))
        lat, q = self._adjoint_args(fn, latent, query_pos, tokens_pos, 3, chunk_points)
        return GF.SampleDirectionalLatentFn.apply(latent, self.decoder, q, lat, chunk_points, dirs)

    def sample_hessian_vjp(self, latent: torch.Tensor, query_pos: torch.Tensor, cot_pred: Optional[torch.Tensor],
                           cot_jac: Optional[torch.Tensor], cot_hess: Optional[torch.Tensor],
                           tokens_pos: Optional[torch.Tensor] = None, chunk_points: Optional[int] = None) -> torch.Tensor:
        """The ADJOINT of ``sample_hessian`` / ``sample_hessian_rows``: -> grad_latent [D*H*W, lifting_channels] (fp32) for cotangents
        ``cot_pred`` [Nq, output_size], ``cot_jac`` [Nq, output_size, 3] and ``cot_hess`` [Nq, output_size, 3, 3] (float32; each may
        be None, but not all three) -- the gradient of a loss on mixed second derivatives (the divergence of a viscous stress, a
        strain-rate term, any second-order residual that is not the Laplacian) with respect to the latent.
        ``MAGNODecoder.sample_hessian_vjp``: the cotangents through the transpose of the polarisation, then the jet adjoint along the
        six directions (13 chains through the per-edge MLP: a loss on v^T H v of known v is ``sample_directional_vjp``'s at 3).
        Exactness, routes and refusals are ``sample_laplacian_vjp``'s."""
        lat, q = self._adjoint_args("sample_hessian_vjp", latent, query_pos, tokens_pos)
        return self.decoder.sample_hessian_vjp(latent, q, cot_pred, cot_jac, cot_hess, lat, chunk_points=chunk_points)

    def sample_hessian_autograd(self, latent: torch.Tensor, query_pos: torch.Tensor, tokens_pos: Optional[torch.Tensor] = None,
                                chunk_points: Optional[int] = None):
        """``sample_hessian`` as a differentiable function of the latent: -> (pred [Nq, output_size], jac [Nq, output_size, 3],
        hess [Nq, output_size, 3, 3]) whose backward is ``sample_hessian_vjp`` (``functional.SampleHessianLatentFn``).  The forward is
        ``sample_hessian``'s ('knn') / ``sample_hessian_rows``'s ('radius', 'bidirectional') result bit for bit; an output that
        received no gradient contributes no cotangent.  Gradients flow to ``latent`` ONLY: a ``query_pos`` that requires grad raises
        ValueError.  Configurations ``sample_hessian_vjp`` refuses are refused here, before the forward runs."""
        lat, q = self._adjoint_args("sample_hessian_autograd", latent, query_pos, tokens_pos, 3, chunk_points,
                                    self.decoder.HESSIAN_VJP_WHAT)
        return GF.SampleHessianLatentFn.apply(latent, self.decoder, q, lat, chunk_points)

    def forward(self, batch, tokens_pos: Optional[torch.Tensor] = None, tokens_batch_idx: Optional[torch.Tensor] = None,
                query_coord_pos: Optional[torch.Tensor] = None, query_coord_batch_idx: Optional[torch.Tensor] = None,
                condition: Optional[float] = None) -> torch.Tensor:
        num_graphs = batch.num_graphs
        device = batch.pos.device
        lat, lat_bidx = self._tokens(num_graphs, device, tokens_pos, tokens_batch_idx)
        if query_coord_pos is None:
            q_pos, q_bidx = batch.pos, batch.batch
        else:
            assert query_coord_batch_idx is not None, "query_coord_batch_idx is required if query_coord_pos is provided"
            assert query_coord_pos.shape[0] == query_coord_batch_idx.shape[0]
            q_pos, q_bidx = query_coord_pos.to(device), query_coord_batch_idx.to(device)
        flat = self._latent(batch, lat, lat_bidx, condition)
        shard_group = getattr(self, "_shard_group", None)
        if shard_group is not None and getattr(self, "_seq_group", None) is None:
            # decoder runs on this rank's points only: its latent gradient is a partial sum (sequence-parallel: the
            # reduce-scatter inside process() already sums it)
            from ..sharding import AllReduceGradFn
            flat = AllReduceGradFn.apply(flat, shard_group)
        return self.decoder(rndata_flat=flat, phys_pos_query=q_pos, batch_idx_phys_query=q_bidx, latent_tokens_pos=lat,
                            latent_tokens_batch_idx=lat_bidx, batch=batch)
