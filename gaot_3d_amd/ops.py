"""Tensor-level wrappers over the C ABI: take torch tensors (device memory + stream plumbing only),
pass raw pointers to libgaot3d_hip.so.  Every function requires CUDA(HIP) tensors and raises otherwise."""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import GaotError, MlpGradT, MlpT, check

Tensor = torch.Tensor


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> C.c_void_p:
    """the current stream's hipStream_t (the raw getter is ~20x cheaper than building a torch.cuda.Stream per launch)"""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[Tensor]) -> C.c_void_p:
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:   # a host address reaches the kernels as an illegal access on the device: refuse it here
        raise GaotError(f"expected a tensor on the GPU (the HIP path has no CPU fallback), got {t.device}")
    return C.c_void_p(t.data_ptr())


def _req(t: Tensor, dtype, name: str) -> Tensor:
    if not t.is_cuda:
        raise GaotError(f"{name}: expected a tensor on the GPU (the HIP path has no CPU fallback), got {t.device}")
    if t.dtype != dtype:
        raise GaotError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _req_rows(t: Tensor, dtype, cols: int, name: str, dense: bool = True, rows: Optional[int] = None) -> int:
    """a row operand of the fused kernels: a 2-D ``dtype`` matrix [rows, cols], contiguous (``dense``) or with unit column stride
    and any row stride; -> its number of rows"""
    if t.dtype != dtype or t.dim() != 2 or t.shape[1] != cols or (rows is not None and t.shape[0] != rows) \
            or not (t.is_contiguous() if dense else t.stride(1) == 1):
        raise GaotError(f"{name}: {'contiguous ' if dense else ''}{dtype} [{'rows' if rows is None else rows}, {cols}] expected, "
                        f"got {t.dtype} {tuple(t.shape)} with strides {tuple(t.stride())}")
    return int(t.shape[0])


def _ws(nbytes: int, device) -> Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _slices_of_one_buffer(n: int, sizes, dtype, device, align: int = 1) -> List[Tensor]:
    """n flat tensors that are slices of ONE buffer (the outputs of a multi-tensor launch): ``sizes`` elements each (one int for
    all, or one per slice), every slice starting at a multiple of ``align`` elements"""
    sizes = [int(sizes)] * n if isinstance(sizes, int) else [int(sz) for sz in sizes]
    offs, total = [], 0
    for sz in sizes:
        offs.append(total)
        total += (sz + align - 1) // align * align
    buf = torch.empty(total, dtype=dtype, device=device)
    return [buf[o:o + sz] for o, sz in zip(offs, sizes)]


# Optional per-call device timing (bench.py): HIP events recorded on the stream the kernels are launched on.
TIMING = {"enabled": False, "events": {}}


class _timed:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if TIMING["enabled"]:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record(torch.cuda.current_stream())
        return self

    def __exit__(self, *exc):
        if TIMING["enabled"]:
            self.e1.record(torch.cuda.current_stream())
            TIMING["events"].setdefault(self.name, []).append((self.e0, self.e1))
        return False


def timing_reset(enabled: bool):
    TIMING["enabled"] = enabled
    TIMING["events"] = {}


def timing_summary():
    """-> {name: (calls, total_ms)} ; call after torch.cuda.synchronize()"""
    return {k: (len(v), sum(a.elapsed_time(b) for a, b in v)) for k, v in TIMING["events"].items()}


# ------------------------------------------------------------------------------------------------
# CSR
# ------------------------------------------------------------------------------------------------
@dataclass
class SortedEdges:
    """Edge list sorted (stably) by one endpoint.  ``key`` = the sort endpoint, ``other`` = the other."""
    rowptr: Tensor   # int32 [num_rows+1]
    perm: Optional[Tensor]     # int32 [E]; None for a list written directly in sorted order (graph.query_lists: no edge_index)
    key: Tensor      # int32 [E]
    other: Tensor    # int32 [E]
    num_rows: int

    @property
    def num_edges(self) -> int:
        return int(self.key.shape[0])


def csr_build(edge_index: Tensor, sort_row: int, num_rows: int) -> SortedEdges:
    lib = _lib.load()
    if edge_index.dtype not in (torch.int32, torch.int64):
        raise GaotError(f"edge_index must be int32 or int64, got {edge_index.dtype}")
    ei = _req(edge_index, edge_index.dtype, "edge_index")
    if ei.dim() != 2 or ei.shape[0] != 2:
        raise GaotError(f"edge_index must be [2,E], got {tuple(ei.shape)}")
    e = int(ei.shape[1])
    dev = ei.device
    rowptr = torch.empty(num_rows + 1, dtype=torch.int32, device=dev)
    perm = torch.empty(e, dtype=torch.int32, device=dev)
    key = torch.empty(e, dtype=torch.int32, device=dev)
    other = torch.empty(e, dtype=torch.int32, device=dev)
    nb = lib.gaot_csr_workspace_bytes(e, num_rows)
    ws = _ws(nb, dev)
    check(lib.gaot_csr_build(_ptr(ei), int(ei.dtype == torch.int64), e, sort_row, num_rows, _ptr(rowptr), _ptr(perm),
                             _ptr(key), _ptr(other), _ptr(ws), ws.numel(), _stream()), "gaot_csr_build")
    return SortedEdges(rowptr, perm, key, other, num_rows)


@dataclass
class BipartiteGraph:
    """Both orderings of one reference ``edge_index`` (row 0 = source, row 1 = query)."""
    by_dst: SortedEdges   # key = query,  other = source
    by_src: Optional[SortedEdges]   # key = source, other = query; None for forward-only lists (graph.query_lists): the fused
                                    # forward reads by_dst alone, every backward needs both
    num_src: int
    num_dst: int


def build_graph(edge_index: Tensor, num_src: int, num_dst: int) -> BipartiteGraph:
    return BipartiteGraph(csr_build(edge_index, 1, num_dst), csr_build(edge_index, 0, num_src), num_src, num_dst)


# ------------------------------------------------------------------------------------------------
# GNO integral transform
# ------------------------------------------------------------------------------------------------
def _mlp_struct(weights: Sequence[Tensor], biases: Sequence[Tensor]) -> Tuple[MlpT, List[Tensor]]:
    n = len(weights)
    if n < 2 or n > _lib.MAX_MLP_LAYERS:
        raise GaotError(f"kernel MLP must have 2..{_lib.MAX_MLP_LAYERS} linear layers, got {n}")
    keep = []
    m = MlpT()
    m.n_hidden = n - 1
    m.hidden = int(weights[0].shape[0])
    m.channels = int(weights[-1].shape[0])
    for l, (w, b) in enumerate(zip(weights, biases)):
        if w.dim() == 3:  # Conv1d(k=1) storage of mlp_type='channel'
            w = w[:, :, 0]
        w = _req(w, torch.float32, f"mlp.weight[{l}]")
        b = _req(b, torch.float32, f"mlp.bias[{l}]")
        exp_in = 6 if l == 0 else m.hidden
        exp_out = m.channels if l == n - 1 else m.hidden
        if tuple(w.shape) != (exp_out, exp_in):
            raise GaotError(f"kernel MLP layer {l}: weight shape {tuple(w.shape)} unsupported by the fused HIP path "
                            f"(needs [{exp_out},{exp_in}]: coord_dim 3, equal hidden widths)")
        keep += [w, b]
        m.weight[l] = w.data_ptr()
        m.bias[l] = b.data_ptr()
    return m, keep


def gno_forward(weights, biases, y_pos: Tensor, x_pos: Tensor, f_y: Tensor, g: BipartiteGraph,
                precision: Optional[int] = None) -> Tensor:
    lib = _lib.load()
    prec = _PRECISION["mode"] if precision is None else precision
    m, keep = _mlp_struct(weights, biases)
    y_pos = _req(y_pos, torch.float32, "y_pos")
    x_pos = _req(x_pos, torch.float32, "x_pos")
    f_y = _req(f_y, torch.float32, "f_y")
    if f_y.shape[1] != m.channels:
        raise GaotError(f"f_y has {f_y.shape[1]} channels, kernel MLP outputs {m.channels}")
    q = g.num_dst
    e = g.by_dst.num_edges
    out = torch.empty(q, m.channels, dtype=torch.float32, device=x_pos.device)
    ws = _ws(lib.gaot_gno_fwd_workspace_bytes(e, m.channels), x_pos.device)
    with _timed(f"gno_fwd_nh{m.n_hidden}"):
        check(lib.gaot_gno_fwd(C.byref(m), _ptr(y_pos), _ptr(x_pos), _ptr(f_y), _ptr(g.by_dst.other), _ptr(g.by_dst.key),
                               _ptr(g.by_dst.rowptr), e, q, _ptr(out), prec, _ptr(ws), ws.numel(), _stream()), "gaot_gno_fwd")
    return out


def gno_backward(weights, biases, y_pos: Tensor, x_pos: Tensor, f_y: Tensor, grad_out: Tensor, g: BipartiteGraph,
                 precision: Optional[int] = None, coords: bool = False):
    """-> (grad_f_y, [grad_w...], [grad_b...]); with ``coords`` also (grad_y_pos, grad_x_pos) appended: the kernel writes
    W_0^T dz_0 per edge (gaot_gno_bwd_coords, source-sorted order), summed here by source and by query with the fixed-order
    segmented sums"""
    lib = _lib.load()
    prec = _PRECISION["mode"] if precision is None else precision
    m, keep = _mlp_struct(weights, biases)
    y_pos = _req(y_pos, torch.float32, "y_pos")
    x_pos = _req(x_pos, torch.float32, "x_pos")
    f_y = _req(f_y, torch.float32, "f_y")
    grad_out = _req(grad_out, torch.float32, "grad_out")
    e = g.by_src.num_edges
    dev = x_pos.device
    grad_f = torch.empty(g.num_src, m.channels, dtype=torch.float32, device=dev)
    gw = [torch.empty(tuple(w.shape), dtype=torch.float32, device=dev) for w in weights]
    gb = [torch.empty(tuple(b.shape), dtype=torch.float32, device=dev) for b in biases]
    gs = MlpGradT()
    for l in range(len(weights)):
        gs.weight[l] = gw[l].data_ptr()
        gs.bias[l] = gb[l].data_ptr()
    ws = _ws(lib.gaot_gno_bwd_workspace_bytes(C.byref(m), e, g.num_dst), dev)
    if coords:
        gec = torch.empty(e, 6, dtype=torch.float32, device=dev)
        with _timed(f"gno_bwd_coords_nh{m.n_hidden}"):
            check(lib.gaot_gno_bwd_coords(C.byref(m), _ptr(y_pos), _ptr(x_pos), _ptr(f_y), _ptr(grad_out), _ptr(g.by_dst.rowptr),
                                          _ptr(g.by_src.key), _ptr(g.by_src.other), _ptr(g.by_src.rowptr), e, g.num_src,
                                          g.num_dst, _ptr(grad_f), C.byref(gs), _ptr(gec), prec, _ptr(ws), ws.numel(), _stream()),
                  "gaot_gno_bwd_coords")
        from . import edgeops as EO
        gy = EO.segment_reduce(gec, g.by_src.rowptr, None, g.num_src, EO.SUM, col0=0, channels=3)
        gx = EO.segment_reduce(gec, g.by_dst.rowptr, EO.dst_to_src_map(g), g.num_dst, EO.SUM, col0=3, channels=3)
        return grad_f, gw, gb, gy, gx
    with _timed(f"gno_bwd_nh{m.n_hidden}"):
        check(lib.gaot_gno_bwd(C.byref(m), _ptr(y_pos), _ptr(x_pos), _ptr(f_y), _ptr(grad_out), _ptr(g.by_dst.rowptr),
                               _ptr(g.by_src.key), _ptr(g.by_src.other), _ptr(g.by_src.rowptr), e, g.num_src, g.num_dst,
                               _ptr(grad_f), C.byref(gs), prec, _ptr(ws), ws.numel(), _stream()), "gaot_gno_bwd")
    return grad_f, gw, gb


GNO_MODES = {"nonlinear": 1, "nonlinear_kernelonly": 2}      # csrc/gno_common.h MODE_*


def _gno_nl_args(mode, weights, biases, y_pos: Tensor, x_pos: Tensor, f_y: Optional[Tensor], src_table: Tensor, g: BipartiteGraph):
    md = GNO_MODES.get(mode, mode)
    if md not in (1, 2):
        raise GaotError(f"gno (nonlinear): mode must be one of {tuple(GNO_MODES)}, got {mode!r}")
    m, keep = _mlp_struct(weights, biases)
    y_pos = _req(y_pos, torch.float32, "y_pos")
    x_pos = _req(x_pos, torch.float32, "x_pos")
    src_table = _req(src_table, torch.float32, "src_table")
    if tuple(src_table.shape) != (g.num_src, 64) or m.hidden != 64:
        raise GaotError(f"src_table must be [{g.num_src}, 64] (hidden width 64), got {tuple(src_table.shape)}, hidden {m.hidden}")
    if y_pos.shape[0] != g.num_src or x_pos.shape[0] != g.num_dst:
        raise GaotError(f"y_pos / x_pos have {y_pos.shape[0]} / {x_pos.shape[0]} rows, the graph {g.num_src} / {g.num_dst}")
    if md == 1:
        f_y = _req(f_y, torch.float32, "f_y")
        if tuple(f_y.shape) != (g.num_src, m.channels):
            raise GaotError(f"f_y must be [{g.num_src}, {m.channels}], got {tuple(f_y.shape)}")
    else:
        f_y = None
    return md, m, keep, y_pos, x_pos, f_y, src_table


def gno_nl_forward(mode, weights, biases, y_pos: Tensor, x_pos: Tensor, f_y: Optional[Tensor], src_table: Tensor,
                   g: BipartiteGraph, precision: Optional[int] = None) -> Tensor:
    """the fused transform for transform_type 'nonlinear' / 'nonlinear_kernelonly' (``mode``): ``weights[0]`` is the coordinate block
    W_0c [64, 6] of the first layer, ``src_table`` = f_y W_0f^T [n_src, 64] its per-node feature term.  'nonlinear': f_y [n_src, 32]
    multiplies the kernel; 'nonlinear_kernelonly': f_y is not used (pass None)."""
    lib = _lib.load()
    prec = _PRECISION["mode"] if precision is None else precision
    md, m, keep, y_pos, x_pos, f_y, src_table = _gno_nl_args(mode, weights, biases, y_pos, x_pos, f_y, src_table, g)
    q, e = g.num_dst, g.by_dst.num_edges
    out = torch.empty(q, m.channels, dtype=torch.float32, device=x_pos.device)
    ws = _ws(lib.gaot_gno_fwd_workspace_bytes(e, m.channels), x_pos.device)
    with _timed(f"gno_fwd_nl{md}_nh{m.n_hidden}"):
        check(lib.gaot_gno_fwd_nl(C.byref(m), md, _ptr(y_pos), _ptr(x_pos), _ptr(f_y), _ptr(src_table), _ptr(g.by_dst.other),
                                  _ptr(g.by_dst.key), _ptr(g.by_dst.rowptr), e, q, _ptr(out), prec, _ptr(ws), ws.numel(), _stream()),
              "gaot_gno_fwd_nl")
    return out


GNO_KNN_K = (1, 2, 4, 8, 16, 32)      # the divisors of the kernels' 32-edge tile (gaot_gno_fwd_knn)


def _gno_mode_args(fn, mode, weights, biases, y_pos, x_pos, f_y, src_table, lists):
    """the operand checks of the forward-mode entry points, which take the transform type as ``mode`` (0 / 'linear', 'nonlinear',
    'nonlinear_kernelonly') and their neighbour lists as ``lists``: the regular list (nbr, k) of ``gno_forward_knn*`` or the graph whose
    by-query list ``gno_forward_jac`` / ``gno_forward_jet2`` read -> (..., (nbr, k) or the graph, the number of queries)"""
    md = {"linear": 0, **GNO_MODES}.get(mode, mode)
    if md not in (0, 1, 2):
        raise GaotError(f"{fn}: mode must be 'linear' or one of {tuple(GNO_MODES)}, got {mode!r}")
    m, keep = _mlp_struct(weights, biases)
    y_pos = _req(y_pos, torch.float32, "y_pos")
    x_pos = _req(x_pos, torch.float32, "x_pos")
    if y_pos.dim() != 2 or x_pos.dim() != 2 or y_pos.shape[1] != 3 or x_pos.shape[1] != 3:
        raise GaotError(f"y_pos / x_pos must be [*, 3], got {tuple(y_pos.shape)} / {tuple(x_pos.shape)}")
    n_src = int(y_pos.shape[0])
    if md != 2:
        f_y = _req(f_y, torch.float32, "f_y")
        if tuple(f_y.shape) != (n_src, m.channels):
            raise GaotError(f"f_y must be [{n_src}, {m.channels}], got {tuple(f_y.shape)}")
    else:
        f_y = None
    if md != 0:
        src_table = _req(src_table, torch.float32, "src_table")
        if tuple(src_table.shape) != (n_src, 64):
            raise GaotError(f"src_table must be [{n_src}, 64], got {tuple(src_table.shape)}")
    else:
        src_table = None
    q = int(x_pos.shape[0])
    if isinstance(lists, tuple):
        nbr, k = _req(lists[0], torch.int32, "nbr"), int(lists[1])
        if nbr.numel() != q * k:
            raise GaotError(f"nbr must hold {q} x {k} ids, got {nbr.numel()}")
        lists = (nbr, k)
    elif n_src != lists.num_src or q != lists.num_dst:
        raise GaotError(f"y_pos / x_pos have {n_src} / {q} rows, the graph {lists.num_src} / {lists.num_dst}")
    return md, m, keep, y_pos, x_pos, f_y, src_table, lists, q


def _gno_planes(x_pos, q, m, *counts):
    """the results of a forward-mode entry point: out [q, channels] and one stack of derivative planes [max(n, 1), q, channels] per count"""
    new = lambda *lead: torch.empty(*lead, q, m.channels, dtype=torch.float32, device=x_pos.device)
    return (new(), *(new(max(n, 1)) for n in counts))


def gno_forward_knn(mode, weights, biases, y_pos: Tensor, x_pos: Tensor, f_y: Optional[Tensor], src_table: Optional[Tensor],
                    nbr: Tensor, k: int, precision: Optional[int] = None) -> Tensor:
    """the fused transform's FORWARD on a regular neighbour list (gaot_gno_fwd_knn): ``nbr`` int32 [n_query * k] with
    nbr[q*k + j] = the j-th source of query q (``knn_grid``'s output as it stands), k in ``GNO_KNN_K``.  ``mode``: 0 / 'linear'
    (``src_table`` None), 'nonlinear', 'nonlinear_kernelonly' (``f_y`` None), operands as in ``gno_forward`` / ``gno_nl_forward``.
    One launch, no edge list, no sorted lists, no workspace; bit-identical to those two on ``build_graph`` of the same lists.  No
    backward."""
    lib = _lib.load()
    prec = _PRECISION["mode"] if precision is None else precision
    md, m, keep, y_pos, x_pos, f_y, src_table, (nbr, k), q = _gno_mode_args("gno_forward_knn", mode, weights, biases, y_pos, x_pos, f_y,
                                                                            src_table, (nbr, k))
    (out,) = _gno_planes(x_pos, q, m)
    with _timed(f"gno_fwd_knn{f'_nl{md}' if md else ''}_nh{m.n_hidden}"):
        check(lib.gaot_gno_fwd_knn(C.byref(m), md, _ptr(y_pos), _ptr(x_pos), _ptr(f_y), _ptr(src_table), _ptr(nbr), k, q, _ptr(out),
                                   prec, _stream()), "gaot_gno_fwd_knn")
    return out


def gno_adjoint(weights, biases, y_pos: Tensor, x_pos: Tensor, grad_out: Tensor, g: BipartiteGraph, k: Optional[int] = None) -> Tensor:
    """The ADJOINT of the linear transform with respect to f_y (gaot_gno_adj): -> grad_f_y [n_src, 32] with
        grad_f_y[t] = sum over the edges e of source t of  K(y_pos[t], x_pos[q_e]) * grad_out[q_e] / deg(q_e)
    -- what ``gno_backward`` returns as its first result, from ONE forward evaluation of the per-edge kernel MLP: no MLP backward, no
    weight gradients, no f_y.  Reads the by-SOURCE list ``g.by_src`` (``graph.by_source`` builds it for a chunk of queries); deg(q)
    comes from ``g.by_dst.rowptr``, or, with ``k`` given, is the constant k of a regular list and ``g.by_dst`` may be None.  Exact fp32
    whatever the precision mode (the same bits in both), no atomics, bit-reproducible run to run; a source without edges gets exact
    zeros.  Two launches (main + fix-up; the fix-up alone without edges).  Rows are long -- every query that selected a source -- so
    most straddle the 32-edge tiles and one fix-up thread adds a row's tile partials in order: slow when the queries cluster on a
    few sources, but correct."""
    m, keep, y_pos, x_pos, grad_out, rowptr_dst, kk, e = _gno_adjoint_args("gno_adjoint", weights, biases, y_pos, x_pos, grad_out, g, k)
    return _gno_adjoint_launch("gaot_gno_adj", m, y_pos, x_pos, (_ptr(grad_out),), rowptr_dst, kk, g, e, m.channels)


def _gno_adjoint_args(fn, weights, biases, y_pos, x_pos, grad_out, g, k):
    """the operand rules of the three ``gno_adjoint*`` entry points -> (the MLP struct, what keeps its arrays alive, y_pos, x_pos,
    grad_out, rowptr_dst or None, the k passed to the ABI, the number of edges)"""
    m, keep = _mlp_struct(weights, biases)
    y_pos = _req(y_pos, torch.float32, "y_pos")
    x_pos = _req(x_pos, torch.float32, "x_pos")
    grad_out = _req(grad_out, torch.float32, "grad_out")
    if y_pos.dim() != 2 or x_pos.dim() != 2 or y_pos.shape[1] != 3 or x_pos.shape[1] != 3:
        raise GaotError(f"{fn}: y_pos / x_pos must be [*, 3], got {tuple(y_pos.shape)} / {tuple(x_pos.shape)}")
    if g.by_src is None:
        raise GaotError(f"{fn}: the graph has no by-source list (graph.by_source builds one)")
    if y_pos.shape[0] != g.num_src or x_pos.shape[0] != g.num_dst:
        raise GaotError(f"{fn}: y_pos / x_pos have {y_pos.shape[0]} / {x_pos.shape[0]} rows, the graph {g.num_src} / {g.num_dst}")
    if tuple(grad_out.shape) != (g.num_dst, m.channels):
        raise GaotError(f"{fn}: grad_out must be [{g.num_dst}, {m.channels}], got {tuple(grad_out.shape)}")
    e = g.by_src.num_edges
    if k is None:
        if g.by_dst is None:
            raise GaotError(f"{fn}: the degrees need the by-query offsets (g.by_dst.rowptr) or the k of a regular list")
        rowptr_dst, kk = g.by_dst.rowptr, 0
    else:
        rowptr_dst, kk = None, int(k)
        if kk < 1 or e != g.num_dst * kk:
            raise GaotError(f"{fn}: a regular list of {g.num_dst} queries x k = {kk} holds {g.num_dst * max(kk, 0)} edges, got {e}")
    return m, keep, y_pos, x_pos, grad_out, rowptr_dst, kk, e


def _gno_adjoint_planes(fn, name, t, lead, grad_out) -> None:
    """a stack of cotangent planes beside ``grad_out`` [n_query, 32]: contiguous float32 [one of ``lead``, n_query, 32] on its device"""
    if not isinstance(t, Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 3 \
            or t.shape[0] not in lead or t.shape[1:] != grad_out.shape or t.device != grad_out.device:
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}, strides {tuple(t.stride())}" if isinstance(t, Tensor) else type(t).__name__
        raise GaotError(f"{fn}: {name} must be contiguous float32 [{' or '.join(str(n) for n in lead)}, {grad_out.shape[0]}, "
                        f"{grad_out.shape[1]}] on {grad_out.device}, got {got}")


def _gno_adjoint_launch(entry, m, y_pos, x_pos, cots, rowptr_dst, kk, g, e, *ws_args) -> Tensor:
    """the launch of the three ``gno_adjoint*`` entry points: grad_f [n_src, 32] allocated, ``entry``'s workspace (sized by the edges
    and ``ws_args``) and the call under its timing label -- ``entry`` without 'gaot_', then the number of hidden layers.  ``cots``: the
    ABI's arguments between x_pos and rowptr_dst (the cotangent planes and, for the jets, their directions)."""
    lib = _lib.load()
    dev = x_pos.device
    grad_f = torch.empty(g.num_src, m.channels, dtype=torch.float32, device=dev)
    ws = _ws(getattr(lib, f"{entry}_workspace_bytes")(e, *ws_args), dev)
    with _timed(f"{entry[len('gaot_'):]}_nh{m.n_hidden}"):
        check(getattr(lib, entry)(C.byref(m), _ptr(y_pos), _ptr(x_pos), *cots, _ptr(rowptr_dst), kk, _ptr(g.by_src.key),
                                  _ptr(g.by_src.other), _ptr(g.by_src.rowptr), e, g.num_src, g.num_dst, _ptr(grad_f), _ptr(ws),
                                  ws.numel(), _stream()), entry)
    return grad_f


def gno_adjoint_jac(weights, biases, y_pos: Tensor, x_pos: Tensor, grad_out: Tensor, grad_jac: Tensor, g: BipartiteGraph,
                    k: Optional[int] = None) -> Tensor:
    """The ADJOINT of ``gno_forward_knn_jac`` / ``gno_forward_jac`` ('linear') with respect to f_y (gaot_gno_adj_jac): for cotangents
    ``grad_out`` [n_query, 32] on the value and ``grad_jac`` [3, n_query, 32] on the three tangent planes (the layout those two
    write) -> grad_f_y [n_src, 32] with
        grad_f_y[t] = sum over the edges e of source t of  (K_e * grad_out[q_e] + sum_d d_d K_e * grad_jac[d, q_e]) / deg(q_e)
    where d_d K is the derivative of the kernel MLP in coordinate d of the query.  The tangent kernel's per-edge work (value and
    three tangent chains, forward mode) contracted with four gathered cotangent rows into one plane and reduced by source: no MLP
    backward, no weight gradients, no f_y.  Operand rules are ``gno_adjoint``'s, with ``grad_jac`` float32, contiguous, on the
    device; exact fp32 whatever the precision mode (the same bits in both), no atomics, bit-reproducible run to run; a source
    without edges gets exact zeros.  Two launches (main + fix-up; the fix-up alone without edges)."""
    fn = "gno_adjoint_jac"
    m, keep, y_pos, x_pos, grad_out, rowptr_dst, kk, e = _gno_adjoint_args(fn, weights, biases, y_pos, x_pos, grad_out, g, k)
    _gno_adjoint_planes(fn, "grad_jac", grad_jac, (3,), grad_out)
    return _gno_adjoint_launch("gaot_gno_adj_jac", m, y_pos, x_pos, (_ptr(grad_out), _ptr(grad_jac)), rowptr_dst, kk, g, e)


def gno_adjoint_jet2(weights, biases, y_pos: Tensor, x_pos: Tensor, dirs, grad_out: Tensor, grad_d1: Tensor, grad_d2: Tensor,
                     g: BipartiteGraph, k: Optional[int] = None) -> Tensor:
    """The ADJOINT of ``gno_forward_knn_jet2`` / ``gno_forward_jet2`` ('linear') with respect to f_y (gaot_gno_adj_jet2): for the
    directions ``dirs`` (1..6, host values [nd][3]) and cotangents ``grad_out`` [n_query, 32] on the value, ``grad_d1``
    [nd, n_query, 32] on the first and ``grad_d2`` on the second directional derivatives -> grad_f_y [n_src, 32] with
        grad_f_y[t] = sum over the edges e of source t of
                      (K_e * grad_out[q_e] + sum_i D_vi K_e * grad_d1[i, q_e] + sum_i D_vi^2 K_e * grad_d2[i, q_e]) / deg(q_e)
    ``grad_d2`` is [nd, n_query, 32] (one plane per direction) or [1, n_query, 32]: ONE plane every direction contracts with -- the
    cotangent of a Laplacian along the three axes, without copies.  The jet kernel's per-edge work (the value path once, h' and h''
    per direction) contracted with the gathered cotangent rows into one plane and reduced by source: no MLP backward, no weight
    gradients, no f_y.  Operand rules are ``gno_adjoint``'s, with the cotangent planes float32, contiguous, on the device; exact
    fp32 whatever the precision mode (the same bits in both), no atomics, bit-reproducible run to run; a source without edges gets
    exact zeros.  Two launches (main + fix-up; the fix-up alone without edges)."""
    fn = "gno_adjoint_jet2"
    m, keep, y_pos, x_pos, grad_out, rowptr_dst, kk, e = _gno_adjoint_args(fn, weights, biases, y_pos, x_pos, grad_out, g, k)
    hd, nd = _host_dirs(fn, dirs)
    if not 1 <= nd <= 6:
        raise GaotError(f"{fn}: 1..6 directions, got {nd}")
    _gno_adjoint_planes(fn, "grad_d1", grad_d1, (nd,), grad_out)
    _gno_adjoint_planes(fn, "grad_d2", grad_d2, (nd, 1), grad_out)
    stride2 = 0 if grad_d2.shape[0] == 1 and nd > 1 else g.num_dst * m.channels    # one direction: both forms name the same plane
    return _gno_adjoint_launch("gaot_gno_adj_jet2", m, y_pos, x_pos, (hd, nd, _ptr(grad_out), _ptr(grad_d1), _ptr(grad_d2), stride2),
                               rowptr_dst, kk, g, e)


def gno_adjoint_jet2_qd(weights, biases, y_pos: Tensor, x_pos: Tensor, qdirs: Tensor, grad_out: Tensor, grad_d1: Tensor,
                        grad_d2: Tensor, g: BipartiteGraph, k: Optional[int] = None) -> Tensor:
    """``gno_adjoint_jet2`` along PER-QUERY directions (gaot_gno_adj_jet2_qd): the ADJOINT of ``gno_forward_knn_jet2_qd`` /
    ``gno_forward_jet2_qd`` ('linear') with respect to f_y.  ``qdirs`` is a DEVICE tensor [n_query, nd, 3] (1..6 directions per query,
    used as given, read by the kernel: no host read, capturable) -> grad_f_y [n_src, 32] with
        grad_f_y[t] = sum over the edges e of source t of (K_e * grad_out[q_e] + sum_i D_v K_e * grad_d1[i, q_e]
                                                           + sum_i D_v^2 K_e * grad_d2[i, q_e]) / deg(q_e),   v = qdirs[q_e, i]
    Everything else is ``gno_adjoint_jet2``'s: the cotangent planes (``grad_d2`` [nd or 1, n_query, 32]), the lists, the degrees,
    exact fp32 whatever the precision mode, no atomics, bit-reproducible, exact zeros for a source without edges, two launches.  With
    the same directions on every query the result is ``gno_adjoint_jet2``'s on those directions, bit for bit."""
    fn = "gno_adjoint_jet2_qd"
    m, keep, y_pos, x_pos, grad_out, rowptr_dst, kk, e = _gno_adjoint_args(fn, weights, biases, y_pos, x_pos, grad_out, g, k)
    qdirs, nd = _query_dirs(fn, qdirs, x_pos, g.num_dst)
    if not 1 <= nd <= 6:
        raise GaotError(f"{fn}: 1..6 directions, got {nd}")
    _gno_adjoint_planes(fn, "grad_d1", grad_d1, (nd,), grad_out)
    _gno_adjoint_planes(fn, "grad_d2", grad_d2, (nd, 1), grad_out)
    stride2 = 0 if grad_d2.shape[0] == 1 and nd > 1 else g.num_dst * m.channels    # one direction: both forms name the same plane
    return _gno_adjoint_launch("gaot_gno_adj_jet2_qd", m, y_pos, x_pos,
                               (_ptr(qdirs), nd, _ptr(grad_out), _ptr(grad_d1), _ptr(grad_d2), stride2), rowptr_dst, kk, g, e)


def gno_forward_knn_jac(mode, weights, biases, y_pos: Tensor, x_pos: Tensor, f_y: Optional[Tensor], src_table: Optional[Tensor],
                        nbr: Tensor, k: int):
    """``gno_forward_knn`` with the spatial derivative of its result (gaot_gno_fwd_knn_jac): -> (out [n_query, 32],
    jac [3, n_query, 32]) with jac[d, q, c] = d out[q, c] / d x_pos[q, d], the neighbour list of every query held fixed (the derivative
    autograd returns through ``gno_forward`` on the graph of these lists; valid almost everywhere, not across the surfaces where a
    query's k nearest sources change).  Forward mode: three tangents ride through the per-edge MLP beside the value, one launch,
    nothing stored, no backward.  Exact fp32 whatever the precision mode: ``out`` is ``gno_forward_knn(..., precision=0)`` bit for
    bit.  Operands and their checks are those of ``gno_forward_knn``."""
    lib = _lib.load()
    md, m, keep, y_pos, x_pos, f_y, src_table, (nbr, k), q = _gno_mode_args("gno_forward_knn_jac", mode, weights, biases, y_pos, x_pos,
                                                                            f_y, src_table, (nbr, k))
    out, jac = _gno_planes(x_pos, q, m, 3)
    with _timed(f"gno_fwd_knn_jac{f'_nl{md}' if md else ''}_nh{m.n_hidden}"):
        check(lib.gaot_gno_fwd_knn_jac(C.byref(m), md, _ptr(y_pos), _ptr(x_pos), _ptr(f_y), _ptr(src_table), _ptr(nbr), k, q,
                                       _ptr(out), _ptr(jac), _stream()), "gaot_gno_fwd_knn_jac")
    return out, jac


def _host_dirs(fn, dirs):
    """directions as a host float array [nd][3] (a CPU tensor or nested sequences: never a device tensor, whose read would synchronise)"""
    if isinstance(dirs, Tensor):
        if dirs.is_cuda:
            raise GaotError(f"{fn}: dirs must live on the host (the directions are passed to the kernel by value)")
        dirs = dirs.tolist()
    rows = [tuple(float(c) for c in d) for d in dirs]
    if any(len(d) != 3 for d in rows):
        raise GaotError(f"{fn}: dirs must be [nd][3]")
    flat = [c for d in rows for c in d]
    return (C.c_float * max(len(flat), 1))(*flat), len(rows)


def gno_forward_knn_jet2(mode, weights, biases, y_pos: Tensor, x_pos: Tensor, f_y: Optional[Tensor], src_table: Optional[Tensor],
                         nbr: Tensor, k: int, dirs):
    """``gno_forward_knn`` with a directional 2-jet of its result (gaot_gno_fwd_knn_jet2): -> (out [n_query, 32], d1 [nd, n_query, 32],
    d2 [nd, n_query, 32]) with d1[i] = D_v out and d2[i] = D_v^2 out along v = dirs[i] (1..6 directions, host values [nd][3]) with
    respect to x_pos, the neighbour lists held fixed as in ``gno_forward_knn_jac``.  One launch, forward mode, exact fp32 whatever the
    precision mode: ``out`` is ``gno_forward_knn(..., precision=0)`` and, for an axis direction e_d, d1[i] is ``gno_forward_knn_jac``'s
    plane d, bit for bit; a direction's planes do not depend on the other directions.  Six directions e_x, e_y, e_z, e_x+e_y, e_y+e_z,
    e_x+e_z give a Hessian by polarisation.  Operands and their checks are those of ``gno_forward_knn_jac``."""
    lib = _lib.load()
    md, m, keep, y_pos, x_pos, f_y, src_table, (nbr, k), q = _gno_mode_args("gno_forward_knn_jet2", mode, weights, biases, y_pos, x_pos,
                                                                            f_y, src_table, (nbr, k))
    hd, nd = _host_dirs("gno_forward_knn_jet2", dirs)
    out, d1, d2 = _gno_planes(x_pos, q, m, nd, nd)
    with _timed(f"gno_jet2_knn{f'_nl{md}' if md else ''}_nh{m.n_hidden}_d{nd}"):
        check(lib.gaot_gno_fwd_knn_jet2(C.byref(m), md, _ptr(y_pos), _ptr(x_pos), _ptr(f_y), _ptr(src_table), _ptr(nbr), k, q, hd, nd,
                                        _ptr(out), _ptr(d1), _ptr(d2), _stream()), "gaot_gno_fwd_knn_jet2")
    return out, d1, d2


def gno_forward_jac(mode, weights, biases, y_pos: Tensor, x_pos: Tensor, f_y: Optional[Tensor], src_table: Optional[Tensor],
                    g: BipartiteGraph):
    """``gno_forward_knn_jac`` on RAGGED rows (gaot_gno_fwd_jac): the value and the Jacobian of the fused transform on the by-query list
    of any graph -> (out [n_query, 32], jac [3, n_query, 32]), every query's list held fixed, rows of any length (an empty row gives
    exact zeros in all four planes).  Reads ``g.by_dst.{other, key, rowptr}`` alone: ``g.by_src`` may be None (``graph.query_lists``).
    Two launches (the tangent kernel and one fix-up over the four planes), exact fp32 whatever the precision mode: ``out`` is
    ``gno_forward`` / ``gno_nl_forward(..., precision=0)`` on the same graph bit for bit, and on a list of equal rows of k in
    ``GNO_KNN_K`` edges both results are ``gno_forward_knn_jac``'s.  ``mode`` and the operands as in ``gno_forward_knn``."""
    lib = _lib.load()
    md, m, keep, y_pos, x_pos, f_y, src_table, g, q = _gno_mode_args("gno_forward_jac", mode, weights, biases, y_pos, x_pos, f_y,
                                                                     src_table, g)
    e = g.by_dst.num_edges
    out, jac = _gno_planes(x_pos, q, m, 3)
    ws = _ws(lib.gaot_gno_fwd_jac_workspace_bytes(e), x_pos.device)
    with _timed(f"gno_fwd_jac{f'_nl{md}' if md else ''}_nh{m.n_hidden}"):
        check(lib.gaot_gno_fwd_jac(C.byref(m), md, _ptr(y_pos), _ptr(x_pos), _ptr(f_y), _ptr(src_table), _ptr(g.by_dst.other),
                                   _ptr(g.by_dst.key), _ptr(g.by_dst.rowptr), e, q, _ptr(out), _ptr(jac), _ptr(ws), ws.numel(),
                                   _stream()), "gaot_gno_fwd_jac")
    return out, jac


def gno_forward_jet2(mode, weights, biases, y_pos: Tensor, x_pos: Tensor, f_y: Optional[Tensor], src_table: Optional[Tensor],
                     g: BipartiteGraph, dirs):
    """``gno_forward_knn_jet2`` on RAGGED rows (gaot_gno_fwd_jet2): the value and the directional 2-jets of the fused transform on the
    by-query list of any graph -> (out [n_query, 32], d1 [nd, n_query, 32], d2 [nd, n_query, 32]), every query's list held fixed, rows
    of any length (an empty row gives exact zeros in all 1 + 2 nd planes).  Reads ``g.by_dst`` alone, as ``gno_forward_jac``.  Two
    launches (the jet kernel and one fix-up over all planes), exact fp32 whatever the precision mode: ``out`` is ``gno_forward_jac``'s,
    for an axis direction e_d plane d1 is its Jacobian plane d, and on a list of equal rows of k in ``GNO_KNN_K`` edges every plane is
    ``gno_forward_knn_jet2``'s, bit for bit.  ``mode`` and the operands as in ``gno_forward_jac``, ``dirs`` as in
    ``gno_forward_knn_jet2``.  Workspace: 256 (1 + 2 nd) bytes per 32-edge tile."""
    lib = _lib.load()
    md, m, keep, y_pos, x_pos, f_y, src_table, g, q = _gno_mode_args("gno_forward_jet2", mode, weights, biases, y_pos, x_pos, f_y,
                                                                     src_table, g)
    hd, nd = _host_dirs("gno_forward_jet2", dirs)
    e = g.by_dst.num_edges
    out, d1, d2 = _gno_planes(x_pos, q, m, nd, nd)
    ws = _ws(lib.gaot_gno_fwd_jet2_workspace_bytes(e, min(max(nd, 0), 6)), x_pos.device)
    with _timed(f"gno_jet2_rows{f'_nl{md}' if md else ''}_nh{m.n_hidden}_d{nd}"):
        check(lib.gaot_gno_fwd_jet2(C.byref(m), md, _ptr(y_pos), _ptr(x_pos), _ptr(f_y), _ptr(src_table), _ptr(g.by_dst.other),
                                    _ptr(g.by_dst.key), _ptr(g.by_dst.rowptr), e, q, hd, nd, _ptr(out), _ptr(d1), _ptr(d2), _ptr(ws),
                                    ws.numel(), _stream()), "gaot_gno_fwd_jet2")
    return out, d1, d2


def _query_dirs(fn, qdirs, x_pos: Tensor, q: int):
    """per-query directions as a contiguous fp32 DEVICE tensor [q, nd, 3] on the queries' device -> (qdirs, nd); the range of nd is
    the entry point's check"""
    if not isinstance(qdirs, Tensor) or qdirs.dtype != torch.float32 or qdirs.device != x_pos.device:
        raise GaotError(f"{fn}: qdirs must be a float32 tensor on {x_pos.device} (per-query directions are read by the kernel)")
    if qdirs.dim() != 3 or qdirs.shape[0] != q or qdirs.shape[2] != 3:
        raise GaotError(f"{fn}: qdirs must be [{q}, nd, 3], got {tuple(qdirs.shape)}")
    return qdirs.contiguous(), int(qdirs.shape[1])


def gno_forward_knn_jet2_qd(mode, weights, biases, y_pos: Tensor, x_pos: Tensor, f_y: Optional[Tensor], src_table: Optional[Tensor],
                            nbr: Tensor, k: int, qdirs: Tensor):
    """``gno_forward_knn_jet2`` along PER-QUERY directions (gaot_gno_fwd_knn_jet2_qd): ``qdirs`` is a DEVICE tensor [n_query, nd, 3]
    (1..6 directions per query, used as given) -> (out [n_query, 32], d1 [nd, n_query, 32], d2 [nd, n_query, 32]) with
    d1[i, q] = D_v out[q] and d2[i, q] = D_v^2 out[q] along v = qdirs[q, i].  One launch, exact fp32 whatever the precision mode, no
    host read of the directions (capturable).  Per edge the operations of ``gno_forward_knn_jet2`` in its order: the rows of query q
    are that call's with q's directions, bit for bit; a direction slot's planes do not depend on the other slots; a zero direction
    gives zeros.  Operands and their checks are those of ``gno_forward_knn_jet2``."""
    lib = _lib.load()
    md, m, keep, y_pos, x_pos, f_y, src_table, (nbr, k), q = _gno_mode_args("gno_forward_knn_jet2_qd", mode, weights, biases, y_pos,
                                                                            x_pos, f_y, src_table, (nbr, k))
    qdirs, nd = _query_dirs("gno_forward_knn_jet2_qd", qdirs, x_pos, q)
    out, d1, d2 = _gno_planes(x_pos, q, m, nd, nd)
    with _timed(f"gno_jet2_knn_qd{f'_nl{md}' if md else ''}_nh{m.n_hidden}_d{nd}"):
        check(lib.gaot_gno_fwd_knn_jet2_qd(C.byref(m), md, _ptr(y_pos), _ptr(x_pos), _ptr(f_y), _ptr(src_table), _ptr(nbr), k, q,
                                           _ptr(qdirs), nd, _ptr(out), _ptr(d1), _ptr(d2), _stream()), "gaot_gno_fwd_knn_jet2_qd")
    return out, d1, d2


def gno_forward_jet2_qd(mode, weights, biases, y_pos: Tensor, x_pos: Tensor, f_y: Optional[Tensor], src_table: Optional[Tensor],
                        g: BipartiteGraph, qdirs: Tensor):
    """``gno_forward_jet2`` (RAGGED rows) along PER-QUERY directions (gaot_gno_fwd_jet2_qd): ``qdirs`` as in
    ``gno_forward_knn_jet2_qd`` -> (out [n_query, 32], d1 [nd, n_query, 32], d2 [nd, n_query, 32]); an empty row gives exact zeros in
    all 1 + 2 nd planes.  Two launches (the jet kernel and one fix-up over all planes), the workspace of ``gno_forward_jet2``; on a
    list of equal rows of k in ``GNO_KNN_K`` edges every plane is ``gno_forward_knn_jet2_qd``'s, bit for bit."""
    lib = _lib.load()
    md, m, keep, y_pos, x_pos, f_y, src_table, g, q = _gno_mode_args("gno_forward_jet2_qd", mode, weights, biases, y_pos, x_pos, f_y,
                                                                     src_table, g)
    qdirs, nd = _query_dirs("gno_forward_jet2_qd", qdirs, x_pos, q)
    e = g.by_dst.num_edges
    out, d1, d2 = _gno_planes(x_pos, q, m, nd, nd)
    ws = _ws(lib.gaot_gno_fwd_jet2_workspace_bytes(e, min(max(nd, 0), 6)), x_pos.device)
    with _timed(f"gno_jet2_rows_qd{f'_nl{md}' if md else ''}_nh{m.n_hidden}_d{nd}"):
        check(lib.gaot_gno_fwd_jet2_qd(C.byref(m), md, _ptr(y_pos), _ptr(x_pos), _ptr(f_y), _ptr(src_table), _ptr(g.by_dst.other),
                                       _ptr(g.by_dst.key), _ptr(g.by_dst.rowptr), e, q, _ptr(qdirs), nd, _ptr(out), _ptr(d1), _ptr(d2),
                                       _ptr(ws), ws.numel(), _stream()), "gaot_gno_fwd_jet2_qd")
    return out, d1, d2


def gno_nl_backward(mode, weights, biases, y_pos: Tensor, x_pos: Tensor, f_y: Optional[Tensor], src_table: Tensor, grad_out: Tensor,
                    g: BipartiteGraph, precision: Optional[int] = None, coords: bool = False):
    """-> (grad_f_y, grad_src_table, [grad_w...], [grad_b...]); with ``coords`` also (grad_y_pos, grad_x_pos) appended.
    grad_src_table[s] = the sum of dz_0 over the edges of source s ([n_src, 64]); grad_f_y is the gs * k term of 'nonlinear' alone
    (None for 'nonlinear_kernelonly'): the terms through src_table -- dW_0f = grad_src_table^T f_y, grad f_y += grad_src_table W_0f --
    are per-node products of the caller's."""
    lib = _lib.load()
    prec = _PRECISION["mode"] if precision is None else precision
    md, m, keep, y_pos, x_pos, f_y, src_table = _gno_nl_args(mode, weights, biases, y_pos, x_pos, f_y, src_table, g)
    grad_out = _req(grad_out, torch.float32, "grad_out")
    if tuple(grad_out.shape) != (g.num_dst, m.channels):
        raise GaotError(f"grad_out must be [{g.num_dst}, {m.channels}], got {tuple(grad_out.shape)}")
    e = g.by_src.num_edges
    dev = x_pos.device
    grad_f = torch.empty(g.num_src, m.channels, dtype=torch.float32, device=dev) if md == 1 else None
    grad_t = torch.empty(g.num_src, 64, dtype=torch.float32, device=dev)
    gw = [torch.empty(tuple(w.shape[:2]), dtype=torch.float32, device=dev) for w in weights]
    gb = [torch.empty(tuple(b.shape), dtype=torch.float32, device=dev) for b in biases]
    gs = MlpGradT()
    for l in range(len(weights)):
        gs.weight[l] = gw[l].data_ptr()
        gs.bias[l] = gb[l].data_ptr()
    ws = _ws(lib.gaot_gno_bwd_nl_workspace_bytes(C.byref(m), e, g.num_dst), dev)
    gec = torch.empty(e, 6, dtype=torch.float32, device=dev) if coords else None
    with _timed(f"gno_bwd_nl{md}{'_coords' if coords else ''}_nh{m.n_hidden}"):
        check(lib.gaot_gno_bwd_nl(C.byref(m), md, _ptr(y_pos), _ptr(x_pos), _ptr(f_y), _ptr(src_table), _ptr(grad_out),
                                  _ptr(g.by_dst.rowptr), _ptr(g.by_src.key), _ptr(g.by_src.other), _ptr(g.by_src.rowptr), e,
                                  g.num_src, g.num_dst, _ptr(grad_f), _ptr(grad_t), C.byref(gs), _ptr(gec), prec, _ptr(ws),
                                  ws.numel(), _stream()), "gaot_gno_bwd_nl")
    if coords:
        from . import edgeops as EO
        gy = EO.segment_reduce(gec, g.by_src.rowptr, None, g.num_src, EO.SUM, col0=0, channels=3)
        gx = EO.segment_reduce(gec, g.by_dst.rowptr, EO.dst_to_src_map(g), g.num_dst, EO.SUM, col0=3, channels=3)
        return grad_f, grad_t, gw, gb, gy, gx
    return grad_f, grad_t, gw, gb


GNO_W_MODES = {"linear": 0, "nonlinear": 1, "nonlinear_kernelonly": 2}      # csrc/gno_common.h MODE_*


def _gno_w_args(mode, weights, biases, y_pos: Tensor, x_pos: Tensor, f_y: Optional[Tensor], src_table: Optional[Tensor],
                edge_w: Tensor, g: BipartiteGraph):
    """shape checks of the weighted transform: those of ``_gno_nl_args`` (mode 0: no src_table), and edge_w [E] fp32"""
    md = GNO_W_MODES.get(mode, mode)
    if md not in (0, 1, 2):
        raise GaotError(f"gno (weighted): mode must be one of {tuple(GNO_W_MODES)}, got {mode!r}")
    if md == 0:
        m, keep = _mlp_struct(weights, biases)
        y_pos = _req(y_pos, torch.float32, "y_pos")
        x_pos = _req(x_pos, torch.float32, "x_pos")
        if y_pos.shape[0] != g.num_src or x_pos.shape[0] != g.num_dst:
            raise GaotError(f"y_pos / x_pos have {y_pos.shape[0]} / {x_pos.shape[0]} rows, the graph {g.num_src} / {g.num_dst}")
        f_y = _req(f_y, torch.float32, "f_y")
        if tuple(f_y.shape) != (g.num_src, m.channels):
            raise GaotError(f"f_y must be [{g.num_src}, {m.channels}], got {tuple(f_y.shape)}")
        src_table = None
    else:
        md, m, keep, y_pos, x_pos, f_y, src_table = _gno_nl_args(md, weights, biases, y_pos, x_pos, f_y, src_table, g)
    edge_w = _req(edge_w, torch.float32, "edge_w")
    if tuple(edge_w.shape) != (g.by_dst.num_edges,):
        raise GaotError(f"edge_w must be [{g.by_dst.num_edges}] (one weight per edge, dst-sorted order), got {tuple(edge_w.shape)}")
    return md, m, keep, y_pos, x_pos, f_y, src_table, edge_w


def gno_w_forward(mode, weights, biases, y_pos: Tensor, x_pos: Tensor, f_y: Optional[Tensor], src_table: Optional[Tensor],
                  edge_w: Tensor, g: BipartiteGraph, precision: Optional[int] = None) -> Tensor:
    """the fused WEIGHTED transform out_q = sum_{e -> q} edge_w[e] k_e f_y[s_e] (use_attn: a weight per edge in the dst-sorted
    order, rows summed) for ``mode`` 'linear' (src_table None), 'nonlinear' or 'nonlinear_kernelonly' (f_y None); the other
    operands as in ``gno_forward`` / ``gno_nl_forward``"""
    lib = _lib.load()
    prec = _PRECISION["mode"] if precision is None else precision
    md, m, keep, y_pos, x_pos, f_y, src_table, edge_w = _gno_w_args(mode, weights, biases, y_pos, x_pos, f_y, src_table, edge_w, g)
    q, e = g.num_dst, g.by_dst.num_edges
    out = torch.empty(q, m.channels, dtype=torch.float32, device=x_pos.device)
    ws = _ws(lib.gaot_gno_fwd_workspace_bytes(e, m.channels), x_pos.device)
    with _timed(f"gno_fwd_w{md}_nh{m.n_hidden}"):
        check(lib.gaot_gno_fwd_w(C.byref(m), md, _ptr(y_pos), _ptr(x_pos), _ptr(f_y), _ptr(src_table), _ptr(edge_w),
                                 _ptr(g.by_dst.other), _ptr(g.by_dst.key), _ptr(g.by_dst.rowptr), e, q, _ptr(out), prec, _ptr(ws),
                                 ws.numel(), _stream()), "gaot_gno_fwd_w")
    return out


def gno_w_backward(mode, weights, biases, y_pos: Tensor, x_pos: Tensor, f_y: Optional[Tensor], src_table: Optional[Tensor],
                   edge_w: Tensor, grad_out: Tensor, g: BipartiteGraph, precision: Optional[int] = None, want_grad_w: bool = True):
    """-> (grad_f_y, grad_src_table, [grad_w...], [grad_b...], grad_edge_w): as ``gno_nl_backward`` (grad_src_table None for
    'linear', grad_f_y None for 'nonlinear_kernelonly'), and grad_edge_w[e] = sum_c grad_out[q_e, c] k_e[c] f_y[s_e, c] in the
    dst-sorted order (None unless ``want_grad_w``: the kernel then skips its reduction over the channels)"""
    lib = _lib.load()
    prec = _PRECISION["mode"] if precision is None else precision
    md, m, keep, y_pos, x_pos, f_y, src_table, edge_w = _gno_w_args(mode, weights, biases, y_pos, x_pos, f_y, src_table, edge_w, g)
    grad_out = _req(grad_out, torch.float32, "grad_out")
    if tuple(grad_out.shape) != (g.num_dst, m.channels):
        raise GaotError(f"grad_out must be [{g.num_dst}, {m.channels}], got {tuple(grad_out.shape)}")
    from . import edgeops as EO
    e = g.by_src.num_edges
    dev = x_pos.device
    grad_f = torch.empty(g.num_src, m.channels, dtype=torch.float32, device=dev) if md != 2 else None
    grad_t = torch.empty(g.num_src, 64, dtype=torch.float32, device=dev) if md != 0 else None
    grad_ew = torch.empty(e, dtype=torch.float32, device=dev) if want_grad_w else None
    gw = [torch.empty(tuple(w.shape[:2]), dtype=torch.float32, device=dev) for w in weights]
    gb = [torch.empty(tuple(b.shape), dtype=torch.float32, device=dev) for b in biases]
    gs = MlpGradT()
    for l in range(len(weights)):
        gs.weight[l] = gw[l].data_ptr()
        gs.bias[l] = gb[l].data_ptr()
    s2d = EO.src_to_dst_map(g)
    ws = _ws(lib.gaot_gno_bwd_w_workspace_bytes(C.byref(m), e, g.num_dst), dev)
    with _timed(f"gno_bwd_w{md}_nh{m.n_hidden}"):
        check(lib.gaot_gno_bwd_w(C.byref(m), md, _ptr(y_pos), _ptr(x_pos), _ptr(f_y), _ptr(src_table), _ptr(grad_out), _ptr(edge_w),
                                 _ptr(s2d), _ptr(g.by_src.key), _ptr(g.by_src.other), _ptr(g.by_src.rowptr), e, g.num_src,
                                 g.num_dst, _ptr(grad_f), _ptr(grad_t), C.byref(gs), _ptr(grad_ew), prec, _ptr(ws), ws.numel(),
                                 _stream()), "gaot_gno_bwd_w")
    return grad_f, grad_t, gw, gb, grad_ew


EDGE_BILINEAR_WS_BYTES = 65536      # include/gaot3d_hip.h GAOT_EDGE_BILINEAR_WS_BYTES


def _bilinear_args(x_pos: Tensor, y_pos: Tensor, g: BipartiteGraph):
    x_pos = _req(x_pos, torch.float32, "x_pos")
    y_pos = _req(y_pos, torch.float32, "y_pos")
    if x_pos.dim() != 2 or y_pos.dim() != 2 or x_pos.shape[1] != 3 or y_pos.shape[1] != 3 or x_pos.shape[0] < g.num_dst \
            or y_pos.shape[0] < g.num_src:
        raise GaotError(f"edge_bilinear: x_pos / y_pos must be [>= {g.num_dst}, 3] / [>= {g.num_src}, 3], got {tuple(x_pos.shape)} / "
                        f"{tuple(y_pos.shape)}")
    return x_pos, y_pos


def edge_bilinear_forward(x_pos: Tensor, y_pos: Tensor, g: BipartiteGraph, m: Tensor, scale: float) -> Tensor:
    """scores[e] = scale * [x_pos[q_e], 1]^T m [y_pos[s_e], 1] in the dst-sorted edge order; m: [4, 4] fp32 on the device"""
    lib = _lib.load()
    x_pos, y_pos = _bilinear_args(x_pos, y_pos, g)
    m = _req(m, torch.float32, "m")
    if tuple(m.shape) != (4, 4):
        raise GaotError(f"edge_bilinear: m must be [4, 4], got {tuple(m.shape)}")
    e = g.by_dst.num_edges
    out = torch.empty(e, dtype=torch.float32, device=x_pos.device)
    with _timed("edge_bilinear_fwd"):
        check(lib.gaot_edge_bilinear_fwd(_ptr(x_pos), _ptr(y_pos), _ptr(g.by_dst.other), _ptr(g.by_dst.key), e, _ptr(m), float(scale),
                                         _ptr(out), _stream()), "gaot_edge_bilinear_fwd")
    return out


def edge_bilinear_backward(x_pos: Tensor, y_pos: Tensor, g: BipartiteGraph, dscores: Tensor, scale: float) -> Tensor:
    """dm [4, 4] = scale * sum_e dscores[e] [x_pos[q_e], 1] [y_pos[s_e], 1]^T (dscores in the dst-sorted order); fixed summation order"""
    lib = _lib.load()
    x_pos, y_pos = _bilinear_args(x_pos, y_pos, g)
    dscores = _req(dscores, torch.float32, "dscores")
    e = g.by_dst.num_edges
    if tuple(dscores.shape) != (e,):
        raise GaotError(f"edge_bilinear: dscores must be [{e}], got {tuple(dscores.shape)}")
    dm = torch.empty(4, 4, dtype=torch.float32, device=x_pos.device)
    ws = _ws(EDGE_BILINEAR_WS_BYTES, x_pos.device)
    with _timed("edge_bilinear_bwd"):
        check(lib.gaot_edge_bilinear_bwd(_ptr(x_pos), _ptr(y_pos), _ptr(g.by_dst.other), _ptr(g.by_dst.key), e, _ptr(dscores),
                                         float(scale), _ptr(dm), _ptr(ws), ws.numel(), _stream()), "gaot_edge_bilinear_bwd")
    return dm


# ------------------------------------------------------------------------------------------------
# precision switch: "fp32" = exact-fp32 MFMA everywhere (parity mode); "bf16" = bf16 operands with
# fp32 accumulation for the dense GEMMs / attention (BASELINE config 1)
# ------------------------------------------------------------------------------------------------
_PRECISION = {"mode": 0}
_ATTN_F32_FUSED = os.environ.get("GAOT_ATTN_F32_FUSED", "1") != "0"    # fp32 mode: the one-pass attention backward (A/B switch)
_ATTN_F32_FUSED_CAP = int(os.environ.get("GAOT_ATTN_F32_FUSED_MAX_MB", "4096")) << 20     # ... while its slab partials fit in this


def set_precision(mode: str):
    if mode not in ("fp32", "bf16"):
        raise ValueError(f"precision must be 'fp32' or 'bf16', got {mode}")
    _PRECISION["mode"] = 0 if mode == "fp32" else 1


def get_precision() -> str:
    return "bf16" if _PRECISION["mode"] else "fp32"


@contextlib.contextmanager
def fp32_arithmetic():
    """run the enclosed calls in fp32 mode whatever the mode set, and put the mode back (the sampled field's adjoint and the forward it
    recomputes are exact fp32 in both precision modes)"""
    was = _PRECISION["mode"]
    _PRECISION["mode"] = 0
    try:
        yield
    finally:
        _PRECISION["mode"] = was


# activation ids of the GEMM epilogues / gaot_act_bwd (csrc/common.h GAOT_ACT_*)
ACT = {None: 0, "none": 0, "gelu": 1, "relu": 2, "silu": 3, "tanh": 4, "leaky_relu": 5, "elu": 6, "sigmoid": 7, "softplus": 8,
       "selu": 9, "relu6": 10, "hardswish": 11, "mish": 12, "gelu_tanh": 13}


def gemm(a: Tensor, b: Tensor, m: int, n: int, k: int, lda: int, ldb: int, a_trans: bool, b_trans: bool,
         bias: Optional[Tensor] = None, act: int = 0, residual: Optional[Tensor] = None, ldr: int = 0,
         want_preact: bool = False, out: Optional[Tensor] = None, ldc: Optional[int] = None,
         precision: Optional[int] = None, out_dtype: torch.dtype = torch.float32):
    """Raw GEMM on 2-D row-major buffers (see include/gaot3d_hip.h: gaot_gemm / gaot_gemm_ex).  Operands are fp32;
    a bf16 tensor (an FFN intermediate of the bf16 path) is passed through as bf16-in-memory."""
    lib = _lib.load()
    dev = a.device
    if out is None:
        out = torch.empty(m, n, dtype=out_dtype, device=dev)
        ldc = n
    pre = torch.empty(m, n, dtype=torch.float32, device=dev) if want_preact else None
    if want_preact and ldc != n:
        raise GaotError("preact output requires a dense output")
    nb = lib.gaot_gemm_workspace_bytes(m, n, k)
    ws = _ws(nb, dev) if nb else None
    prec = _PRECISION["mode"] if precision is None else precision
    a16, b16, c16 = a.dtype == torch.bfloat16, b.dtype == torch.bfloat16, out.dtype == torch.bfloat16
    if a16 or b16 or c16:
        check(lib.gaot_gemm_ex(_ptr(a), _ptr(b), _ptr(out), m, n, k, lda, ldb, ldc, int(a_trans), int(b_trans), int(a16),
                               int(b16), int(c16), _ptr(bias), act, _ptr(residual), ldr, _ptr(pre), prec, _ptr(ws),
                               ws.numel() if ws is not None else 0, _stream()), "gaot_gemm_ex")
    else:
        check(lib.gaot_gemm(_ptr(a), _ptr(b), _ptr(out), m, n, k, lda, ldb, ldc, int(a_trans), int(b_trans), _ptr(bias),
                            act, _ptr(residual), ldr, _ptr(pre), prec, _ptr(ws), ws.numel() if ws is not None else 0,
                            _stream()), "gaot_gemm")
    return (out, pre) if want_preact else out


# ---- deferred completion of fixed-order reductions (include/gaot3d_hip.h, ABI 10) -------------------------------------------------
# Weight gradients are read by nobody before the optimizer step.  Their producers (split-K dy^T x products, RMSNorm weight
# gradients, bias column sums) leave their partials in a workspace; ONE gaot_reduce_multi launch at the end of the backward pass
# (an autograd-engine final callback: it runs before loss.backward() / torch.autograd.grad() return) sums them in the very order
# the in-call passes use -- the values are bit-identical, ~90 launches of ~5 us per configs[1] step become two.
class _ReduceDesc(C.Structure):   # gaot_reduce_desc_t
    _fields_ = [("part", C.c_void_p), ("out", C.c_void_p), ("n", C.c_int64), ("parts", C.c_int32), ("lanes", C.c_int32)]


# The deferral is OPT-IN (round 6): a step that knows every parameter has ONE consumer that goes through these operators
# (bench.py, sharding.ShardedStep at world size 1, a trainer after reading INTEGRATION.md §5) calls ``defer_reductions(True)`` or sets
# GAOT_DEFER_REDUCE=1.  Off, every reduction completes inside the call that produced it.
_DEFER = {"enabled": os.environ.get("GAOT_DEFER_REDUCE", "0") == "1",
          "stack": [],            # [(graph-task id, {id(param)})]: the running backward pass and the passes it is nested in
          "pending": [], "pending_bytes": 0,
          "cap_bytes": int(os.environ.get("GAOT_DEFER_CAP_MB", "1024")) << 20}


def defer_reductions(enabled: bool) -> bool:
    """switch the deferral on / off (default OFF; GAOT_DEFER_REDUCE=1 turns it on); returns the previous setting.  Whatever is
    pending is completed first and the per-pass bookkeeping is dropped."""
    prev, _DEFER["enabled"] = _DEFER["enabled"], bool(enabled)
    _flush_pending()
    _DEFER["stack"].clear()
    return prev


def _task_done(task: int) -> None:
    """final callback of graph task ``task``: complete what is pending, forget the pass (and any nested pass above it that died
    without its callback).  A callback that runs outside every autograd node belongs to a TOP-LEVEL pass: nothing below it on the
    stack can be alive (a pass that raised half-way never runs its callbacks) -- drop it all."""
    _flush_pending()
    st = _DEFER["stack"]
    node = getattr(torch._C, "_current_autograd_node", None)
    if node is None or node() is None:
        st.clear()
        return
    for i, (t, _s) in enumerate(st):
        if t == task:
            del st[i:]
            break


def defer_ok(params) -> bool:
    """May the gradients of these parameters be completed at the end of the running backward pass?  Only when the caller opted in
    (``defer_reductions(True)``), inside a backward pass, and only for plain contiguous leaf parameters that nothing can observe
    earlier: no gradient to accumulate into yet (AccumulateGrad then takes the returned tensor itself, no arithmetic on it), no
    tensor / post-accumulate hooks (gradient buckets of a sharded step, user hooks), NO initialised process group whatever its
    size (DistributedDataParallel's reducer hooks the gradient accumulators in C++ at world size 1 too), no create_graph /
    anomaly mode.  A parameter that turns up a second time -- in this pass or in a pass this one is nested in -- completes
    everything pending first and takes the in-call pass.  A NESTED pass (reentrant ``torch.utils.checkpoint``, a custom Function
    calling ``torch.autograd.grad`` in its backward) first completes what the enclosing pass left pending, then defers on its own
    list, completed by its own final callback.  ``params=None`` (callers that cannot name their parameters): no.

    What this cannot see: a gradient that reaches one of these parameters through a plain torch op in the same
    pass (a weight regulariser, weight tying through torch ops) -- the engine would add it to a buffer whose values do not exist
    yet.  Hence opt-in."""
    if params is None or not _DEFER["enabled"]:
        return False
    dist = torch.distributed
    if dist.is_available() and dist.is_initialized():
        return False
    get_task = getattr(torch._C, "_current_graph_task_id", None)      # (a private hook of the autograd engine: without it, no deferral)
    task = get_task() if get_task is not None else -1
    if task < 0 or torch.is_grad_enabled() or torch.is_anomaly_enabled():   # not in a backward pass / create_graph / NaN checks
        return False
    st = _DEFER["stack"]
    if not st or st[-1][0] != task:
        at = next((i for i, (t, _s) in enumerate(st) if t == task), -1)
        if at >= 0:
            del st[at + 1:]                 # nested passes above this one ended without their callback (they raised)
        else:
            # a pass we have not seen: top-level, or nested in the one on top of the stack.  What that one left pending is
            # completed NOW (its partials are all written, same stream; the storages are kept alive) -- never dropped
            _flush_pending()
            st.append((task, set()))
            torch.autograd.Variable._execution_engine.queue_callback(functools.partial(_task_done, task))
    ok = True
    for p in params:
        if p is None:
            continue
        if (not p.is_leaf) or p.grad_fn is not None or p.grad is not None or p._backward_hooks \
                or getattr(p, "_post_accumulate_grad_hooks", None) or not p.is_contiguous():
            ok = False
        if any(id(p) in seen for _t, seen in st):
            # the parameter is used twice: the engine is about to ADD this gradient to the one deferred earlier -- complete
            # everything pending now (same stream, ahead of that add) and take the in-call pass
            _flush_pending()
            ok = False
    if ok:
        st[-1][1].update(id(p) for p in params if p is not None)
    return ok


def _defer(part: Tensor, out: Tensor, n: int, parts: int, lanes: int) -> None:
    # `out` is about to be handed to autograd: keep its STORAGE alive, not the tensor -- a second reference to the returned tensor
    # (a view of it holds one too: its base) would make AccumulateGrad clone it, a copy of values that do not exist yet
    _DEFER["pending"].append((part, out.untyped_storage(), out.data_ptr(), int(n), int(parts), int(lanes)))
    # the partial tables stay allocated until the flush (configs[1]: ~70 MB per layer, 0.7 GB per pass): past the cap, complete now
    _DEFER["pending_bytes"] += part.numel() * part.element_size()
    if _DEFER["pending_bytes"] > _DEFER["cap_bytes"]:
        _flush_pending()


def flush_deferred() -> None:
    """sum every pending partial table into its output (one launch per 64 tables) -- safe at any time: the partials of a pending
    entry are complete in stream order the moment it is queued"""
    _flush_pending()


def _flush_pending() -> None:
    pend, _DEFER["pending"], _DEFER["pending_bytes"] = _DEFER["pending"], [], 0
    if not pend:
        return
    arr = (_ReduceDesc * len(pend))()
    for i, (part, _keep, out_ptr, n, parts, lanes) in enumerate(pend):
        arr[i].part, arr[i].out, arr[i].n, arr[i].parts, arr[i].lanes = part.data_ptr(), out_ptr, n, parts, lanes
    check(_lib.load().gaot_reduce_multi(arr, len(pend), _stream()), "gaot_reduce_multi")


def deferred_pending() -> int:
    return len(_DEFER["pending"])


def gemm_dw(a: Tensor, b: Tensor, m: int, n: int, k: int, lda: int, ldb: int, precision: Optional[int] = None,
            defer: bool = False) -> Tensor:
    """the weight-gradient product dW[m, n] = a^T b (a [k, lda], b [k, ldb], reduction over the k rows); ``defer``: its split-K
    completion waits for flush_deferred (see defer_ok)"""
    if not defer:
        return gemm(a, b, m, n, k, lda, ldb, True, False, precision=precision)
    lib = _lib.load()
    dev = a.device
    out = torch.empty(m, n, dtype=torch.float32, device=dev)
    nb = lib.gaot_gemm_workspace_bytes(m, n, k)
    ws = _ws(nb, dev) if nb else None
    prec = _PRECISION["mode"] if precision is None else precision
    splits, lanes = C.c_int(0), C.c_int(0)
    check(lib.gaot_gemm_ex_partials(_ptr(a), _ptr(b), _ptr(out), m, n, k, lda, ldb, n, 1, 0, int(a.dtype == torch.bfloat16),
                                    int(b.dtype == torch.bfloat16), prec, _ptr(ws), ws.numel() if ws is not None else 0,
                                    C.byref(splits), C.byref(lanes), _stream()), "gaot_gemm_ex_partials")
    if splits.value > 1:
        _defer(ws, out, m * n, splits.value, lanes.value)
    return out


def colsum(x: Tensor, m: int, n: int, ld: int, defer: bool = False) -> Tensor:
    lib = _lib.load()
    out = torch.empty(n, dtype=torch.float32, device=x.device)
    ws = _ws(lib.gaot_colsum_workspace_bytes(m, n), x.device)
    if defer and m > 0 and n > 0:
        check(lib.gaot_colsum(_ptr(x), m, n, ld, None, _ptr(ws), ws.numel(), _stream()), "gaot_colsum")
        _defer(ws, out, n, lib.gaot_colsum_parts(m), 32)
        return out
    check(lib.gaot_colsum(_ptr(x), m, n, ld, _ptr(out), _ptr(ws), ws.numel(), _stream()), "gaot_colsum")
    return out


def act_fwd(z: Tensor, act: int) -> Tensor:
    """h = act(z) for the activation ids the GEMM epilogue does not carry (ACT >= 4)"""
    lib = _lib.load()
    h = torch.empty_like(z)
    check(lib.gaot_act_fwd(_ptr(z), _ptr(h), z.numel(), act, _stream()), "gaot_act_fwd")
    return h


def act_bwd(z: Tensor, dh: Tensor, act: int) -> Tensor:
    lib = _lib.load()
    dz = torch.empty_like(z)
    check(lib.gaot_act_bwd(_ptr(z), _ptr(dh), _ptr(dz), z.numel(), act, _stream()), "gaot_act_bwd")
    return dz


def axpy(a: Tensor, b: Tensor, alpha: float = 1.0, period: Optional[int] = None) -> Tensor:
    lib = _lib.load()
    out = torch.empty_like(a)
    check(lib.gaot_axpy(_ptr(a), _ptr(b), float(alpha), _ptr(out), a.numel(), period or a.numel(), _stream()),
          "gaot_axpy")
    return out


def stream_copy_gbps(nbytes: int = 1 << 30, reps: int = 10, variant: Optional[int] = None) -> float:
    """measured float4 streaming-copy rate of this device in GB/s (read + written bytes over the HIP-event time of ``reps``
    copies of ``nbytes``): the practical HBM ceiling quoted beside the 8 TB/s spec figure.  ``variant``: a form of
    gaot_stream_copy_ex (default: the library's fastest)"""
    lib = _lib.load()
    src = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)

    def go():
        if variant is None:
            check(lib.gaot_stream_copy(_ptr(src), _ptr(dst), nbytes, _stream()), "gaot_stream_copy")
        else:
            check(lib.gaot_stream_copy_ex(_ptr(src), _ptr(dst), nbytes, int(variant), _stream()), "gaot_stream_copy_ex")
    for _ in range(2):
        go()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        go()
    b.record()
    torch.cuda.synchronize()
    return 2.0 * nbytes * reps / (a.elapsed_time(b) * 1e-3) / 1e9


def rmsnorm_fwd(x: Tensor, w: Tensor, eps: float, want_bf16: bool = False):
    """-> (y, rstd, y_bf16 | None); the bf16 copy (same rounding a GEMM would apply to y as its A operand) is written by
    the same pass"""
    lib = _lib.load()
    d = x.shape[-1]
    rows = x.numel() // d
    y = torch.empty_like(x)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    yb = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if (want_bf16 and d % 8 == 0) else None
    check(lib.gaot_rmsnorm_fwd(_ptr(x), _ptr(w), _ptr(y), _ptr(rstd), _ptr(yb), rows, d, float(eps), _stream()),
          "gaot_rmsnorm_fwd")
    return y, rstd, yb


def rmsnorm_bwd(x: Tensor, w: Tensor, dy: Tensor, rstd: Tensor, dx_add: Optional[Tensor] = None, defer: bool = False,
                dx_add2: Optional[Tensor] = None):
    """``defer``: the weight gradient's partial rows are summed by flush_deferred (see defer_ok); ``dx_add`` / ``dx_add2``: gradients
    that reach x through other consumers (the block's residual; the U-ViT skip tap), added by the same pass"""
    lib = _lib.load()
    d = x.shape[-1]
    rows = x.numel() // d
    dx = torch.empty_like(x)
    dw = torch.empty_like(w)
    ws = _ws(lib.gaot_rmsnorm_bwd_workspace_bytes(rows, d), x.device)
    if dx_add is not None:
        dx_add = _req(dx_add, torch.float32, "dx_add")
    if dx_add2 is not None:
        dx_add2 = _req(dx_add2, torch.float32, "dx_add2")
        if dx_add is None:
            dx_add, dx_add2 = dx_add2, None
    defer = defer and rows > 0
    if dx_add2 is not None:
        check(lib.gaot_rmsnorm_bwd2(_ptr(x), _ptr(w), _ptr(dy), _ptr(rstd), _ptr(dx_add), _ptr(dx_add2), _ptr(dx), None if defer else _ptr(dw),
                                    rows, d, _ptr(ws), ws.numel(), _stream()), "gaot_rmsnorm_bwd2")
    else:
        check(lib.gaot_rmsnorm_bwd(_ptr(x), _ptr(w), _ptr(dy), _ptr(rstd), _ptr(dx_add), _ptr(dx), None if defer else _ptr(dw), rows, d,
                                   _ptr(ws), ws.numel(), _stream()), "gaot_rmsnorm_bwd")
    if defer:
        _defer(ws, dw, d, lib.gaot_rmsnorm_bwd_parts(rows), 32)
    return dx, dw


def rope_(buf: Tensor, rows: int, ld: int, col0: int, nheads: int, seq_len: int, freqs: Tensor, inverse: bool,
          head_dim: int = 32):
    lib = _lib.load()
    check(lib.gaot_rope(_ptr(buf), rows, ld, col0, nheads, head_dim, seq_len, _ptr(freqs), int(inverse), _stream()),
          "gaot_rope")


def row_softmax(scores: Tensor, grad: Optional[Tensor] = None, w: Optional[Tensor] = None) -> Tensor:
    """softmax over the last axis of a dense [rows, n] fp32 matrix (grad / w given: its backward ds = w (dw - sum(w dw))):
    the per-row segment kernels of csrc/edgeops.hip on the row pointer 0, n, 2n, ..."""
    lib = _lib.load()
    rows, n = scores.shape
    if rows * n >= 2 ** 31:
        raise GaotError("row_softmax: more than 2^31 scores")
    rowptr = torch.arange(0, rows * n + 1, n, dtype=torch.int32, device=scores.device)
    out = torch.empty_like(scores)
    if grad is None:
        check(lib.gaot_segment_softmax_fwd(_ptr(_req(scores, torch.float32, "scores")), _ptr(rowptr), rows, _ptr(out), _stream()),
              "gaot_segment_softmax_fwd")
    else:
        check(lib.gaot_segment_softmax_bwd(_ptr(w), _ptr(_req(grad, torch.float32, "dw")), _ptr(rowptr), rows, _ptr(out), _stream()),
              "gaot_segment_softmax_bwd")
    return out


def _drop_args(p: float, seed: Optional[Tensor]):
    if p <= 0.0:
        return 0.0, None
    if seed is None or seed.dtype != torch.int64 or not seed.is_cuda or seed.numel() != 1:
        raise ValueError("attention dropout needs a one-element int64 device tensor as seed")
    return float(p), _ptr(seed)


def dropout_seed_next(state: Tensor, stride: int) -> Tensor:
    """-> a fresh one-element int64 tensor holding the current seed word; ``state`` advances by ``stride`` (one launch)"""
    lib = _lib.load()
    out = torch.empty(1, dtype=torch.int64, device=state.device)
    check(lib.gaot_dropout_seed_next(_ptr(state), stride & 0xFFFFFFFFFFFFFFFF, _ptr(out), _stream()), "gaot_dropout_seed_next")
    return out


def dropout_seed_block(state: Tensor, stride: int, n: int) -> Tensor:
    """-> int64 [n]: the seed words of the next n dropout calls; ``state`` advances by n * stride (one launch)"""
    lib = _lib.load()
    out = torch.empty(n, dtype=torch.int64, device=state.device)
    check(lib.gaot_dropout_seed_block(_ptr(state), stride & 0xFFFFFFFFFFFFFFFF, int(n), _ptr(out), _stream()), "gaot_dropout_seed_block")
    return out


def dropout(x: Tensor, seed: Tensor, p: float) -> Tensor:
    """x .* keep / (1 - p) with keep(i) = hash(seed, i) >= round(p 2^32)  (include/gaot3d_hip.h: gaot_dropout)"""
    lib = _lib.load()
    x = _req(x, torch.float32, "x")
    out = torch.empty_like(x)
    check(lib.gaot_dropout(_ptr(x), _ptr(seed), float(p), x.numel(), _ptr(out), _stream()), "gaot_dropout")
    return out


def attn_dropout_mask(seed: Tensor, p: float, b: int, h: int, s: int) -> Tensor:
    """keep[b, h, q, k] (uint8) of the attention dropout mask the kernels regenerate from ``seed`` (checks only)"""
    lib = _lib.load()
    keep = torch.empty(b, h, s, s, dtype=torch.uint8, device=seed.device)
    check(lib.gaot_attn_dropout_mask(_ptr(seed), float(p), b, h, s, _ptr(keep), _stream()), "gaot_attn_dropout_mask")
    return keep


def _qkv_args(qkv: Tensor, h: int, hkv: int, head_dim: int, dqkv: Optional[Tensor] = None):
    """the q | k | v column blocks of a fused fp32 [rows, (h + 2 hkv) * head_dim] projection as the attention entry points take them:
    -> ((q, k, v), (ldq, ldk, ldv, ldo)); with the gradient buffer ``dqkv`` of the same layout
    -> ((q, k, v), (dq, dk, dv), (ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv))"""
    ld = qkv.shape[1]
    offs = (0, 4 * h * head_dim, 4 * (h + hkv) * head_dim)      # bytes
    q3 = tuple(C.c_void_p(qkv.data_ptr() + o) for o in offs)
    if dqkv is None:
        return q3, (ld, ld, ld, h * head_dim)
    return q3, tuple(C.c_void_p(dqkv.data_ptr() + o) for o in offs), (ld, ld, ld, h * head_dim, h * head_dim, ld, ld, ld)


def attn_fwd(qkv: Tensor, b: int, s: int, h: int, hkv: int, scale: float, dropout_p: float = 0.0,
             seed: Optional[Tensor] = None, head0: int = 0, heads_total: int = 0):
    """qkv: [B*S, (h + 2*hkv)*32] fused projection output (q | k | v column blocks).  ``head0`` / ``heads_total``: the h heads
    are heads head0 .. of heads_total (a rank's slice): the dropout mask is keyed by the global head index"""
    lib = _lib.load()
    dev = qkv.device
    o = torch.empty(b * s, h * 32, dtype=torch.float32, device=dev)
    lse = torch.empty(b, h, s, dtype=torch.float32, device=dev)
    q3, lds = _qkv_args(qkv, h, hkv, 32)
    with _timed("attn_fwd"):
        dp, sp = _drop_args(dropout_p, seed)
        check(lib.gaot_attn_fwd(*q3, _ptr(o), _ptr(lse), *lds, b, s, h, hkv, 32, float(scale), dp, sp,
                                int(head0), int(heads_total), _PRECISION["mode"], _stream()), "gaot_attn_fwd")
    return o, lse


def attn_bwd(qkv: Tensor, o: Tensor, d_o: Tensor, lse: Tensor, b: int, s: int, h: int, hkv: int, scale: float,
             dropout_p: float = 0.0, seed: Optional[Tensor] = None, head0: int = 0, heads_total: int = 0) -> Tensor:
    lib = _lib.load()
    dp, sp = _drop_args(dropout_p, seed)
    dev = qkv.device
    dqkv = torch.empty_like(qkv)
    delta = torch.empty(b, h, s, dtype=torch.float32, device=dev)
    q3, g3, lds = _qkv_args(qkv, h, hkv, 32, dqkv)
    # dK, dV and dQ from one pass (5 S^2 d products instead of 7); its fp32 dQ slab partials live in a buffer of this call -- b * h *
    # ceil(s / 256) * s * 128 bytes (1.07 GB at S = 16 384, 8 heads; quadratic in S): past the cap the two-pass kernels run
    nb = int(lib.gaot_attn_bwd_fused_f32_scratch_bytes(b, s, h)) if _ATTN_F32_FUSED else 0
    # (a long sequence with few kv heads per launch -- one rank's share of a sharded step -- leaves the one-pass kernel fewer than one
    # workgroup per CU, 256 keys each; the two-pass kernels split twice as fine)
    starved = s >= 4096 and b * hkv * ((s + 255) // 256) < 256
    one_pass = _ATTN_F32_FUSED and nb <= _ATTN_F32_FUSED_CAP and not starved
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev) if one_pass else None
    for name, mask in (("attn_bwd_delta", 1),) if one_pass else (("attn_bwd_delta", 1), ("attn_bwd_dkv", 2), ("attn_bwd_dq", 4)):
        with _timed(name):
            check(lib.gaot_attn_bwd(*q3, _ptr(o), _ptr(d_o), _ptr(lse), _ptr(delta), *g3, *lds, b, s, h, hkv, 32,
                                    float(scale), dp, sp, int(head0), int(heads_total), _PRECISION["mode"], mask, _stream()),
                  "gaot_attn_bwd")
    if one_pass:
        with _timed("attn_bwd_fused_f32"):
            check(lib.gaot_attn_bwd_fused_f32(*q3, _ptr(o), _ptr(d_o), _ptr(lse), _ptr(delta), *g3, *lds, b, s, h, hkv, 32,
                                              float(scale), dp, sp, int(head0), int(heads_total), 0, _ptr(scratch), nb, _stream()),
                  "gaot_attn_bwd_fused_f32")
    return dqkv


HD_HEAD_DIM_RULE = "head_dim must be a multiple of 4 with 4 <= head_dim <= 128"


def attn_hd_head_dim_ok(head_dim: int) -> bool:
    """the head sizes csrc/attn_hd.hip takes (gaot_attn_hd_fwd / gaot_attn_hd_bwd apply the same rule)"""
    return 4 <= head_dim <= 128 and head_dim % 4 == 0


def attn_hd_fwd(qkv: Tensor, b: int, s: int, h: int, hkv: int, head_dim: int, scale: float, dropout_p: float = 0.0,
                seed: Optional[Tensor] = None, head0: int = 0, heads_total: int = 0):
    """flash attention for every head size that is a multiple of 4 up to 128 in bf16 mode (csrc/attn_hd.hip).  qkv: [B*S, (h + 2*hkv)*head_dim] fused fp32
    projection output (q | k | v column blocks), already rotated; -> (o [B*S, h*head_dim], lse [b, h, s]).  ``head0`` /
    ``heads_total`` as in attn_fwd"""
    lib = _lib.load()
    qkv = _req(qkv, torch.float32, "qkv")
    if not attn_hd_head_dim_ok(head_dim):
        raise GaotError(f"attn_hd_fwd: {HD_HEAD_DIM_RULE}, got {head_dim}")
    if qkv.dim() != 2 or tuple(qkv.shape) != (b * s, (h + 2 * hkv) * head_dim):
        raise GaotError(f"attn_hd_fwd: qkv must be [{b * s}, {(h + 2 * hkv) * head_dim}], got {tuple(qkv.shape)}")
    dev = qkv.device
    o = torch.empty(b * s, h * head_dim, dtype=torch.float32, device=dev)
    lse = torch.empty(b, h, s, dtype=torch.float32, device=dev)
    q3, lds = _qkv_args(qkv, h, hkv, head_dim)
    with _timed("attn_hd_fwd"):
        dp, sp = _drop_args(dropout_p, seed)
        check(lib.gaot_attn_hd_fwd(*q3, _ptr(o), _ptr(lse), *lds, b, s, h, hkv, head_dim, float(scale),
                                   dp, sp, int(head0), int(heads_total), _stream()), "gaot_attn_hd_fwd")
    return o, lse


def attn_hd_bwd(qkv: Tensor, o: Tensor, d_o: Tensor, lse: Tensor, b: int, s: int, h: int, hkv: int, head_dim: int,
                scale: float, dropout_p: float = 0.0, seed: Optional[Tensor] = None, head0: int = 0,
                heads_total: int = 0) -> Tensor:
    """-> dqkv, the gradient w.r.t. the (rotated) fused projection, in its layout; delta, dK / dV and dQ are three launches"""
    lib = _lib.load()
    dp, sp = _drop_args(dropout_p, seed)
    qkv = _req(qkv, torch.float32, "qkv")
    o = _req(o, torch.float32, "o")
    d_o = _req(d_o, torch.float32, "d_o")
    lse = _req(lse, torch.float32, "lse")
    if not attn_hd_head_dim_ok(head_dim):
        raise GaotError(f"attn_hd_bwd: {HD_HEAD_DIM_RULE}, got {head_dim}")
    if tuple(qkv.shape) != (b * s, (h + 2 * hkv) * head_dim) or tuple(o.shape) != (b * s, h * head_dim) or o.shape != d_o.shape \
            or lse.numel() != b * h * s:
        raise GaotError("attn_hd_bwd: qkv / o / d_o / lse do not match (b, s, h, hkv, head_dim)")
    dqkv = torch.empty_like(qkv)
    delta = torch.empty(b, h, s, dtype=torch.float32, device=qkv.device)
    q3, g3, lds = _qkv_args(qkv, h, hkv, head_dim, dqkv)
    for name, mask in (("attn_hd_bwd_delta", 1), ("attn_hd_bwd_dkv", 2), ("attn_hd_bwd_dq", 4)):
        with _timed(name):
            check(lib.gaot_attn_hd_bwd(*q3, _ptr(o), _ptr(d_o), _ptr(lse), _ptr(delta), *g3, *lds, b, s, h, hkv,
                                       head_dim, float(scale), dp, sp, int(head0), int(heads_total), mask, _stream()),
                  "gaot_attn_hd_bwd")
    return dqkv


def attn_fwd_bf16(qkv: Optional[Tensor], freqs: Optional[Tensor], b: int, s: int, h: int, hkv: int, scale: float,
                  dropout_p: float = 0.0, seed: Optional[Tensor] = None, image: Optional[Tensor] = None, head0: int = 0,
                  heads_total: int = 0):
    """bf16 matrix-core attention on the fused fp32 projection; returns (o, lse, bf16 image kept for backward).
    ``image``: the projection already written as the kernels' image (qkv_image): qkv is then not read"""
    lib = _lib.load()
    dev = image.device if image is not None else qkv.device
    o = torch.empty(b * s, h * 32, dtype=torch.float32, device=dev)
    lse = torch.empty(b, h, s, dtype=torch.float32, device=dev)
    img = image if image is not None else _ws(lib.gaot_attn_bf16_image_bytes(b, s, h, hkv), dev)
    with _timed("attn_fwd"):
        dp, sp = _drop_args(dropout_p, seed)
        check(lib.gaot_attn_fwd_bf16(_ptr(None if image is not None else qkv), _ptr(freqs), _ptr(img), _ptr(o), _ptr(lse), b, s,
                                     h, hkv, 32, float(scale), dp, sp, int(head0), int(heads_total), _stream()), "gaot_attn_fwd_bf16")
    return o, lse, img


_ROPE_TABLES: dict = {}


def rope_table(freqs: Tensor, s: int) -> Tensor:
    """[s, 16, 2] (cos, sin) of position * frequency for a 32-wide head, cached per (frequencies, s): the frequencies are a
    frozen parameter, so the table is built once"""
    key = (id(freqs), int(s))
    ent = _ROPE_TABLES.get(key)
    # the entry holds the frequencies tensor itself: validated by identity + in-place version, never by address (an
    # address can be re-used by another model's frequencies)
    if ent is not None and ent[0] is freqs and ent[1] == freqs._version:
        _ROPE_TABLES[key] = _ROPE_TABLES.pop(key)     # most recently used last
        return ent[2]
    if freqs.numel() != 16 or freqs.dtype != torch.float32:
        raise GaotError("rope_table: 16 fp32 frequencies (head_dim 32) expected")
    t = torch.empty(s, 16, 2, dtype=torch.float32, device=freqs.device)
    check(_lib.load().gaot_rope_table(_ptr(freqs), int(s), 16, _ptr(t), _stream()), "gaot_rope_table")
    _ROPE_TABLES.pop(key, None)
    _ROPE_TABLES[key] = (freqs, freqs._version, t)
    while len(_ROPE_TABLES) > 64:                     # evict the least recently used entry only (a captured graph may
        _ROPE_TABLES.pop(next(iter(_ROPE_TABLES)))    # still reference the tables of the live models)
    return t


def qkv_image(xb: Tensor, wcat: Tensor, rows: int, b: int, s: int, h: int, hkv: int, freqs: Optional[Tensor],
              scale: float) -> Tensor:
    """x [rows, 256] bf16 times the co-located q|k|v weights [(h + 2 hkv) * 32, 256] bf16, written straight as the attention
    kernels' bf16 image (RoPE on q and k, q pre-scaled): the fp32 projection never exists (csrc/gemm_k256.hip)"""
    lib = _lib.load()
    if xb.dtype != torch.bfloat16 or wcat.dtype != torch.bfloat16 or not (xb.is_contiguous() and wcat.is_contiguous()):
        raise GaotError("qkv_image: contiguous bf16 operands expected")
    img = _ws(lib.gaot_attn_bf16_image_bytes(b, s, h, hkv), xb.device)
    table = rope_table(freqs, s) if freqs is not None else None
    with _timed("qkv_image"):
        check(lib.gaot_qkv_image(_ptr(xb), _ptr(wcat), _ptr(img), rows, xb.shape[1], wcat.shape[1], s, h, hkv, _ptr(table),
                                 _qscale(scale), _stream()), "gaot_qkv_image")
    return img


def attn_bwd_scratch(b: int, s: int, h: int, hkv: int, device) -> Tensor:
    """the backward's scratch buffer; its first b*s*h*32 bf16 elements are the dO image"""
    return _ws(_lib.load().gaot_attn_bwd_bf16_scratch_bytes(b, s, h, hkv), device)


def attn_bwd_bf16(img: Tensor, o: Tensor, d_o: Optional[Tensor], lse: Tensor, b: int, s: int, h: int, hkv: int, scale: float,
                  dropout_p: float = 0.0, seed: Optional[Tensor] = None, freqs: Optional[Tensor] = None,
                  do_image: Optional[Tensor] = None, fused: Optional[bool] = None, head0: int = 0, heads_total: int = 0,
                  delta: Optional[Tensor] = None) -> Tensor:
    """``freqs``: the forward's RoPE frequencies -> the returned dq / dk are w.r.t. the UNrotated projection.
    ``do_image`` (instead of d_o): an attn_bwd_scratch buffer whose head already holds the bf16 dO (sequence-parallel
    exchange): only delta is computed from it.
    ``fused``: dK / dV / dQ from one pass over the score tiles (csrc/attn_bf16.hip: k_attn_bwd_fused) instead of the dK/dV
    pass + the dQ pass; default: whenever its grid fills the chip (gaot_attn_bwd_bf16_fused_eligible)"""
    lib = _lib.load()
    dp, sp = _drop_args(dropout_p, seed)
    dev = o.device
    dqkv = torch.empty(b * s, (h + 2 * hkv) * 32, dtype=torch.float32, device=dev)
    have_delta = delta is not None      # ``delta`` (with do_image): the row constants are already there too (oproj_bwd_image): no first phase
    if have_delta and (do_image is None or tuple(delta.shape) != (b, h, s) or delta.dtype != torch.float32):
        raise GaotError("attn_bwd_bf16: delta needs do_image and the shape [b, h, s]")
    if not have_delta:
        delta = torch.empty(b, h, s, dtype=torch.float32, device=dev)
    doimg = do_image if do_image is not None else attn_bwd_scratch(b, s, h, hkv, dev)
    can_fuse = bool(lib.gaot_attn_bwd_bf16_fused_eligible(b, s, h, hkv))
    if fused and not can_fuse:
        raise GaotError("attn_bwd_bf16: the fused backward needs >= 128 workgroups (ceil(S/512) * hkv * b, times up to 8 query "
                        "parts of >= 1024 rows) and <= 1 GiB of dQ slab partials")
    phases = ((("attn_bwd", 16), ("attn_bwd_dq_reduce", 32)) if (can_fuse if fused is None else fused)
              else (("attn_bwd_dkv", 2), ("attn_bwd_dq", 4)))
    first = () if have_delta else (("attn_bwd_delta", 8 if do_image is not None else 1),)
    for name, mask in first + phases:
        with _timed(name):
            check(lib.gaot_attn_bwd_bf16(_ptr(img), _ptr(o), _ptr(d_o), _ptr(lse), _ptr(doimg), _ptr(delta), _ptr(dqkv),
                                         _ptr(freqs), b, s, h, hkv, 32, float(scale), dp, sp, int(head0), int(heads_total), mask,
                                         _stream()), "gaot_attn_bwd_bf16")
    return dqkv


def _qscale(scale: float) -> float:
    """fp32(scale) * fp32(log2 e), rounded once in fp32 (host arithmetic: numpy, not a torch op on the step's path)"""
    import numpy as np
    return float(np.float32(scale) * np.float32(1.4426950408889634))


def qkv_image_packed(xb: Tensor, wcat: Tensor, rows: int, pos0: int, s_total: int, h: int, hkv: int, freqs: Optional[Tensor],
                     scale: float, world: int) -> Tensor:
    """the q|k|v projection of this rank's token rows written as the send buffer of the sequence-parallel all-to-all:
    bf16 [world, rows, (h + 2 hkv) / world * 32] (include/gaot3d_hip.h: gaot_qkv_image_packed)"""
    lib = _lib.load()
    if xb.dtype != torch.bfloat16 or wcat.dtype != torch.bfloat16 or not (xb.is_contiguous() and wcat.is_contiguous()):
        raise GaotError("qkv_image_packed: contiguous bf16 operands expected")
    lw = (h + 2 * hkv) // world * 32
    out = torch.empty(world, rows, lw, dtype=torch.bfloat16, device=xb.device)
    table = rope_table(freqs, s_total) if freqs is not None else None
    with _timed("qkv_image"):
        check(lib.gaot_qkv_image_packed(_ptr(xb), _ptr(wcat), _ptr(out), rows, xb.shape[1], wcat.shape[1], int(pos0), h, hkv,
                                        _ptr(table), _qscale(scale), world, _stream()), "gaot_qkv_image_packed")
    return out


_DT = {torch.float32: 0, torch.bfloat16: 1}


def pack_heads(rows_buf: Tensor, blocks: Tensor, world: int, segs, to_blocks: bool) -> None:
    """rows layout [rows, ld] <-> blocks layout [world, rows, sum(width)]; ``segs`` = [(col0, width), ...] (<= 3 column
    segments, each `world` groups of `width` columns); fp32 or bf16 on either side (include/gaot3d_hip.h: gaot_pack_heads)"""
    lib = _lib.load()
    if not (rows_buf.is_contiguous() and blocks.is_contiguous() and rows_buf.is_cuda and blocks.is_cuda):
        raise GaotError("pack_heads: contiguous device tensors expected")
    rows, ld = rows_buf.shape
    col0 = (C.c_int * len(segs))(*[int(c) for c, _ in segs])
    wid = (C.c_int * len(segs))(*[int(w) for _, w in segs])
    if tuple(blocks.shape) != (world, rows, sum(int(w) for _, w in segs)):
        raise GaotError(f"pack_heads: blocks buffer has shape {tuple(blocks.shape)}")
    check(lib.gaot_pack_heads(_ptr(rows_buf), _ptr(blocks), rows, ld, world, len(segs), col0, wid, _DT[rows_buf.dtype],
                              _DT[blocks.dtype], int(to_blocks), _stream()), "gaot_pack_heads")


def swiglu_fwd(ag: Tensor, f: int) -> Tensor:
    lib = _lib.load()
    rows = ag.shape[0]
    u = torch.empty(rows, f, dtype=torch.float32, device=ag.device)
    check(lib.gaot_swiglu_fwd(_ptr(ag), _ptr(u), rows, f, _stream()), "gaot_swiglu_fwd")
    return u


def swiglu_bwd(ag: Tensor, du: Tensor, f: int) -> Tensor:
    lib = _lib.load()
    dag = torch.empty_like(ag)
    check(lib.gaot_swiglu_bwd(_ptr(ag), _ptr(du), _ptr(dag), ag.shape[0], f, _stream()), "gaot_swiglu_bwd")
    return dag


def cast_bf16(x: Tensor) -> Tensor:
    """bf16 copy (round to nearest even) of an fp32 tensor, in the order of its SHAPE (a strided view is copied first)"""
    lib = _lib.load()
    x = _req(x, torch.float32, "x")
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    check(lib.gaot_cast_bf16(_ptr(x), _ptr(out), x.numel(), _stream()), "gaot_cast_bf16")
    return out


class _CastEntry(C.Structure):   # gaot_cast_tensor_t
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("numel", C.c_int64)]


def cast_bf16_multi(xs: Sequence[Tensor]) -> List[Tensor]:
    """bf16 copies of many fp32 tensors in ONE launch; the copies are slices of one buffer (16-byte aligned).  A strided input is
    copied first, in the order of its shape"""
    lib = _lib.load()
    if not xs:
        return []
    flat = _slices_of_one_buffer(len(xs), [x.numel() for x in xs], torch.bfloat16, xs[0].device, align=8)
    outs = [o.view(x.shape) for o, x in zip(flat, xs)]
    entries = (_CastEntry * len(xs))()
    # the contiguous copies _req makes stay referenced until the launch is enqueued: a copy released inside the loop gives its block
    # back to the caching allocator, which hands it to the NEXT input's copy -- two entries of the table then name one address
    srcs = [_req(x, torch.float32, "x") for x in xs]
    for i, (x, o) in enumerate(zip(srcs, outs)):
        entries[i] = _CastEntry(x.data_ptr(), o.data_ptr(), x.numel())
    check(lib.gaot_cast_bf16_multi(entries, len(xs), _stream()), "gaot_cast_bf16_multi")
    return outs


def cast_bf16_transpose_multi(xs: Sequence[Tensor]) -> List[Tensor]:
    """bf16 TRANSPOSED copies ([cols, rows]) of many fp32 matrices in ONE launch.  A strided matrix (a transposed view, a column
    slice) is copied first, like every other operand that goes through _req; anything but a matrix is refused"""
    lib = _lib.load()
    if not xs:
        return []
    for x in xs:
        if x.dim() != 2:
            raise GaotError(f"cast_bf16_transpose_multi: 2-D tensors expected, got shape {tuple(x.shape)}")
    flat = _slices_of_one_buffer(len(xs), [x.numel() for x in xs], torch.bfloat16, xs[0].device, align=8)
    outs = [o.view(x.shape[1], x.shape[0]) for o, x in zip(flat, xs)]
    entries = (_CastEntry * len(xs))()
    rows, cols = (C.c_int * len(xs))(), (C.c_int * len(xs))()
    srcs = [_req(x, torch.float32, "x") for x in xs]     # kept until the launch is enqueued (see cast_bf16_multi)
    for i, (x, o) in enumerate(zip(srcs, outs)):
        entries[i] = _CastEntry(x.data_ptr(), o.data_ptr(), x.numel())
        rows[i], cols[i] = x.shape[0], x.shape[1]
    check(lib.gaot_cast_bf16_transpose_multi(entries, rows, cols, len(xs), _stream()), "gaot_cast_bf16_transpose_multi")
    return outs


def swiglu_fwd_bf16(ag: Tensor, f: int) -> Tensor:
    """bf16 [rows, 2F] -> bf16 [rows, F]"""
    lib = _lib.load()
    u = torch.empty(ag.shape[0], f, dtype=torch.bfloat16, device=ag.device)
    check(lib.gaot_swiglu_fwd_bf16(_ptr(ag), _ptr(u), ag.shape[0], f, _stream()), "gaot_swiglu_fwd_bf16")
    return u


def ffn_w13_swiglu(xb: Tensor, w13b: Tensor, f: int):
    """x [rows, 256] bf16 times the co-located [w1; w3] bf16 weights -> (a | g bf16 [rows, 2F], silu(a) g bf16 [rows, F]) in one
    launch (include/gaot3d_hip.h: gaot_ffn_w13_swiglu)"""
    lib = _lib.load()
    if xb.dtype != torch.bfloat16 or w13b.dtype != torch.bfloat16 or not (xb.is_contiguous() and w13b.is_contiguous()):
        raise GaotError("ffn_w13_swiglu: contiguous bf16 operands expected")
    rows = xb.shape[0]
    ag = torch.empty(rows, 2 * f, dtype=torch.bfloat16, device=xb.device)
    u = torch.empty(rows, f, dtype=torch.bfloat16, device=xb.device)
    with _timed("ffn_w13_swiglu"):
        check(lib.gaot_ffn_w13_swiglu(_ptr(xb), _ptr(w13b), _ptr(ag), _ptr(u), rows, xb.shape[1], w13b.shape[1], int(f), _stream()),
              "gaot_ffn_w13_swiglu")
    return ag, u


def ffn_pack(w13: Tensor, w2: Tensor, f: int, with_backward: bool) -> Tensor:
    """the fp32 co-located [w1; w3] ([2F, 256]) and w2 ([256, F]) as the fragment-ordered bf16 images the fused FFN kernels stream
    (include/gaot3d_hip.h: gaot_ffn_pack); one uint8 buffer"""
    lib = _lib.load()
    _req_rows(w13, torch.float32, 256, "ffn_pack: [w1; w3]", rows=2 * f)
    _req_rows(w2, torch.float32, f, "ffn_pack: w2", rows=256)
    packed = torch.empty(lib.gaot_ffn_packed_bytes(int(f), int(with_backward)), dtype=torch.uint8, device=w13.device)
    check(lib.gaot_ffn_pack(_ptr(w13), _ptr(w2), int(f), _ptr(packed), int(with_backward), _stream()), "gaot_ffn_pack")
    return packed


class _FfnPackItem(C.Structure):   # gaot_ffn_pack_t
    _fields_ = [("w13", C.c_void_p), ("w2", C.c_void_p), ("packed", C.c_void_p)]


def ffn_pack_multi(pairs, f: int, with_backward: bool) -> List[Tensor]:
    """ffn_pack for every (w13, w2) pair of a Transformer in ONE launch; the images are slices of one buffer"""
    lib = _lib.load()
    pairs = list(pairs)
    if not pairs:
        return []
    for w13, w2 in pairs:
        _req_rows(w13, torch.float32, 256, "ffn_pack_multi: [w1; w3]", rows=2 * f)
        _req_rows(w2, torch.float32, f, "ffn_pack_multi: w2", rows=256)
    outs = _slices_of_one_buffer(len(pairs), int(lib.gaot_ffn_packed_bytes(int(f), int(with_backward))), torch.uint8, pairs[0][0].device)
    items = (_FfnPackItem * len(pairs))()
    for i, ((w13, w2), o) in enumerate(zip(pairs, outs)):
        items[i] = _FfnPackItem(w13.data_ptr(), w2.data_ptr(), o.data_ptr())
    check(lib.gaot_ffn_pack_multi(items, len(pairs), int(f), int(with_backward), _stream()), "gaot_ffn_pack_multi")
    return outs


def ffn_fwd(xb: Tensor, packed: Tensor, f: int, residual: Optional[Tensor] = None, save: bool = True):
    """y = w2(silu(w1 x) * w3 x) + residual in one launch (include/gaot3d_hip.h: gaot_ffn_fwd): x [rows, 256] bf16, ``packed`` from
    ffn_pack -> (y fp32 [rows, 256], a | g bf16 [rows, 2F] or None, u bf16 [rows, F] or None)"""
    lib = _lib.load()
    rows = _req_rows(xb, torch.bfloat16, 256, "ffn_fwd: input")
    if residual is not None:
        _req_rows(residual, torch.float32, 256, "ffn_fwd: residual", dense=False, rows=rows)
    y = torch.empty(rows, 256, dtype=torch.float32, device=xb.device)
    ag = torch.empty(rows, 2 * f, dtype=torch.bfloat16, device=xb.device) if save else None
    u = torch.empty(rows, f, dtype=torch.bfloat16, device=xb.device) if save else None
    with _timed("ffn_fwd"):
        check(lib.gaot_ffn_fwd(_ptr(xb), _ptr(packed), _ptr(residual), residual.stride(0) if residual is not None else 0, _ptr(y),
                               _ptr(ag), _ptr(u), rows, int(f), _stream()), "gaot_ffn_fwd")
    return y, ag, u


class _BlockPackItem(C.Structure):   # gaot_block_pack_t
    _fields_ = [("w13", C.c_void_p), ("w2", C.c_void_p), ("wo", C.c_void_p), ("packed", C.c_void_p)]


def block_pack_multi(triples, f: int) -> List[Tensor]:
    """ffn_pack_multi with the backward images plus the fragment image of o_proj.weight, for every (w13, w2, wo) of a Transformer in ONE
    launch (include/gaot3d_hip.h: gaot_block_pack_multi); the images are slices of one buffer"""
    lib = _lib.load()
    triples = list(triples)
    if not triples:
        return []
    for w13, w2, wo in triples:
        _req_rows(w13, torch.float32, 256, "block_pack_multi: [w1; w3]", rows=2 * f)
        _req_rows(w2, torch.float32, f, "block_pack_multi: w2", rows=256)
        _req_rows(wo, torch.float32, 256, "block_pack_multi: o_proj", rows=256)
    outs = _slices_of_one_buffer(len(triples), int(lib.gaot_block_packed_bytes(int(f))), torch.uint8, triples[0][0].device)
    items = (_BlockPackItem * len(triples))()
    for i, ((w13, w2, wo), o) in enumerate(zip(triples, outs)):
        items[i] = _BlockPackItem(w13.data_ptr(), w2.data_ptr(), wo.data_ptr(), o.data_ptr())
    check(lib.gaot_block_pack_multi(items, len(triples), int(f), _stream()), "gaot_block_pack_multi")
    return outs


def block_tail_fwd(attn_out: Tensor, x: Tensor, norm_weight: Tensor, eps: float, packed: Tensor, f: int):
    """h = x + o_proj(attn_out); n = RMSNorm(h); y = n + ffn(n) in one launch (include/gaot3d_hip.h: gaot_block_tail_fwd) ->
    (y fp32 [rows, 256], h fp32 [rows, 256], yb = bf16(n), rstd [rows]); ``packed`` from block_pack_multi"""
    lib = _lib.load()
    rows = attn_out.shape[0]
    for t, nm in ((attn_out, "attn_out"), (x, "x")):
        _req_rows(t, torch.float32, 256, f"block_tail_fwd: {nm}", dense=False, rows=rows)
    nw = _req(norm_weight, torch.float32, "norm_weight")
    dev = attn_out.device
    y = torch.empty(rows, 256, dtype=torch.float32, device=dev)
    h = torch.empty(rows, 256, dtype=torch.float32, device=dev)
    yb = torch.empty(rows, 256, dtype=torch.bfloat16, device=dev)
    rstd = torch.empty(rows, dtype=torch.float32, device=dev)
    with _timed("block_tail_fwd"):
        check(lib.gaot_block_tail_fwd(_ptr(attn_out), attn_out.stride(0), _ptr(x), x.stride(0), _ptr(nw), float(eps), _ptr(packed), _ptr(h),
                                      _ptr(y), _ptr(yb), _ptr(rstd), rows, int(f), _stream()), "gaot_block_tail_fwd")
    return y, h, yb, rstd


class _QkvPackItem(C.Structure):   # gaot_qkv_pack_t
    _fields_ = [("w", C.c_void_p), ("packed", C.c_void_p)]


def qkv_pack_multi(ws, with_backward: bool) -> List[Tensor]:
    """the co-located fp32 q | k | v weights ([N, 256]) of every block as fragment images in ONE launch (gaot_qkv_pack_multi)"""
    lib = _lib.load()
    ws = list(ws)
    if not ws:
        return []
    n = ws[0].shape[0]
    for w in ws:
        _req_rows(w, torch.float32, 256, "qkv_pack_multi: q | k | v weight", rows=n)
    outs = _slices_of_one_buffer(len(ws), int(lib.gaot_qkv_packed_bytes(n, int(with_backward))), torch.uint8, ws[0].device)
    items = (_QkvPackItem * len(ws))()
    for i, (w, o) in enumerate(zip(ws, outs)):
        items[i] = _QkvPackItem(w.data_ptr(), o.data_ptr())
    check(lib.gaot_qkv_pack_multi(items, len(ws), n, int(with_backward), _stream()), "gaot_qkv_pack_multi")
    return outs


def skip_pack_multi(ws) -> List[Tensor]:
    """skip_proj weights ([256, 512] fp32) of the decoder blocks as fragment images in ONE launch (gaot_skip_pack_multi)"""
    lib = _lib.load()
    ws = list(ws)
    if not ws:
        return []
    for w in ws:
        _req_rows(w, torch.float32, 512, "skip_pack_multi: skip_proj weight", rows=256)
    outs = _slices_of_one_buffer(len(ws), int(lib.gaot_skip_packed_bytes()), torch.uint8, ws[0].device)
    items = (_QkvPackItem * len(ws))()
    for i, (w, o) in enumerate(zip(ws, outs)):
        items[i] = _QkvPackItem(w.data_ptr(), o.data_ptr())
    check(lib.gaot_skip_pack_multi(items, len(ws), _stream()), "gaot_skip_pack_multi")
    return outs


def cat_norm_qkv_image(xa: Tensor, xb: Tensor, skip_packed: Tensor, skip_bias: Optional[Tensor], norm_weight: Tensor, eps: float, packed: Tensor,
                       b: int, s: int, h: int, hkv: int, freqs: Optional[Tensor], scale: float):
    """skip_proj(cat([xa, xb])) + attn_norm + q | k | v image in one launch (gaot_cat_norm_qkv_image) ->
    (image, x_out fp32 [rows, 256], yb, rstd)"""
    lib = _lib.load()
    rows = b * s
    for t in (xa, xb):
        _req_rows(t, torch.float32, 256, "cat_norm_qkv_image: input", dense=False, rows=rows)
    nw = _req(norm_weight, torch.float32, "norm_weight")
    bs = None if skip_bias is None else _req(skip_bias, torch.float32, "skip_bias")
    img = _ws(lib.gaot_attn_bf16_image_bytes(b, s, h, hkv), xa.device)
    xo = torch.empty(rows, 256, dtype=torch.float32, device=xa.device)
    yb = torch.empty(rows, 256, dtype=torch.bfloat16, device=xa.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=xa.device)
    table = rope_table(freqs, s) if freqs is not None else None
    with _timed("cat_norm_qkv_image"):
        check(lib.gaot_cat_norm_qkv_image(_ptr(xa), xa.stride(0), _ptr(xb), xb.stride(0), _ptr(skip_packed), _ptr(bs), _ptr(xo), _ptr(nw), float(eps),
                                          _ptr(packed), _ptr(img), _ptr(yb), _ptr(rstd), rows, s, h, hkv, _ptr(table), _qscale(scale), _stream()),
              "gaot_cat_norm_qkv_image")
    return img, xo, yb, rstd


def norm_qkv_image(x: Tensor, norm_weight: Tensor, eps: float, packed: Tensor, b: int, s: int, h: int, hkv: int, freqs: Optional[Tensor],
                   scale: float):
    """attn_norm + q | k | v projection written as the attention kernels' bf16 image in one launch (gaot_norm_qkv_image) ->
    (image, yb = bf16(norm(x)) [rows, 256], rstd [rows])"""
    lib = _lib.load()
    rows = _req_rows(x, torch.float32, 256, "norm_qkv_image: input", dense=False, rows=b * s)
    nw = _req(norm_weight, torch.float32, "norm_weight")
    img = _ws(lib.gaot_attn_bf16_image_bytes(b, s, h, hkv), x.device)
    yb = torch.empty(rows, 256, dtype=torch.bfloat16, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    table = rope_table(freqs, s) if freqs is not None else None
    with _timed("norm_qkv_image"):
        check(lib.gaot_norm_qkv_image(_ptr(x), x.stride(0), _ptr(nw), float(eps), _ptr(packed), _ptr(img), _ptr(yb), _ptr(rstd), rows, s, h, hkv,
                                      _ptr(table), _qscale(scale), _stream()), "gaot_norm_qkv_image")
    return img, yb, rstd


def _finish_parts(part: Tensor, n: int, parts: int, lanes: int, defer: bool) -> Tensor:
    """out[n] = the fixed-order sum of ``parts`` partial rows: left to flush_deferred (defer) or one gaot_reduce_multi launch now"""
    out = torch.empty(n, dtype=torch.float32, device=part.device)
    if defer:
        _defer(part, out, n, parts, lanes)
        return out
    arr = (_ReduceDesc * 1)()
    arr[0].part, arr[0].out, arr[0].n, arr[0].parts, arr[0].lanes = part.data_ptr(), out.data_ptr(), n, parts, lanes
    check(_lib.load().gaot_reduce_multi(arr, 1, _stream()), "gaot_reduce_multi")
    return out


def ffn_bwd_norm(yb: Tensor, dy: Tensor, packed: Tensor, f: int, h: Tensor, norm_weight: Tensor, rstd: Tensor, defer: bool = False):
    """ffn_bwd with ffn_norm's backward in its epilogue (include/gaot3d_hip.h: gaot_ffn_bwd_norm) -> (dh fp32 [rows, 256], dag, u, dyb,
    d(norm weight) [256])"""
    lib = _lib.load()
    rows = _req_rows(yb, torch.bfloat16, 256, "ffn_bwd_norm: input")
    _req_rows(dy, torch.float32, 256, "ffn_bwd_norm: gradient", rows=rows)
    _req_rows(h, torch.float32, 256, "ffn_bwd_norm: norm input", dense=False, rows=rows)
    nw = _req(norm_weight, torch.float32, "norm_weight")
    dev = yb.device
    dag = torch.empty(rows, 2 * f, dtype=torch.bfloat16, device=dev)
    u = torch.empty(rows, f, dtype=torch.bfloat16, device=dev)
    dyb = torch.empty(rows, 256, dtype=torch.bfloat16, device=dev)
    dh = torch.empty(rows, 256, dtype=torch.float32, device=dev)
    parts = int(lib.gaot_norm_bwd_parts(rows))
    part = torch.empty(parts, 256, dtype=torch.float32, device=dev)
    with _timed("ffn_bwd_norm"):
        check(lib.gaot_ffn_bwd_norm(_ptr(yb), _ptr(dy), _ptr(packed), _ptr(h), h.stride(0), _ptr(nw), _ptr(rstd), _ptr(dag), _ptr(u), _ptr(dyb),
                                    _ptr(dh), _ptr(part), rows, int(f), _stream()), "gaot_ffn_bwd_norm")
    return dh, dag, u, dyb, _finish_parts(part, 256, parts, 32, defer)


def qkv_bwd_norm(dqkv: Tensor, packed: Tensor, x: Tensor, norm_weight: Tensor, rstd: Tensor, dres: Optional[Tensor] = None,
                 dtap: Optional[Tensor] = None, defer: bool = False):
    """d(norm x) = dqkv Wqkv with attn_norm's backward in its epilogue (include/gaot3d_hip.h: gaot_qkv_bwd_norm; ``packed`` from
    qkv_pack_multi(..., with_backward=True)) -> (dx fp32 [rows, 256], d(norm weight) [256])"""
    lib = _lib.load()
    rows, n = dqkv.shape
    if dqkv.dtype != torch.float32 or not dqkv.is_contiguous() or n % 256:
        raise GaotError("qkv_bwd_norm: contiguous fp32 [rows, N] gradient with N a multiple of 256 expected")
    _req_rows(x, torch.float32, 256, "qkv_bwd_norm: norm input", dense=False, rows=rows)
    nw = _req(norm_weight, torch.float32, "norm_weight")
    dres = None if dres is None else _req(dres, torch.float32, "dres")
    dtap = None if dtap is None else _req(dtap, torch.float32, "dtap")
    dev = dqkv.device
    dx = torch.empty(rows, 256, dtype=torch.float32, device=dev)
    parts = int(lib.gaot_norm_bwd_parts(rows))
    part = torch.empty(parts, 256, dtype=torch.float32, device=dev)
    with _timed("qkv_bwd_norm"):
        check(lib.gaot_qkv_bwd_norm(_ptr(dqkv), n, _ptr(packed), _ptr(x), x.stride(0), _ptr(nw), _ptr(rstd), _ptr(dres), _ptr(dtap), _ptr(dx),
                                    _ptr(part), rows, _stream()), "gaot_qkv_bwd_norm")
    return dx, _finish_parts(part, 256, parts, 32, defer)


def qkv_bwd_norm_cat(dqkv: Tensor, packed: Tensor, x: Tensor, norm_weight: Tensor, rstd: Tensor, dres: Optional[Tensor], skip_packed: Tensor,
                     same: bool, defer: bool = False):
    """qkv_bwd_norm for a decoder block (include/gaot3d_hip.h: gaot_qkv_bwd_norm_cat): also the skip projection's two input gradients
    from the dx rows on chip -> (dx, dxa, dxb or None when ``same`` (dxa then holds the sum), d(norm weight))"""
    lib = _lib.load()
    rows, n = dqkv.shape
    if dqkv.dtype != torch.float32 or not dqkv.is_contiguous() or n % 256:
        raise GaotError("qkv_bwd_norm_cat: contiguous fp32 [rows, N] gradient with N a multiple of 256 expected")
    _req_rows(x, torch.float32, 256, "qkv_bwd_norm_cat: norm input", dense=False, rows=rows)
    if skip_packed.numel() != int(lib.gaot_skip_packed_bytes()):
        raise GaotError("qkv_bwd_norm_cat: skip_packed is not a skip_pack_multi image")
    nw = _req(norm_weight, torch.float32, "norm_weight")
    dres = None if dres is None else _req(dres, torch.float32, "dres")
    dev = dqkv.device
    dx = torch.empty(rows, 256, dtype=torch.float32, device=dev)
    dxa = torch.empty(rows, 256, dtype=torch.float32, device=dev)
    dxb = None if same else torch.empty(rows, 256, dtype=torch.float32, device=dev)
    parts = int(lib.gaot_norm_bwd_parts(rows))
    part = torch.empty(parts, 256, dtype=torch.float32, device=dev)
    with _timed("qkv_bwd_norm_cat"):
        check(lib.gaot_qkv_bwd_norm_cat(_ptr(dqkv), n, _ptr(packed), _ptr(x), x.stride(0), _ptr(nw), _ptr(rstd), _ptr(dres), _ptr(skip_packed),
                                        _ptr(dx), _ptr(dxa), _ptr(dxb), int(bool(same)), _ptr(part), rows, _stream()), "gaot_qkv_bwd_norm_cat")
    return dx, dxa, dxb, _finish_parts(part, 256, parts, 32, defer)


def oproj_bwd_image(dh: Tensor, attn_out: Tensor, packed: Tensor, f: int, b: int, s: int, h: int, hkv: int):
    """d_o = dh Wo as the flash backward's operands (include/gaot3d_hip.h: gaot_oproj_bwd_image): -> (an attn_bwd_scratch buffer whose head
    holds the bf16 dO image, delta fp32 [b, h, s]) for attn_bwd_bf16(do_image=..., delta=...)"""
    lib = _lib.load()
    if h != 8:
        raise GaotError("oproj_bwd_image: 8 heads of 32 expected")
    rows = b * s
    for t, nm in ((dh, "dh"), (attn_out, "attn_out")):
        _req_rows(t, torch.float32, 256, f"oproj_bwd_image: {nm}", rows=rows)
    scratch = attn_bwd_scratch(b, s, h, hkv, dh.device)
    delta = torch.empty(b, h, s, dtype=torch.float32, device=dh.device)
    with _timed("oproj_bwd_image"):
        check(lib.gaot_oproj_bwd_image(_ptr(dh), _ptr(attn_out), _ptr(packed), int(f), _ptr(scratch), _ptr(delta), rows, int(s), _stream()),
              "gaot_oproj_bwd_image")
    return scratch, delta


def norm_ffn_fwd(h: Tensor, norm_weight: Tensor, eps: float, packed: Tensor, f: int):
    """RMSNorm + FFN + residual in one launch (include/gaot3d_hip.h: gaot_norm_ffn_fwd): h fp32 [rows, 256] ->
    (y fp32 [rows, 256] = n + ffn(n), yb = bf16(n) [rows, 256], rstd [rows]) with n = RMSNorm(h)"""
    lib = _lib.load()
    rows = _req_rows(h, torch.float32, 256, "norm_ffn_fwd: input", dense=False)
    nw = _req(norm_weight, torch.float32, "norm_weight")
    y = torch.empty(rows, 256, dtype=torch.float32, device=h.device)
    yb = torch.empty(rows, 256, dtype=torch.bfloat16, device=h.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=h.device)
    with _timed("norm_ffn_fwd"):
        check(lib.gaot_norm_ffn_fwd(_ptr(h), h.stride(0), _ptr(nw), float(eps), _ptr(packed), _ptr(y), _ptr(yb), _ptr(rstd), rows, int(f),
                                    _stream()), "gaot_norm_ffn_fwd")
    return y, yb, rstd


def ffn_bwd_dag(xb: Tensor, dy: Tensor, packed: Tensor, f: int, want_dyb: bool = True):
    """the first half of the FFN backward for a forward that saved nothing (include/gaot3d_hip.h: gaot_ffn_bwd_dag): x [rows, 256] bf16,
    dy fp32 [rows, 256], ``packed`` from ffn_pack(..., with_backward=True) -> (dag bf16 [rows, 2F], u bf16 [rows, F], dyb bf16 or None)"""
    lib = _lib.load()
    rows = _req_rows(xb, torch.bfloat16, 256, "ffn_bwd_dag: input")
    _req_rows(dy, torch.float32, 256, "ffn_bwd_dag: gradient", rows=rows)
    dag = torch.empty(rows, 2 * f, dtype=torch.bfloat16, device=xb.device)
    u = torch.empty(rows, f, dtype=torch.bfloat16, device=xb.device)
    dyb = torch.empty(rows, 256, dtype=torch.bfloat16, device=xb.device) if want_dyb else None
    with _timed("ffn_bwd_dag"):
        check(lib.gaot_ffn_bwd_dag(_ptr(xb), _ptr(dy), _ptr(packed), _ptr(dag), _ptr(u), _ptr(dyb), rows, int(f), _stream()), "gaot_ffn_bwd_dag")
    return dag, u, dyb


def ffn_bwd(xb: Tensor, dy: Tensor, packed: Tensor, f: int, add_dy: bool, want_dyb: bool = True):
    """ffn_bwd_dag with the input gradient in the same launch (include/gaot3d_hip.h: gaot_ffn_bwd) ->
    (dx fp32 [rows, 256] = dag W13 (+ dy), dag, u, dyb)"""
    lib = _lib.load()
    rows = _req_rows(xb, torch.bfloat16, 256, "ffn_bwd: input")
    _req_rows(dy, torch.float32, 256, "ffn_bwd: gradient", rows=rows)
    dag = torch.empty(rows, 2 * f, dtype=torch.bfloat16, device=xb.device)
    u = torch.empty(rows, f, dtype=torch.bfloat16, device=xb.device)
    dyb = torch.empty(rows, 256, dtype=torch.bfloat16, device=xb.device) if want_dyb else None
    dx = torch.empty(rows, 256, dtype=torch.float32, device=xb.device)
    with _timed("ffn_bwd"):
        check(lib.gaot_ffn_bwd(_ptr(xb), _ptr(dy), _ptr(packed), _ptr(dag), _ptr(u), _ptr(dyb), _ptr(dx), int(add_dy), rows, int(f), _stream()),
              "gaot_ffn_bwd")
    return dx, dag, u, dyb


def ffn_w2_bwd_swiglu(dyb: Tensor, w2t: Tensor, ag: Tensor, f: int) -> Tensor:
    """dy [rows, 256] bf16, W2^T [F, 256] bf16, a | g bf16 [rows, 2F] -> d(a) | d(g) bf16 [rows, 2F]: the du = dy W2 product with the
    SwiGLU backward in its epilogue (include/gaot3d_hip.h: gaot_ffn_w2_bwd_swiglu)"""
    lib = _lib.load()
    if any(t.dtype != torch.bfloat16 or not t.is_contiguous() for t in (dyb, w2t, ag)):
        raise GaotError("ffn_w2_bwd_swiglu: contiguous bf16 operands expected")
    dag = torch.empty_like(ag)
    with _timed("ffn_w2_bwd_swiglu"):
        check(lib.gaot_ffn_w2_bwd_swiglu(_ptr(dyb), _ptr(w2t), _ptr(ag), _ptr(dag), dyb.shape[0], dyb.shape[1], w2t.shape[1], int(f),
                                         _stream()), "gaot_ffn_w2_bwd_swiglu")
    return dag


def swiglu_bwd_bf16(ag: Tensor, du: Tensor, f: int) -> Tensor:
    lib = _lib.load()
    dag = torch.empty_like(ag)
    check(lib.gaot_swiglu_bwd_bf16(_ptr(ag), _ptr(du), _ptr(dag), ag.shape[0], f, _stream()), "gaot_swiglu_bwd_bf16")
    return dag


def patchify(src: Tensor, b: int, d: int, h: int, w: int, p: int, c: int, to_tokens: bool) -> Tensor:
    lib = _lib.load()
    dst = torch.empty_like(src)
    check(lib.gaot_patchify(_ptr(src), _ptr(dst), b, d, h, w, p, c, int(to_tokens), _stream()), "gaot_patchify")
    return dst


def mse_fwd(pred: Tensor, target: Tensor) -> Tensor:
    lib = _lib.load()
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    ws = _ws(lib.gaot_mse_workspace_bytes(), pred.device)
    check(lib.gaot_mse_fwd(_ptr(pred), _ptr(target), pred.numel(), _ptr(loss), _ptr(ws), ws.numel(), _stream()),
          "gaot_mse_fwd")
    return loss


def mse_bwd(pred: Tensor, target: Tensor, grad_loss: Tensor) -> Tensor:
    lib = _lib.load()
    dp = torch.empty_like(pred)
    check(lib.gaot_mse_bwd(_ptr(pred), _ptr(target), pred.numel(), _ptr(grad_loss), _ptr(dp), _stream()), "gaot_mse_bwd")
    return dp


def geoembed_stats_sharded_queries(source_pos: Tensor, query_pos: Tensor, g: BipartiteGraph, group, num_queries_total: int) -> Tensor:
    """statistical features when the QUERY rows are spread over the ranks of ``group`` (each rank holds all edges of its
    queries): local raw features (two sweeps per row: centroid, then centred second moments), one fp64 SUM all-reduce of
    the 18 column sums, z-score over all rows.  ``group=None``: no exchange (all rows are local)"""
    import torch.distributed as dist
    lib = _lib.load()
    source_pos = _req(source_pos, torch.float32, "source_pos")
    query_pos = _req(query_pos, torch.float32, "query_pos")
    if source_pos.shape[1] != 3:
        raise GaotError("geoembed statistical features: coord_dim must be 3 on the HIP path")
    q = g.num_dst
    feat = torch.empty(q, 9, dtype=torch.float32, device=query_pos.device)
    sums = torch.empty(18, dtype=torch.float64, device=query_pos.device)
    ws = _ws(lib.gaot_geoembed_stats_workspace_bytes(), query_pos.device)
    check(lib.gaot_geoembed_raw(_ptr(source_pos), _ptr(query_pos), _ptr(g.by_dst.rowptr), _ptr(g.by_dst.other), q, _ptr(feat),
                                _ptr(sums), _ptr(ws), ws.numel(), _stream()), "gaot_geoembed_raw")
    if group is not None:
        from . import comm
        comm.run(lambda: dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=group), (sums,), "all_reduce")
    check(lib.gaot_geoembed_finalize(_ptr(feat), q, _ptr(sums), int(num_queries_total), _ptr(ws), ws.numel(), _stream()),
          "gaot_geoembed_finalize")
    return feat


def geoembed_moments(source_pos: Tensor, query_pos: Tensor, g: BipartiteGraph) -> Tensor:
    """fp64 [Q, 12] additive moments of every query row's neighbourhood (include/gaot3d_hip.h: gaot_geoembed_moments)"""
    lib = _lib.load()
    source_pos = _req(source_pos, torch.float32, "source_pos")
    query_pos = _req(query_pos, torch.float32, "query_pos")
    if source_pos.shape[1] != 3:
        raise GaotError("geoembed statistical features: coord_dim must be 3 on the HIP path")
    mom = torch.empty(g.num_dst, 12, dtype=torch.float64, device=query_pos.device)
    check(lib.gaot_geoembed_moments(_ptr(source_pos), _ptr(query_pos), _ptr(g.by_dst.rowptr), _ptr(g.by_dst.other), g.num_dst,
                                    _ptr(mom), _stream()), "gaot_geoembed_moments")
    return mom


def geoembed_from_moments(mom: Tensor) -> Tensor:
    lib = _lib.load()
    q = mom.shape[0]
    feat = torch.empty(q, 9, dtype=torch.float32, device=mom.device)
    ws = _ws(lib.gaot_geoembed_stats_workspace_bytes(), mom.device)
    check(lib.gaot_geoembed_from_moments(_ptr(mom), q, _ptr(feat), _ptr(ws), ws.numel(), _stream()), "gaot_geoembed_from_moments")
    return feat


def geoembed_from_moments_bwd(mom: Tensor, grad_feat: Tensor) -> Tensor:
    """dL/d features [Q, 9] -> dL/d moments [Q, 12] fp64 (include/gaot3d_hip.h: gaot_geoembed_from_moments_bwd)"""
    lib = _lib.load()
    q = mom.shape[0]
    grad_feat = _req(grad_feat, torch.float32, "grad_features")
    adj = torch.empty(q, 12, dtype=torch.float64, device=mom.device)
    ws = _ws(lib.gaot_geoembed_from_moments_bwd_workspace_bytes(q), mom.device)
    check(lib.gaot_geoembed_from_moments_bwd(_ptr(mom), _ptr(grad_feat), q, _ptr(adj), _ptr(ws), ws.numel(), _stream()),
          "gaot_geoembed_from_moments_bwd")
    return adj


def geoembed_moments_bwd(source_pos: Tensor, query_pos: Tensor, g: BipartiteGraph, adj: Tensor):
    """dL/d moments -> (dL/du per edge [E, 3] in the by-query edge order, dL/d query_pos [Q, 3])"""
    lib = _lib.load()
    source_pos = _req(source_pos, torch.float32, "source_pos")
    query_pos = _req(query_pos, torch.float32, "query_pos")
    ge = torch.empty(g.by_dst.num_edges, 3, dtype=torch.float32, device=query_pos.device)
    gq = torch.empty(g.num_dst, 3, dtype=torch.float32, device=query_pos.device)
    check(lib.gaot_geoembed_moments_bwd(_ptr(source_pos), _ptr(query_pos), _ptr(g.by_dst.rowptr), _ptr(g.by_dst.other),
                                        g.num_dst, _ptr(adj), _ptr(ge), _ptr(gq), _stream()), "gaot_geoembed_moments_bwd")
    return ge, gq


def _ptr_array(ts):
    arr = (C.c_void_p * len(ts))()
    for i, t in enumerate(ts):
        arr[i] = _ptr(t).value
    return arr


def scale_mix_fwd(xs, logits: Tensor):
    lib = _lib.load()
    n, c = xs[0].shape
    out = torch.empty_like(xs[0])
    w = torch.empty(n, len(xs), dtype=torch.float32, device=out.device)
    check(lib.gaot_scale_mix_fwd(_ptr_array(xs), len(xs), _ptr(logits), _ptr(out), _ptr(w), n, c, _stream()),
          "gaot_scale_mix_fwd")
    return out, w


def scale_mix_bwd(xs, w: Tensor, dout: Tensor):
    lib = _lib.load()
    n, c = xs[0].shape
    dxs = [torch.empty_like(x) for x in xs]
    dlog = torch.empty_like(w)
    check(lib.gaot_scale_mix_bwd(_ptr_array(xs), len(xs), _ptr(w), _ptr(dout), _ptr_array(dxs), _ptr(dlog), n, c,
                                 _stream()), "gaot_scale_mix_bwd")
    return dxs, dlog


def mlp2_forward(x: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Optional[Tensor]) -> Tensor:
    """out = w2 gelu(w1 x + b1) + b2, x [rows, 32] (include/gaot3d_hip.h: gaot_mlp2_fwd)"""
    lib = _lib.load()
    rows, hid, oc = x.shape[0], w1.shape[0], w2.shape[0]
    out = torch.empty(rows, oc, dtype=torch.float32, device=x.device)
    check(lib.gaot_mlp2_fwd(_ptr(x), rows, x.shape[1], hid, oc, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(out), _stream()),
          "gaot_mlp2_fwd")
    return out


def mlp2_jvp_supported(in_dim: int, hidden: int, out_dim: int, num_tangents: int, act: int) -> bool:
    return bool(_lib.load().gaot_mlp2_jvp_supported(int(in_dim), int(hidden), int(out_dim), int(num_tangents), int(act)))


def mlp2_jvp(x: Tensor, dxs: Sequence[Tensor], w1: Tensor, b1: Tensor, w2: Tensor, b2: Optional[Tensor], y: Optional[Tensor] = None,
             jac: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """-> (y [rows, out], jac [rows, out, T]): y = w2 gelu(w1 x + b1) + b2 and jac[:, :, d] its tangent along dxs[d], exact fp32 in
    one launch (include/gaot3d_hip.h: gaot_mlp2_jvp).  x and the T <= 3 planes dense fp32 [rows, 32]; ``y`` / ``jac`` name the
    destinations (fp32 views with any positive strides, y with unit column stride), else both are allocated"""
    lib = _lib.load()
    rows, hid, oc, t = _req_rows(x, torch.float32, 32, "mlp2_jvp: x"), int(w1.shape[0]), int(w2.shape[0]), len(dxs)
    if t > 3:
        raise GaotError(f"mlp2_jvp: at most 3 tangent planes, got {t}")
    for d in dxs:
        _req_rows(d, torch.float32, 32, "mlp2_jvp: tangent plane", rows=rows)
    for name, w, shape in (("w1", w1, (hid, 32)), ("b1", b1, (hid,)), ("w2", w2, (oc, hid))) + ((("b2", b2, (oc,)),) if b2 is not None else ()):
        if w.dtype != torch.float32 or tuple(w.shape) != shape or not w.is_contiguous():
            raise GaotError(f"mlp2_jvp: {name}: contiguous float32 {shape} expected, got {w.dtype} {tuple(w.shape)}")
    if y is None:
        y = torch.empty(rows, oc, dtype=torch.float32, device=x.device)
    if jac is None:
        jac = torch.empty(rows, oc, t, dtype=torch.float32, device=x.device)
    _req_rows(y, torch.float32, oc, "mlp2_jvp: y", dense=False, rows=rows)
    if jac.dtype != torch.float32 or tuple(jac.shape) != (rows, oc, t) or not jac.is_cuda:
        raise GaotError(f"mlp2_jvp: jac: float32 [{rows}, {oc}, {t}] on the GPU expected, got {jac.dtype} {tuple(jac.shape)} on {jac.device}")
    # the stride of a dimension of extent <= 1 is never used (torch reports anything there); the library checks the others
    ldy = int(y.stride(0)) if rows > 1 else oc
    js = [int(s) if n > 1 else 1 for s, n in zip(jac.stride(), jac.shape)]
    p = [_ptr(d) for d in dxs] + [None] * (3 - t)
    with _timed(f"mlp2_jvp_h{hid}_t{t}"):
        check(lib.gaot_mlp2_jvp(_ptr(x), p[0], p[1], p[2], t, rows, 32, hid, oc, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(y), ldy,
                                _ptr(jac) if t else None, js[0], js[1], js[2], _stream()), "gaot_mlp2_jvp")
    return y, jac


def mlp2_jet2_supported(in_dim: int, hidden: int, out_dim: int, nd: int, act: int) -> bool:
    return bool(_lib.load().gaot_mlp2_jet2_supported(int(in_dim), int(hidden), int(out_dim), int(nd), int(act)))


def mlp2_jet2(x: Tensor, dxs: Sequence[Tensor], ddxs: Sequence[Tensor], w1: Tensor, b1: Tensor, w2: Tensor, b2: Optional[Tensor],
              y: Optional[Tensor] = None, d1: Optional[Tensor] = None, d2: Optional[Tensor] = None, store_y: bool = True):
    """-> (y [rows, out], d1 [rows, out, nd], d2 [rows, out, nd]): y = w2 gelu(w1 x + b1) + b2 with its first and second directional
    derivative along nd = 1..3 directions, given per direction the first-order plane dxs[d] and the second-order plane ddxs[d] of x
    (dense fp32 [rows, 32]): d1 = w2 (gelu' * w1 dx), d2 = w2 (gelu'' * (w1 dx)^2 + gelu' * w1 ddx).  Exact fp32 in one launch
    (include/gaot3d_hip.h: gaot_mlp2_jet2); y and d1 are ``mlp2_jvp``'s bit for bit.  ``y`` / ``d1`` / ``d2`` name the destinations
    (fp32 views with positive strides, d1 and d2 with the SAME strides), else they are allocated; ``store_y=False`` skips the value
    (y is returned as None)."""
    lib = _lib.load()
    rows, hid, oc, t = _req_rows(x, torch.float32, 32, "mlp2_jet2: x"), int(w1.shape[0]), int(w2.shape[0]), len(dxs)
    if not 1 <= t <= 3 or len(ddxs) != t:
        raise GaotError(f"mlp2_jet2: 1..3 directions with one dx and one ddx plane each, got {t} and {len(ddxs)}")
    for d in list(dxs) + list(ddxs):
        _req_rows(d, torch.float32, 32, "mlp2_jet2: direction plane", rows=rows)
    for name, w, shape in (("w1", w1, (hid, 32)), ("b1", b1, (hid,)), ("w2", w2, (oc, hid))) + ((("b2", b2, (oc,)),) if b2 is not None else ()):
        if w.dtype != torch.float32 or tuple(w.shape) != shape or not w.is_contiguous():
            raise GaotError(f"mlp2_jet2: {name}: contiguous float32 {shape} expected, got {w.dtype} {tuple(w.shape)}")
    if not store_y:
        y = None
    elif y is None:
        y = torch.empty(rows, oc, dtype=torch.float32, device=x.device)
    if d1 is None:
        d1 = torch.empty(rows, oc, t, dtype=torch.float32, device=x.device)
    if d2 is None:
        d2 = torch.empty(rows, oc, t, dtype=torch.float32, device=x.device)
    ldy = oc
    if y is not None:
        _req_rows(y, torch.float32, oc, "mlp2_jet2: y", dense=False, rows=rows)
        ldy = int(y.stride(0)) if rows > 1 else oc
    for name, j in (("d1", d1), ("d2", d2)):
        if j.dtype != torch.float32 or tuple(j.shape) != (rows, oc, t) or not j.is_cuda:
            raise GaotError(f"mlp2_jet2: {name}: float32 [{rows}, {oc}, {t}] on the GPU expected, got {j.dtype} {tuple(j.shape)} on {j.device}")
    # the stride of a dimension of extent <= 1 is never used (torch reports anything there); the library checks the others
    js = [int(s) if n > 1 else 1 for s, n in zip(d1.stride(), d1.shape)]
    if js != [int(s) if n > 1 else 1 for s, n in zip(d2.stride(), d2.shape)]:
        raise GaotError(f"mlp2_jet2: d1 and d2 must have the same strides, got {d1.stride()} and {d2.stride()}")
    p = [_ptr(d) for d in dxs] + [None] * (3 - t)
    pp = [_ptr(d) for d in ddxs] + [None] * (3 - t)
    with _timed(f"mlp2_jet2_h{hid}_d{t}"):
        check(lib.gaot_mlp2_jet2(_ptr(x), p[0], p[1], p[2], pp[0], pp[1], pp[2], t, rows, 32, hid, oc, _ptr(w1), _ptr(b1), _ptr(w2),
                                 _ptr(b2), _ptr(y) if y is not None else None, ldy, _ptr(d1), _ptr(d2), js[0], js[1], js[2], _stream()),
              "gaot_mlp2_jet2")
    return y, d1, d2


def mlp2_lap_cot_mid(zus: Tensor, a: Optional[Tensor], ad: Tensor, al: Tensor, b1: Optional[Tensor] = None,
                     out: Optional[Tensor] = None) -> Tensor:
    """The elementwise middle of the cotangent of the two-layer MLP's LAPLACIAN jet in one launch (include/gaot3d_hip.h:
    gaot_mlp2_lap_cot_mid).  ``zus`` [5, rows, hidden]: the stack [z - b1; u_0; u_1; u_2; s] one product with W1 gives (``b1``
    [hidden] or None is added to z here); ``a`` [rows, hidden] or None (no cotangent on the value), ``ad`` [3, rows, hidden], ``al``
    [rows, hidden]: the cotangents of y, y'_d and Lap y pulled to hidden width -> ``out`` [5, rows, hidden] = [dz; du_0; du_1; du_2; ds]
    (erf-GELU: a', a'', a''' from one phi and one Phi per element).  ``out`` may be the storage of the stack [a; ad; al] or ``zus`` itself.
    Everything float32, contiguous, on one device; hidden a multiple of 4.  Bad operands raise GaotError before the launch."""
    lib = _lib.load()
    fn = "mlp2_lap_cot_mid"
    if not isinstance(zus, Tensor) or zus.dim() != 3 or zus.shape[0] != 5:
        raise GaotError(f"{fn}: zus must be [5, rows, hidden], got {tuple(zus.shape) if isinstance(zus, Tensor) else type(zus).__name__}")
    rows, hid = int(zus.shape[1]), int(zus.shape[2])
    if hid < 4 or hid % 4:
        raise GaotError(f"{fn}: hidden must be a positive multiple of 4, got {hid}")
    if out is None:
        out = torch.empty_like(zus)
    for name, t, shape, optional in (("zus", zus, (5, rows, hid), False), ("a", a, (rows, hid), True), ("ad", ad, (3, rows, hid), False),
                                     ("al", al, (rows, hid), False), ("b1", b1, (hid,), True), ("out", out, (5, rows, hid), False)):
        if t is None and optional:
            continue
        if not isinstance(t, Tensor) or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() \
                or t.device != zus.device or t.data_ptr() % 16:
            got = f"{t.dtype} {tuple(t.shape)} on {t.device}, strides {tuple(t.stride())}" if isinstance(t, Tensor) else type(t).__name__
            raise GaotError(f"{fn}: {name} must be contiguous, 16-byte aligned float32 {list(shape)} on {zus.device}, got {got}")
    n = rows * hid
    with _timed(f"mlp2_lap_cot_mid_h{hid}"):
        check(lib.gaot_mlp2_lap_cot_mid(_ptr(zus[0]), _ptr(zus[1]), n, _ptr(zus[4]), _ptr(b1), _ptr(a), _ptr(ad), n, _ptr(al), rows, hid,
                                        _ptr(out), n, _stream()), "gaot_mlp2_lap_cot_mid")
    return out


def mlp2_jet2_cot_mid(zus: Tensor, a: Optional[Tensor], ab: Tensor, b1: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """``mlp2_lap_cot_mid`` with a second-order cotangent PER DIRECTION, one launch for nd = 1..6 (include/gaot3d_hip.h:
    gaot_mlp2_jet2_cot_mid).  ``zus`` [1 + 2 nd, rows, hidden]: the stack [z - b1; u_0..; s_0..] one product with W1 gives (``b1``
    [hidden] or None is added to z here); ``a`` [rows, hidden] or None (no cotangent on the value); ``ab`` [2 nd, rows, hidden]: the
    cotangents of y'_i, then of y''_i, pulled to hidden width -> ``out`` [1 + 2 nd, rows, hidden] = [dz; du_0..; ds_0..] (erf-GELU).
    ``out`` may be the storage of the stack [a; ab] or ``zus`` itself.  Everything float32, contiguous, on one device; hidden a
    multiple of 4.  Bad operands raise GaotError before the launch."""
    lib = _lib.load()
    fn = "mlp2_jet2_cot_mid"
    if not isinstance(zus, Tensor) or zus.dim() != 3 or zus.shape[0] % 2 != 1 or not 1 <= zus.shape[0] // 2 <= 6:
        raise GaotError(f"{fn}: zus must be [1 + 2 nd, rows, hidden] with nd in 1..6, got "
                        f"{tuple(zus.shape) if isinstance(zus, Tensor) else type(zus).__name__}")
    nd, rows, hid = int(zus.shape[0]) // 2, int(zus.shape[1]), int(zus.shape[2])
    if hid < 4 or hid % 4:
        raise GaotError(f"{fn}: hidden must be a positive multiple of 4, got {hid}")
    if out is None:
        out = torch.empty_like(zus)
    for name, t, shape, optional in (("zus", zus, (1 + 2 * nd, rows, hid), False), ("a", a, (rows, hid), True),
                                     ("ab", ab, (2 * nd, rows, hid), False), ("b1", b1, (hid,), True),
                                     ("out", out, (1 + 2 * nd, rows, hid), False)):
        if t is None and optional:
            continue
        if not isinstance(t, Tensor) or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() \
                or t.device != zus.device or t.data_ptr() % 16:
            got = f"{t.dtype} {tuple(t.shape)} on {t.device}, strides {tuple(t.stride())}" if isinstance(t, Tensor) else type(t).__name__
            raise GaotError(f"{fn}: {name} must be contiguous, 16-byte aligned float32 {list(shape)} on {zus.device}, got {got}")
    n = rows * hid
    with _timed(f"mlp2_jet2_cot_mid_h{hid}_d{nd}"):
        check(lib.gaot_mlp2_jet2_cot_mid(_ptr(zus), n, _ptr(b1), _ptr(a), _ptr(ab), n, nd, rows, hid, _ptr(out), n, _stream()),
              "gaot_mlp2_jet2_cot_mid")
    return out


def _finish_tables(ws: Tensor, outs, parts, lanes, defer: bool) -> None:
    """the fixed-order sums of the [parts][n] partial tables that lie one behind the other in ``ws`` (fp32) into ``outs``: left
    to flush_deferred (defer) or ONE gaot_reduce_multi launch now -- the same kernel, the same order, the same bits.  ``parts`` /
    ``lanes``: one int for all tables or one per table"""
    tab = ws.view(torch.float32)
    arr = (_ReduceDesc * len(outs))()
    parts_of = [parts] * len(outs) if isinstance(parts, int) else list(parts)
    lanes_of = [lanes] * len(outs) if isinstance(lanes, int) else list(lanes)
    off = 0
    for j, out in enumerate(outs):
        n, parts, lanes = out.numel(), parts_of[j], lanes_of[j]
        if defer:
            _defer(tab[off:off + parts * n], out, n, parts, lanes)
        else:
            arr[j].part, arr[j].out, arr[j].n, arr[j].parts, arr[j].lanes = tab.data_ptr() + 4 * off, out.data_ptr(), n, parts, lanes
        off += parts * n
    if not defer:
        check(_lib.load().gaot_reduce_multi(arr, len(outs), _stream()), "gaot_reduce_multi")


def mlp2_backward(x: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, dout: Tensor, defer: bool = False):
    """-> (dx, dw1, db1, dw2); the three weight gradients are completed by one launch, or (``defer``, see defer_ok) by
    flush_deferred"""
    lib = _lib.load()
    rows, hid, oc = x.shape[0], w1.shape[0], w2.shape[0]
    dx = torch.empty_like(x)
    dw1, db1, dw2 = torch.empty_like(w1), torch.empty_like(b1), torch.empty_like(w2)
    ws = _ws(lib.gaot_mlp2_bwd_workspace_bytes(hid, oc), x.device)
    check(lib.gaot_mlp2_bwd(_ptr(x), rows, x.shape[1], hid, oc, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(dout), _ptr(dx), None, None, None,
                            _ptr(ws), ws.numel(), _stream()), "gaot_mlp2_bwd")
    _finish_tables(ws, (dw1, db1, dw2), int(lib.gaot_mlp2_bwd_parts(rows)), 4, defer)
    return dx, dw1, db1, dw2


def mlp2_bwd_f32_supported(in_dim: int, hidden: int, out_dim: int, act: int) -> bool:
    return bool(_lib.load().gaot_mlp2_bwd_f32_supported(int(in_dim), int(hidden), int(out_dim), int(act)))


def mlp2_backward_f32(x: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, dout: Tensor):
    """-> (dx, dw1, db1, dw2) of out = w2 gelu(w1 x + b1) + b2 in exact fp32, ONE launch plus the fixed-order completion of the
    weight-gradient partials (include/gaot3d_hip.h: gaot_mlp2_bwd_f32): x dense fp32 [rows, 32], dout dense fp32 [rows, out], hidden
    in {64, 128, 256}, out in 1..4; d_b2 is ``colsum(dout)``.  Every operand is checked BEFORE a launch; a shape outside the family
    raises GaotError (``mlp2_bwd_f32_supported``).  rows == 0 launches nothing and gives zeros."""
    fn = "mlp2_backward_f32"
    for name, t in (("x", x), ("w1", w1), ("b1", b1), ("w2", w2), ("dout", dout)):
        if not isinstance(t, Tensor) or t.dtype != torch.float32 or not t.is_contiguous():
            raise GaotError(f"{fn}: {name}: a contiguous float32 tensor expected, got "
                            f"{(t.dtype, tuple(t.shape)) if isinstance(t, Tensor) else type(t).__name__}")
    if x.dim() != 2 or w1.dim() != 2 or w2.dim() != 2 or b1.dim() != 1 or dout.dim() != 2:
        raise GaotError(f"{fn}: x [rows, 32], w1 [hidden, 32], b1 [hidden], w2 [out, hidden], dout [rows, out] expected, got "
                        f"{tuple(x.shape)}, {tuple(w1.shape)}, {tuple(b1.shape)}, {tuple(w2.shape)}, {tuple(dout.shape)}")
    rows, hid, oc = int(x.shape[0]), int(w1.shape[0]), int(w2.shape[0])
    if tuple(w1.shape) != (hid, x.shape[1]) or tuple(b1.shape) != (hid,) or tuple(w2.shape) != (oc, hid) or tuple(dout.shape) != (rows, oc):
        raise GaotError(f"{fn}: shapes do not fit: x {tuple(x.shape)}, w1 {tuple(w1.shape)}, b1 {tuple(b1.shape)}, w2 {tuple(w2.shape)}, "
                        f"dout {tuple(dout.shape)}")
    lib = _lib.load()
    if not lib.gaot_mlp2_bwd_f32_supported(int(x.shape[1]), hid, oc, 1):
        raise GaotError(f"{fn}: supported shapes are in = 32, hidden in {{64, 128, 256}}, out in 1..4 (got {x.shape[1]} -> {hid} -> {oc})")
    for name, t in (("x", x), ("w1", w1), ("b1", b1), ("w2", w2), ("dout", dout)):
        if not t.is_cuda:
            raise GaotError(f"{fn}: {name}: expected a tensor on the GPU (the HIP path has no CPU fallback), got {t.device}")
    if rows == 0:
        return torch.zeros_like(x), torch.zeros_like(w1), torch.zeros_like(b1), torch.zeros_like(w2)
    if x.data_ptr() % 16:
        raise GaotError(f"{fn}: x must be 16-byte aligned")
    dx = torch.empty_like(x)
    dw1, db1, dw2 = torch.empty_like(w1), torch.empty_like(b1), torch.empty_like(w2)
    ws = _ws(lib.gaot_mlp2_bwd_f32_workspace_bytes(hid, oc), x.device)
    with _timed(f"mlp2_bwd_f32_h{hid}"):
        check(lib.gaot_mlp2_bwd_f32(_ptr(x), rows, 32, hid, oc, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(dout), _ptr(dx), None, None, None,
                                    _ptr(ws), ws.numel(), _stream()), "gaot_mlp2_bwd_f32")
        _finish_tables(ws, (dw1, db1, dw2), int(lib.gaot_mlp2_bwd_f32_parts(rows)), 4, False)
    return dx, dw1, db1, dw2


def _pointnet_args(source_pos: Tensor, query_pos: Tensor, g: BipartiteGraph, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, mode: int):
    source_pos = _req(source_pos, torch.float32, "source_pos")
    query_pos = _req(query_pos, torch.float32, "query_pos")
    w1, b1, w2, b2 = (_req(t, torch.float32, n) for t, n in ((w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2")))
    d = int(query_pos.shape[1]) if query_pos.dim() == 2 else 0
    if source_pos.dim() != 2 or source_pos.shape[1] != d or query_pos.shape[0] != g.num_dst or source_pos.shape[0] != g.num_src:
        raise GaotError(f"pointnet: source_pos [{g.num_src}, D] and query_pos [{g.num_dst}, D] expected, got "
                        f"{tuple(source_pos.shape)} and {tuple(query_pos.shape)}")
    if tuple(w1.shape) != (32, d) or tuple(b1.shape) != (32,) or tuple(w2.shape) != (32, 32) or tuple(b2.shape) != (32,):
        raise GaotError(f"pointnet: the MLP must be Linear({d}, 32) / Linear(32, 32), got weights {tuple(w1.shape)}, {tuple(w2.shape)}")
    if mode not in (1, 2):
        raise GaotError(f"pointnet: mode must be 1 (mean) or 2 (max), got {mode}")
    s = g.by_dst
    head = (_ptr(source_pos), _ptr(query_pos), d, _ptr(s.rowptr), _ptr(s.other), _ptr(s.key), g.num_dst, s.num_edges,
            _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), mode)
    return head, d, (source_pos, query_pos, w1, b1, w2, b2)


def pointnet_fwd(source_pos: Tensor, query_pos: Tensor, g: BipartiteGraph, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor,
                 mode: int):
    """PointNet GeometricEmbedding up to the pooling, fused (include/gaot3d_hip.h: gaot_pointnet_fwd): -> (pooled [Q, 32],
    argmax int32 [Q, 32] for max pooling, else None).  ``mode``: edgeops.MEAN (1) or edgeops.MAX (2)"""
    head, _, keep = _pointnet_args(source_pos, query_pos, g, w1, b1, w2, b2, mode)
    dev = keep[1].device
    pooled = torch.empty(g.num_dst, 32, dtype=torch.float32, device=dev)
    arg = torch.empty(g.num_dst, 32, dtype=torch.int32, device=dev) if mode == 2 else None
    with _timed("pointnet_fwd"):
        check(_lib.load().gaot_pointnet_fwd(*head, _ptr(pooled), _ptr(arg), _stream()), "gaot_pointnet_fwd")
    return pooled, arg


def pointnet_bwd(source_pos: Tensor, query_pos: Tensor, g: BipartiteGraph, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor,
                 mode: int, d_pooled: Tensor, argmax: Optional[Tensor], want_source: bool = False, want_query: bool = False):
    """-> (dw1 [32, D], db1, dw2, db2 (views of one flat gradient), d_source or None, d_query or None): the hidden layers are
    recomputed per edge (gaot_pointnet_bwd); the per-edge W1^T dz1 rows are written only for ``want_source`` and summed by
    source here with the fixed-order segmented sum, as EdgeOffsetFn does"""
    lib = _lib.load()
    head, d, keep = _pointnet_args(source_pos, query_pos, g, w1, b1, w2, b2, mode)
    dev = keep[1].device
    d_pooled = _req(d_pooled, torch.float32, "d_pooled")
    if tuple(d_pooled.shape) != (g.num_dst, 32) or (mode == 2 and (argmax is None or tuple(argmax.shape) != (g.num_dst, 32))):
        raise GaotError("pointnet_bwd: d_pooled (and argmax for max pooling) must be [num_queries, 32]")
    e = g.by_dst.num_edges
    n = 32 * d + 1088
    flat = torch.empty(n, dtype=torch.float32, device=dev)
    dq = torch.empty(g.num_dst, d, dtype=torch.float32, device=dev) if want_query else None
    de = torch.empty(e, d, dtype=torch.float32, device=dev) if want_source else None
    ws = _ws(4 * n * int(lib.gaot_pointnet_bwd_parts(e)), dev)
    with _timed("pointnet_bwd"):
        check(lib.gaot_pointnet_bwd(*head, _ptr(d_pooled), _ptr(argmax if mode == 2 else None), _ptr(flat), _ptr(dq), _ptr(de),
                                    _ptr(ws), ws.numel(), _stream()), "gaot_pointnet_bwd")
    ds = None
    if want_source:
        from . import edgeops as EO
        if e == 0:
            ds = torch.zeros(g.num_src, d, dtype=torch.float32, device=dev)
        else:
            ds = EO.segment_reduce(de, g.by_src.rowptr, EO.src_to_dst_map(g), g.num_src, EO.SUM, channels=d)
    o1, o2 = 32 * d, 32 * d + 32
    return flat[:o1].view(32, d), flat[o1:o2], flat[o2:o2 + 1024].view(32, 32), flat[o2 + 1024:], ds, dq


# single-pass thin fp32 linears (csrc/rowlinear.hip).  ROWLIN counts the calls that took them (tests assert the route)
ROWLIN = {"enabled": True, "fwd": 0, "bwd": 0}


def rowlin_ok(xs: Sequence[Tensor], w: Tensor, bias: Optional[Tensor], act: int, precision: Optional[int]) -> bool:
    """may y = act([xs] w^T + bias) run on the single-pass kernels?  fp32 mode, dense fp32 operands on the GPU, act none / ReLU,
    a shape inside gaot_rowlin_supported, and no side stream for the weight gradients (comm.set_side_stream)"""
    from . import comm
    prec = _PRECISION["mode"] if precision is None else precision
    if not ROWLIN["enabled"] or prec != 0 or act not in (0, 2) or comm.side_stream() is not None or not 1 <= len(xs) <= 4:
        return False
    m = xs[0].shape[0]
    for t in (*xs, w) + (() if bias is None else (bias,)):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            return False
    if any(x.dim() != 2 or x.shape[0] != m for x in xs) or w.dim() != 2 or w.shape[1] != sum(x.shape[1] for x in xs):
        return False
    ks = (C.c_int * len(xs))(*[int(x.shape[1]) for x in xs])
    return bool(_lib.load().gaot_rowlin_supported(ks, len(xs), int(w.shape[0])))


def rowlin_forward(xs: Sequence[Tensor], w: Tensor, bias: Optional[Tensor], relu: bool) -> Tensor:
    """y [M, N] = act([x_0 | x_1 | ...] w^T + bias) in one launch (include/gaot3d_hip.h: gaot_rowlin_fwd)"""
    lib = _lib.load()
    m, n = xs[0].shape[0], w.shape[0]
    y = torch.empty(m, n, dtype=torch.float32, device=w.device)
    ks = (C.c_int * len(xs))(*[int(x.shape[1]) for x in xs])
    check(lib.gaot_rowlin_fwd(_ptr_array(xs), ks, len(xs), _ptr(w), _ptr(bias), m, n, int(relu), _ptr(y), _stream()), "gaot_rowlin_fwd")
    ROWLIN["fwd"] += 1
    return y


def rowlin_backward(xs: Sequence[Tensor], w: Tensor, dy: Tensor, y: Optional[Tensor], relu: bool, need_dx: Sequence[bool],
                    defer: bool = False, want_w: bool = True, want_b: bool = True):
    """-> ([dx_i or None], dw [N, Ktot] or None, db [N] or None) from one walk over the rows of dy (and of the saved output ``y``
    with ReLU); the wanted ones of dw and db are completed by one launch, or (``defer``, see defer_ok) by flush_deferred -- the
    same sums either way; the partial rows of an unwanted one are simply dropped"""
    lib = _lib.load()
    m, n, dev = xs[0].shape[0], w.shape[0], w.device
    dxs = [torch.empty_like(x) if need else None for x, need in zip(xs, need_dx)]
    ROWLIN["bwd"] += 1
    if m == 0:
        return (dxs, torch.zeros_like(w) if want_w else None,
                torch.zeros(n, dtype=torch.float32, device=dev) if want_b else None)
    dw = torch.empty_like(w) if want_w else None
    db = torch.empty(n, dtype=torch.float32, device=dev) if want_b else None
    wp, wl, bp = C.c_int(0), C.c_int(0), C.c_int(0)
    check(lib.gaot_rowlin_plan(m, n, C.byref(wp), C.byref(wl), C.byref(bp)), "gaot_rowlin_plan")
    ws = _ws(4 * (wp.value * w.numel() + bp.value * n), dev)
    tab = ws.view(torch.float32)
    ks = (C.c_int * len(xs))(*[int(x.shape[1]) for x in xs])
    check(lib.gaot_rowlin_bwd(_ptr_array(xs), ks, len(xs), _ptr(w), _ptr(dy), _ptr(y) if relu else None, m, n, int(relu), _ptr_array(dxs),
                              _ptr(tab), C.c_void_p(tab.data_ptr() + 4 * wp.value * w.numel()), _stream()), "gaot_rowlin_bwd")
    if want_w:
        _finish_tables(ws, (dw,) + ((db,) if want_b else ()), (wp.value, bp.value), (wl.value, 32), defer)
    elif want_b:
        _finish_tables(ws[4 * wp.value * w.numel():], (db,), bp.value, 32, defer)
    return dxs, dw, db


def launch_count_reset() -> None:
    _lib.load().gaot_launch_count(1)


def launch_count() -> int:
    """kernel launches issued by the library since the last reset (ATen launches -- fills, cats, index plumbing -- excluded)"""
    return int(_lib.load().gaot_launch_count(0))
