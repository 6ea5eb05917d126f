"""TEST INFRASTRUCTURE -- an exact reference for the neighbour search on a DYADIC LATTICE.

Every token and query coordinate is an integer divided by ``SCALE`` = 8 with magnitude at most 2.  On this lattice every
fp32 difference (|a - b| <= 32 / 8), square (<= 1024 / 64) and three-term sum in the kernels' ``dist2`` is exactly
representable, with or without fused multiply-add contraction, so the distances the device compares ARE the true
distances: a true tie is a device tie and nothing else is.  The reference therefore works on the integers alone
(int64 torch on the CPU) and can arbitrate ties, which ``oracle/graph_oracle.py`` (cdist in floating point) cannot.

Definitions restated (csrc/graph.hip header, gaot_3d_amd/graph.py):
  * knn     : the k tokens of a query with the smallest (distance, token index)
  * radius  : the tokens with d <= r of a centre, ascending index, the first ``cap``
  * encoder 'radius': centres are the TOKENS (<= cap points per token), rows [point, token], grouped by token
  * decoder 'radius': centres are the POINTS (<= cap tokens per point), rows [token, point], grouped by point
  * 'bidirectional' = coalesce(cat(knn, radius)): sorted by (row 0, row 1), duplicates dropped
  * 'reverse' = flip of the bidirectional ENCODER graph
  * the per-query union (graph.query_lists): the decoder graph's rows by query, tokens ascending
Radii are given as the INTEGER ``r2_int`` = (SCALE * r)^2, compared with the integer squared distance.

Imports nothing from the package under test and nothing from oracle/."""
import itertools

import torch

SCALE = 8
LIMIT = 2 * SCALE          # |integer coordinate| <= 16  <->  |coordinate| <= 2
CAP = 32                   # PyG's default max_num_neighbors (what the product calls RADIUS_CAP)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def to_float(ints):
    """integer lattice coordinates -> the fp32 coordinates the device sees (exact: small integers / 8)"""
    assert int(ints.abs().max()) <= LIMIT if ints.numel() else True
    return ints.to(torch.float32) / SCALE


def grid_ints(dims, lo, step):
    """[D*H*W, 3] int64 lattice coordinates of the row-major (indexing='ij') grid with integer origin ``lo`` and steps ``step``"""
    axes = [lo[a] + step[a] * torch.arange(dims[a], dtype=torch.int64) for a in range(3)]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3)


def grid_box(dims, lo, step):
    """(lo, hi) of that grid as floats -- the arguments ``data.latent_grid`` / ``torch.linspace`` take"""
    return (tuple(lo[a] / SCALE for a in range(3)), tuple((lo[a] + step[a] * (dims[a] - 1)) / SCALE for a in range(3)))


def refined_queries(dims, lo, step):
    """every point of the half-step lattice of the box: all grid nodes, edge midpoints, face centres and cell centres.
    -> (int64 [N, 3], int64 [N] = number of half-step coordinates: 0 node, 1 edge midpoint, 2 face centre, 3 cell centre).
    Needs even steps on every axis with more than one node."""
    axes, odd = [], []
    for a in range(3):
        if dims[a] == 1:
            axes.append(torch.tensor([lo[a]], dtype=torch.int64))
            odd.append(torch.zeros(1, dtype=torch.int64))
        else:
            assert step[a] % 2 == 0, "half steps must stay on the lattice"
            n = 2 * dims[a] - 1
            axes.append(lo[a] + (step[a] // 2) * torch.arange(n, dtype=torch.int64))
            odd.append(torch.arange(n, dtype=torch.int64) % 2)
    q = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3)
    kind = torch.stack(torch.meshgrid(*odd, indexing="ij"), dim=-1).reshape(-1, 3).sum(1)
    return q, kind


def outside_queries(dims, lo, step, cells=(1, 3, 12)):
    """points ``cells`` cells outside the box on each side of each axis (the other coordinates on a node, a midpoint where the
    step is even, and the far corner), as far as |coordinate| <= 2 allows; at least one 12-cell point per side is asserted by
    the caller through ``max_cells_outside``"""
    hi = [lo[a] + step[a] * (dims[a] - 1) for a in range(3)]
    out = []
    for a, c, side in itertools.product(range(3), cells, (-1, 1)):
        if dims[a] == 1:
            continue
        v = lo[a] - c * step[a] if side < 0 else hi[a] + c * step[a]
        if abs(v) > LIMIT:
            continue
        for other in range(3):
            p = [0, 0, 0]
            for b in range(3):
                if b == a:
                    p[b] = v
                elif other == 0:
                    p[b] = lo[b]
                elif other == 1:
                    p[b] = lo[b] + (step[b] // 2 if dims[b] > 1 and step[b] % 2 == 0 else 0) + step[b] * ((dims[b] - 1) // 2)
                else:
                    p[b] = hi[b]
            out.append(p)
    # all three coordinates outside at once (a corner direction)
    for c, side in itertools.product(cells, (-1, 1)):
        p = [(lo[a] - c * step[a] if side < 0 else hi[a] + c * step[a]) if dims[a] > 1 else lo[a] for a in range(3)]
        if max(abs(v) for v in p) <= LIMIT:
            out.append(p)
    return torch.tensor(out, dtype=torch.int64).reshape(-1, 3)


def max_cells_outside(q, dims, lo, step):
    """largest distance, in cells, of a query from the box along one axis"""
    best = 0
    for a in range(3):
        if dims[a] == 1:
            continue
        hi = lo[a] + step[a] * (dims[a] - 1)
        best = max(best, int(((lo[a] - q[:, a]).clamp(min=0) // step[a]).max()), int(((q[:, a] - hi).clamp(min=0) // step[a]).max()))
    return best


# ---- the reference ------------------------------------------------------------------------------------------------------------
def d2(q, t):
    """[N, M] int64 squared distances in lattice units (true squared distance * 64)"""
    return ((q[:, None, :] - t[None, :, :]) ** 2).sum(-1)


def knn(q, t, k):
    """[N, k] int64: the k nearest tokens of every query ordered by (distance, token index)"""
    m = t.shape[0]
    key = d2(q, t) * m + torch.arange(m, dtype=torch.int64)
    return torch.argsort(key, dim=1, stable=True)[:, :k]


def radius(centres, others, r2_int, cap=CAP):
    """(centre idx, other idx) int64 lists: for every centre the ``others`` with d2 <= r2_int, ascending index, the first ``cap``;
    grouped by centre (ascending)"""
    hit = d2(centres, others) <= r2_int
    if cap is not None:
        hit = hit & (torch.cumsum(hit.to(torch.int64), dim=1) <= cap)
    c, o = torch.nonzero(hit, as_tuple=True)      # row-major: centre ascending, other ascending inside
    return c, o


def coalesce(e):
    """sort by (row 0, row 1), drop duplicates"""
    if e.shape[1] == 0:
        return e
    big = int(e[1].max()) + 1
    u = torch.unique(e[0] * big + e[1], sorted=True)
    return torch.stack([u // big, u % big])


def knn_edges(q, t, k):
    """[2, N*k] rows [point, token], grouped by point, nearest first"""
    return torch.stack([torch.arange(q.shape[0], dtype=torch.int64).repeat_interleave(k), knn(q, t, k).reshape(-1)])


def encoder_edges(strategy, q, t, r2_int, k):
    """rows [point, token]"""
    if strategy == "knn":
        return knn_edges(q, t, k)
    c, o = radius(t, q, r2_int)                    # centres = tokens: at most CAP points per token
    rad = torch.stack([o, c])
    if strategy == "radius":
        return rad
    if strategy == "bidirectional":
        return coalesce(torch.cat([knn_edges(q, t, k), rad], dim=1))
    raise ValueError(strategy)


def decoder_edges(strategy, q, t, r2_int, k):
    """rows [token, point]"""
    if strategy == "reverse":
        return encoder_edges("bidirectional", q, t, r2_int, k).flip(0)
    if strategy == "knn":
        return knn_edges(q, t, k).flip(0)
    c, o = radius(q, t, r2_int)                    # centres = points: at most CAP tokens per point
    rad = torch.stack([o, c])
    if strategy == "radius":
        return rad
    if strategy == "bidirectional":
        return coalesce(torch.cat([knn_edges(q, t, k).flip(0), rad], dim=1))
    raise ValueError(strategy)


def query_rows(strategy, q, t, r2_int, k):
    """(rowptr [N+1], query ids [E], token ids [E]) of the decoder graph by query, tokens ascending without duplicates, built
    from the per-query definition: the capped radius tokens, for 'bidirectional' united with the k nearest"""
    n, m = q.shape[0], t.shape[0]
    member = torch.zeros(n, m, dtype=torch.bool)
    c, o = radius(q, t, r2_int)
    member[c, o] = True
    if strategy == "bidirectional":
        member.scatter_(1, knn(q, t, k), True)
    elif strategy != "radius":
        raise ValueError(strategy)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(member.sum(1), 0)
    qi, tk = torch.nonzero(member, as_tuple=True)
    return rowptr, qi, tk


# ---- what a set of cases holds (asserted by tests/test_graph_exact_cpu.py) ---------------------------------------------------
def kth_tie_share(q, t, k):
    """share of rows whose k-th and (k+1)-th nearest tokens are at the same distance (k < number of tokens)"""
    s = torch.sort(d2(q, t), dim=1).values
    return float((s[:, k - 1] == s[:, k]).float().mean())


def shell_sizes(q_row, t):
    """cumulative sizes of the distance shells around one query: [number of tokens with d2 <= s for every attained s]"""
    s = torch.sort(d2(q_row[None], t)[0]).values
    last = torch.ones_like(s, dtype=torch.bool)
    last[:-1] = s[1:] != s[:-1]
    return (torch.nonzero(last).flatten() + 1).tolist()


# ---- fp64 brute force for grids that are NOT on the lattice ---------------------------------------------------------------
def knn_fp64(q32, t32, k):
    """(ids [N, k] by (distance, index), sorted squared distances [N, M]) in fp64 on the STORED fp32 coordinates"""
    d = ((q32.double()[:, None, :] - t32.double()[None, :, :]) ** 2).sum(-1)
    order = torch.argsort(d, dim=1, stable=True)
    return order[:, :k], d.gather(1, order)


# ---- the cases (shared by the CPU validity tests and the GPU tests) ---------------------------------------------------------
# name -> (dims, integer origin, integer steps); coordinates = integers / 8
LATTICE_GRIDS = {
    "c5": ((5, 5, 5), (-8, -8, -8), (4, 4, 4)),          # [-1, 1]^3, step 1/2
    "a953": ((9, 5, 3), (-8, -8, -8), (2, 4, 8)),        # [-1, 1]^3, steps 1/4, 1/2, 1
    "c6": ((6, 6, 6), (-4, -4, -4), (2, 2, 2)),          # [-0.5, 0.75]^3, step 1/4: an even node count, no centre node
    "s5": ((5, 5, 5), (-2, -2, -2), (1, 1, 1)),          # [-0.25, 0.25]^3, step 1/8: room for points 12 cells outside
    "an17": ((17, 2, 2), (-8, -8, -8), (1, 16, 16)),     # [-1, 1]^3, steps 1/8, 2, 2: step ratio 16
    "t2": ((2, 2, 2), (-8, -8, -8), (16, 16, 16)),       # k == M == 8 on the register path
    "t4": ((4, 4, 4), (-6, -6, -6), (4, 4, 4)),          # k == M == 64 on the register path
    "d1xx": ((1, 5, 5), (2, -8, -8), (0, 4, 4)),         # one node along an axis, in each position
    "dx1x": ((5, 1, 5), (-8, 2, -8), (4, 0, 4)),
    "dxx1": ((5, 5, 1), (-8, -8, 2), (4, 4, 0)),
    "one": ((1, 1, 1), (2, -4, 6), (0, 0, 0)),           # a single token
}


def lattice_case(name):
    """(dims, (lo, hi) floats, tokens int64 [M, 3], queries int64 [N, 3], kind int64 [N]) -- kind: 0-3 = number of half-step
    coordinates (node, edge midpoint, face centre, cell centre), 4 = a point outside the box"""
    dims, lo, step = LATTICE_GRIDS[name]
    t = grid_ints(dims, lo, step)
    if all(step[a] % 2 == 0 for a in range(3)):
        q, kind = refined_queries(dims, lo, step)
    else:
        q, kind = t.clone(), torch.zeros(t.shape[0], dtype=torch.int64)
    if name == "one":        # points around the single token, some at equal distance from it
        out = torch.tensor([[2, -4, 6], [3, -4, 6], [2, -3, 6], [-16, 16, -16], [16, 16, 16], [2, -4, -10]], dtype=torch.int64)
    else:
        out = outside_queries(dims, lo, tuple(s if s else 1 for s in step))
        if any(dims[a] == 1 for a in range(3)):      # off the plane / line of a degenerate grid as well
            off = q[:: max(q.shape[0] // 16, 1)].clone()
            for a in range(3):
                if dims[a] == 1:
                    off[:, a] += torch.tensor([-5, 3], dtype=torch.int64).repeat(off.shape[0])[: off.shape[0]]
            out = torch.cat([out, off])
    q = torch.cat([q, out])
    kind = torch.cat([kind, torch.full((out.shape[0],), 4, dtype=torch.int64)])
    assert int(q.abs().max()) <= LIMIT and int(t.abs().max()) <= LIMIT
    return dims, grid_box(dims, lo, step), t, q, kind


def perturbed_case(axis, side, w, tol, frac=0.99):
    """A grid OFF the lattice whose window proof is tight (fp64 brute force is its reference).  dims 9 along ``axis`` (step 1/4) and
    3 along the others (step 1) on [-1, 1]^3, all nominal coordinates exact in fp32.  The query sits on the line through the middle
    nodes, just short of half a cell from the base node 4 towards ``side``; its neighbours along that line are, in order, the
    planes 4, 4+s, 4-s, 4+2s, 4-2s, 4+3s.  With k = 2w + 1 the nominal k-th neighbour is plane 4 - s*w, inside the window of
    half-width w, and the first excluded token is plane 4 + s*(w+1).  That token is moved INWARD by delta = frac * tol (``tol``: the
    largest deviation the grid test accepts) and the query placed so that nominally the k-th neighbour wins by delta / 2 -- so the
    moved token truly wins by delta / 2 and a search that stops at this window returns the wrong list.  A second, mirrored query
    (no moved token near it) rides along.
    -> (dims, tokens fp32 [M, 3], queries fp32 [2, 3], k, index of the moved token, index of the displaced k-th neighbour)"""
    assert side in (-1, 1) and w in (1, 2)
    dims = [3, 3, 3]
    dims[axis] = 9
    axes = [torch.linspace(-1.0, 1.0, n, dtype=torch.float64) for n in dims]
    tok = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1)
    delta, step, k = frac * tol, 0.25, 2 * w + 1
    mid = [1, 1, 1]

    def lin(plane):
        c = list(mid)
        c[axis] = plane
        return (c[0] * dims[1] + c[1]) * dims[2] + c[2], tuple(c)

    moved, mc = lin(4 + side * (w + 1))
    kth, _ = lin(4 - side * w)
    tok[mc][axis] -= side * delta
    q = torch.zeros(2, 3, dtype=torch.float64)
    q[0, axis] = side * (0.5 * step - delta / 4)
    q[1, axis] = -side * (0.5 * step - delta / 4)
    return tuple(dims), tok.reshape(-1, 3).to(torch.float32), q.to(torch.float32), k, moved, kth


def ulps_apart(a, b):
    """|a - b| in units of the fp32 spacing at max(|a|, |b|) (a, b: python floats / fp64)"""
    m = max(abs(a), abs(b))
    spacing = float(torch.nextafter(torch.tensor(m, dtype=torch.float32), torch.tensor(float("inf"))) - torch.tensor(m, dtype=torch.float32))
    return abs(a - b) / spacing
