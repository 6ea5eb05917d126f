"""fp64 reference of the statistical GeoEmbed features (csrc/geoembed.hip), stage by stage, its rounding bounds, and the case
graph the CPU and the GPU tests share.  Plain torch, fp64, vectorised with index_add (no loop over rows); it starts from the
fp32 coordinates converted to fp64 and takes nothing from the kernels.

Stages (the kernels' split):
  moments(src, qry, ei)            [Q, 12] = {N, sum d, sum d^2, sum u (3), sum u u^T (xx xy xz yy yz zz)}, u = x - q, d = |u|
  raw_from_moments(mom)            [Q, 9]  = {N, E[d], max(E[d^2] - E[d]^2, 0), centroid - q (3), eigvalsh(cov + 1e-6 I) descending}
  raw_two_sweep(src, qry, ei)      the same, centroid first, then the covariance about it (the form of gaot_geoembed_raw)
  zscore(raw, q_total, colsums)    (raw - mean) / std per column, unbiased std, std < 1e-6 -> 1; Q = 1 gives NaN as torch.std
  features_from_moments(mom)       zscore(raw_from_moments(mom)), differentiable (fp64 autograd = the reference of the backward)
Rows without neighbours are zero before the z-score.  N (column 0 of the moments) is a count, not a function of the coordinates.

Rounding bounds.  u = 2^-24 is the unit round-off of fp32 (half an ulp, relative).  The kernels document these rounding points:
  (1) a distance is formed in fp32 (k_geo_moments / k_geo_raw: "fp32 difference, fp32 norm"): three differences (u each), three
      squares (u each), two additions (u each), one sqrtf (u).  d^2 carries 2u (the differences, squared) + u + 2u = 5u, the root
      halves it and adds its own u: 3.5u, taken as 4u relative per edge; (double)d * (double)d is exact, so d^2 carries 7u, taken as 8u.
  (2) every sum, the variance E[d^2] - E[d]^2, the centroid, the covariance and the Jacobi eigen-solve are fp64.
  (3) a raw feature is rounded to fp32 once (out[i] = (float)...): u |raw|.
  (4) the column mean and the std are rounded to fp32 once (k_geo_colfinal: stats[i] = (float)mean, sd = (float)sqrt(var)).
  (5) k_geo_normalize forms (x - mean) / std in two fp32 operations.
Moments: columns 3..11 are fp64 sums of terms that are computed from identical inputs by identical fp64 operations, so only the order
of the n additions differs (and a multiply-add may be contracted, one rounding fewer): |err| <= n 2^-53 sum|term| to first order,
asserted with 4 n 2^-53 sum|term|.  Columns 1, 2: 4u sum d and 8u sum d^2 from (1); the fp64 summation is 2^-29 of that.
Raw features: columns 0, 3..8 carry (3): u |raw|; the eigenvalues add 1e-14 lambda_max absolute (Jacobi against LAPACK, both a few
2^-53 ||A||, and E[uu^T] - E[u]E[u]^T from fp64 moments cancels at 2^-53 |u|^2); column 1 adds 4u E[d] from (1); column 2 adds
8u E[d^2] + 8u E[d]^2 <= 16u E[d^2] through E[d^2] - E[d]^2.  Call the sum draw.
Z-scored output y = (x - m) / s, x the fp32 raw feature, m and s the fp32 statistics:
  numerator   draw                                      the raw feature's own error
              u |m| + mean over the rows of (draw - u |raw|) + u |m|
                                                        m rounded once (4); the share of the distance terms in the column mean; the
                                                        fp32 roundings (3) of the Q inputs of the mean, to first order u |m| (they
                                                        are independent and of either sign: their mean is far below the worst case)
              u |x - m| <= u (|raw| + |m|)              the fp32 subtraction (5)
              all divided by s
  relative    4u |y|                                    s rounded once (4), s formed from rounded inputs (to first order u, as
                                                        the mean), the fp32 division (5), and one u for the second-order terms
For an fp64-computed column (draw = u |raw|) this is u (2 |raw| + 2 |mean|) / std + 4u |y|; columns 1 and 2 add their distance term
and its share of the mean.  The factor 2 with which every bound is asserted covers fma contraction and the std's own rounding, which
this derivation treats to first order only.  All quantities on the right-hand sides are the reference's."""
import types

import torch

U = 2.0 ** -24
EPS64 = 2.0 ** -53
FACTOR = 2.0          # every derived bound is asserted with this factor over the derived sum
NM, NF = 12, 9


# ---- stages ----------------------------------------------------------------------------------------------------------------------------
def _edge_terms(u):
    d = torch.linalg.vector_norm(u, dim=1)
    ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
    return torch.stack([torch.ones_like(d), d, d * d, ux, uy, uz, ux * ux, ux * uy, ux * uz, uy * uy, uy * uz, uz * uz], dim=1)


def edge_moments(u, qi, num_q):
    """moments of per-edge offsets u [E, 3] (fp64) summed by query row qi [E] -> [Q, 12]; differentiable in u"""
    return torch.zeros(num_q, NM, dtype=torch.float64).index_add(0, qi.long(), _edge_terms(u))


def moments(src, qry, ei, abs_sums=False):
    """[Q, 12] fp64 moments about the query; with ``abs_sums`` the sums of the terms' magnitudes instead (for the bounds)"""
    si, qi = ei[0].long(), ei[1].long()
    u = src.double()[si] - qry.double()[qi]
    if abs_sums:
        return torch.zeros(qry.shape[0], NM, dtype=torch.float64).index_add(0, qi, _edge_terms(u).abs())
    return edge_moments(u, qi, qry.shape[0])


def _assemble(n, davg, ed2, cen, cov):
    has = n > 0.5
    dvar = torch.clamp(ed2 - davg * davg, min=0.0)
    reg = cov + 1e-6 * torch.eye(3, dtype=torch.float64)
    ev = torch.linalg.eigvalsh(reg).flip(dims=[1])
    raw = torch.cat([n[:, None], davg[:, None], dvar[:, None], cen, ev], dim=1)
    return torch.where(has[:, None], raw, torch.zeros_like(raw))


def _sym(xx, xy, xz, yy, yz, zz):
    return torch.stack([torch.stack([xx, xy, xz], 1), torch.stack([xy, yy, yz], 1), torch.stack([xz, yz, zz], 1)], 1)


def raw_from_moments(mom):
    n = mom[:, 0]
    inv = 1.0 / n.clamp(min=1.0)
    c = mom[:, 3:6] * inv[:, None]
    cov = _sym(*(mom[:, 6 + k] * inv for k in range(6))) - c[:, :, None] * c[:, None, :]
    return _assemble(n, mom[:, 1] * inv, mom[:, 2] * inv, c, cov)


def raw_two_sweep(src, qry, ei):
    si, qi = ei[0].long(), ei[1].long()
    nq = qry.shape[0]
    s, q = src.double(), qry.double()
    x = s[si]
    n = torch.zeros(nq, dtype=torch.float64).index_add(0, qi, torch.ones(si.shape[0], dtype=torch.float64))
    inv = 1.0 / n.clamp(min=1.0)
    d = torch.linalg.vector_norm(x - q[qi], dim=1)
    davg = torch.zeros(nq, dtype=torch.float64).index_add(0, qi, d) * inv
    ed2 = torch.zeros(nq, dtype=torch.float64).index_add(0, qi, d * d) * inv
    cen = torch.zeros(nq, 3, dtype=torch.float64).index_add(0, qi, x) * inv[:, None]
    w = x - cen[qi]
    cov = torch.zeros(nq, 3, 3, dtype=torch.float64).index_add(0, qi, w[:, :, None] * w[:, None, :]) * inv[:, None, None]
    return _assemble(n, davg, ed2, cen - q, cov)


def column_sums(raw):
    """the 18 sums gaot_geoembed_raw returns: column sums, then column sums of squares"""
    raw = raw.double()
    return torch.cat([raw.sum(0), (raw * raw).sum(0)])


def column_stats(raw, q_total=None, colsums=None):
    """(mean, std as used, replaced) of the z-score; from ``colsums`` over ``q_total`` rows when given (the sharded form)"""
    if colsums is None:
        q = raw.shape[0]
        assert q_total is None or q_total == q, "rows of a shard need the column sums of all rows"
        mean = raw.sum(0) / q
        var = ((raw - mean) ** 2).sum(0) / (q - 1) if q > 1 else torch.full((raw.shape[1],), float("nan"), dtype=raw.dtype)
    else:
        q = q_total
        mean = colsums[:NF] / q
        var = (colsums[NF:] - q * mean * mean).clamp(min=0.0) / (q - 1) if q > 1 else torch.full((NF,), float("nan"), dtype=torch.float64)
    replaced = var.detach().sqrt() < 1e-6
    std = torch.where(replaced, torch.ones_like(var), var).sqrt()     # (no 0 * inf in the backward of a replaced column)
    return mean, std, replaced


def zscore(raw, q_total=None, colsums=None):
    mean, std, _ = column_stats(raw, q_total, colsums)
    return (raw - mean) / std


def features_from_moments(mom):
    return zscore(raw_from_moments(mom))


# ---- bounds (derivation in the module docstring; reference quantities only; the caller multiplies by FACTOR) --------------------------
def rounding_bound_moments(abs_mom):
    """[Q, 12] from moments(..., abs_sums=True): column 0 exact, 1-2 the fp32 distance, 3-11 the order of n fp64 additions"""
    n = abs_mom[:, :1]
    b = 4.0 * n * EPS64 * abs_mom
    b[:, 0] = 0.0
    b[:, 1] = 4.0 * U * abs_mom[:, 1]
    b[:, 2] = 8.0 * U * abs_mom[:, 2]
    return b


def rounding_bound_moment_order(abs_mom):
    """moments of the same edges summed in another order (the fp32 distances are the same numbers): fp64 order bound in every column"""
    b = 4.0 * abs_mom[:, :1] * EPS64 * abs_mom
    b[:, 0] = 0.0
    return b


def rounding_bound_raw(raw, mom):
    """[Q, 9] error bound of the un-normalised fp32 features"""
    n = mom[:, 0]
    inv = 1.0 / n.clamp(min=1.0)
    b = U * raw.abs()
    b[:, 1] += 4.0 * U * mom[:, 1] * inv
    b[:, 2] += 16.0 * U * mom[:, 2] * inv
    b[:, 6:9] += 1e-14 * raw[:, 6:7].abs()
    return torch.where((n > 0.5)[:, None], b, torch.zeros_like(b))


def rounding_bound_zscore(raw, draw):
    """[Q, 9] error bound of the z-scored fp32 output over ALL rows of the z-score; ``draw`` = rounding_bound_raw of the same rows"""
    mean, std, _ = column_stats(raw)
    y = (raw - mean) / std
    share = (draw - U * raw.abs()).mean(0)      # of the distance (and eigen-solve) terms in the column mean
    return (draw + U * (raw.abs() + 2.0 * mean.abs()) + share) / std + 4.0 * U * y.abs()


def ratio(err, bound, factor=FACTOR):
    """err / (factor * bound) elementwise: 0 where the error is 0 (an exact result, whatever the bound), inf where only the bound is 0"""
    r = err / (factor * bound)
    return torch.where(err == 0, torch.zeros_like(r), torch.where(bound > 0, r, torch.full_like(r, float("inf"))))


def emulate_fp32(raw):
    """the kernels' rounding points (3)-(5) and nothing else: fp64 raw features rounded to fp32, mean and std of the fp32 values
    rounded to fp32, the normalisation in fp32 -> (raw fp32, z-scored fp32)"""
    x = raw.float()
    mean, std, _ = column_stats(x.double())
    return x, (x - mean.float()) / std.float()


# ---- the case graph -------------------------------------------------------------------------------------------------------------------
DEGREES = (0, 1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 257)
CRAFTED = ("collinear", "coplanar", "octahedron", "coincident", "jittered_line", "duplicate")
BULK_ROWS, BULK_POOL = 72, 200


def _uniform(gen, n):
    return (torch.rand(n, 3, generator=gen, dtype=torch.float64) * 2 - 1).float()


def _tile(src, qry, ei, tile):
    """``tile`` copies of a graph side by side: copy k owns sources k S .. (k + 1) S and query rows k Q .. (k + 1) Q"""
    if tile == 1:
        return src, qry, ei
    k = torch.arange(tile)
    ei = torch.stack([(ei[0][None] + k[:, None] * src.shape[0]).reshape(-1), (ei[1][None] + k[:, None] * qry.shape[0]).reshape(-1)])
    return src.repeat(tile, 1), qry.repeat(tile, 1), ei


def case_graph(offset=0.0, tile=1, seed=0):
    """-> namespace(src [S, 3] fp32, qry [Q, 3] fp32, ei [2, E] int64 shuffled, rows {label: query row}, sources {label: source ids},
    num_src, num_q).  One query row per degree in DEGREES and one per crafted case, each with private sources, and BULK_ROWS rows of
    degree 0..12 over a shared pool; rows permuted, edges shuffled; ``offset`` is added to every coordinate (in fp32), ``tile``
    replicates the graph (labels name the first copy)."""
    gen = torch.Generator().manual_seed(seed)
    pool = _uniform(gen, BULK_POOL)
    src_parts, qry_parts, edges, labels, priv = [pool], [], [], [], {}
    ns = BULK_POOL

    def add_row(label, q, pts, ids=None):
        nonlocal ns
        row = len(qry_parts)
        qry_parts.append(q.reshape(1, 3))
        if ids is None:
            ids = torch.arange(ns, ns + pts.shape[0])
            src_parts.append(pts)
            ns += pts.shape[0]
        labels.append(label)
        priv[label] = torch.unique(ids)
        edges.append(torch.stack([ids, torch.full_like(ids, row)]))

    for d in DEGREES:
        add_row(f"deg{d}", _uniform(gen, 1)[0], _uniform(gen, d))
    q = _uniform(gen, 1)[0]
    t = torch.tensor([-0.8, -0.3, 0.1, 0.45, 0.9])
    add_row("collinear", q, q + t[:, None] * torch.tensor([0.48, -0.6, 0.64]))
    q = _uniform(gen, 1)[0]
    ab = _uniform(gen, 6)[:, :2]
    add_row("coplanar", q, q + 0.1 + ab[:, :1] * torch.tensor([0.6, 0.8, 0.0]) + ab[:, 1:] * torch.tensor([0.0, 0.0, 1.0]))
    q = torch.tensor([0.25, -0.5, 0.125])      # exactly representable with +-0.25 at both offsets: the covariance is exactly r^2/3 I
    add_row("octahedron", q, q + 0.25 * torch.cat([torch.eye(3), -torch.eye(3)]))
    q = _uniform(gen, 1)[0]
    add_row("coincident", q, torch.cat([q[None], q + 0.3 * _uniform(gen, 4)]))
    q = _uniform(gen, 1)[0] * 0.5
    t = torch.linspace(-0.5, 0.5, 12)
    jit = 1e-4 * _uniform(gen, 12)
    add_row("jittered_line", q, q + 0.05 + t[:, None] * torch.tensor([0.6, 0.0, 0.8]) + jit)
    q = _uniform(gen, 1)[0]
    p = q + 0.2 * _uniform(gen, 1)
    add_row("duplicate", q, p, ids=torch.full((4,), ns))
    src_parts.append(p)
    ns += 1
    for i in range(BULK_ROWS):
        d = int(torch.randint(0, 13, (1,), generator=gen))
        add_row(f"bulk{i}", _uniform(gen, 1)[0], None, ids=torch.randperm(BULK_POOL, generator=gen)[:d])
    src, qry, ei = torch.cat(src_parts), torch.cat(qry_parts), torch.cat(edges, dim=1)
    nq = qry.shape[0]
    perm = torch.randperm(nq, generator=gen)             # new row of old row r = perm[r]
    qry_p = torch.empty_like(qry)
    qry_p[perm] = qry
    ei = torch.stack([ei[0], perm[ei[1]]])
    rows = {lab: int(perm[r]) for r, lab in enumerate(labels)}
    src, qry_p, ei = _tile(src, qry_p, ei, tile)
    ei = ei[:, torch.randperm(ei.shape[1], generator=gen)]
    off = torch.tensor(float(offset), dtype=torch.float32)
    return types.SimpleNamespace(src=(src + off).contiguous(), qry=(qry_p + off).contiguous(), ei=ei.contiguous(), rows=rows,
                                 sources=priv, num_src=src.shape[0], num_q=qry_p.shape[0])


def degree_graph(degrees, num_q, pool=64, seed=0, offset=0.0, tile=1):
    """num_q rows whose degrees cycle through ``degrees``, sources drawn from a pool (vectorised: the large-Q cases), replicated
    ``tile`` times; edges shuffled"""
    gen = torch.Generator().manual_seed(seed)
    deg = torch.tensor(degrees)[torch.arange(num_q) % len(degrees)]
    dst = torch.arange(num_q).repeat_interleave(deg)
    srcid = torch.randint(0, pool, (int(deg.sum()),), generator=gen)
    src, qry, ei = _tile(_uniform(gen, pool), _uniform(gen, num_q), torch.stack([srcid, dst]), tile)
    ei = ei[:, torch.randperm(ei.shape[1], generator=gen)]
    off = torch.tensor(float(offset), dtype=torch.float32)
    return types.SimpleNamespace(src=(src + off).contiguous(), qry=(qry + off).contiguous(), ei=ei.contiguous(), num_src=src.shape[0],
                                 num_q=qry.shape[0])
