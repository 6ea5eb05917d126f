"""The statistical GeoEmbed kernels (csrc/geoembed.hip: 11 kernels, 8 entry points) against the fp64 stage reference of
tests/geoembed_stat_ref.py, entry point by entry point through the C ABI, every output pre-filled with NaN.

Forward, on the case graph (one row per degree around the 8-lane group and the 32-edge trip of the moment loop, rank-0 / 1 / 2 / isotropic
covariances, a coincident source, a 1e8 eigenvalue ratio; offsets 0 and +100): gaot_geoembed_moments (degree exact, fp64 columns within the
summation-order bound, the two fp32-distance columns within 4u / 8u, additivity over a split edge list), gaot_geoembed_raw (elementwise
raw bound, exact (float)1e-6 eigenvalues and zero variance on the duplicate-point and degree-1 rows, zero empty rows, the 18 column
sums), gaot_geoembed_from_moments and gaot_geoembed_raw + gaot_geoembed_finalize (elementwise z-score bound; unequal query shards with
num_queries_total = Q; a zero-row shard), the project's 5e-5 bar per COLUMN peak, and at offset +100 the kernels at least 4 x closer to
fp64 than the fp32 oracle in the centroid columns.  Z-score edges: Q = 1 (NaN), 2, all rows empty, a constant column, a std of 1e-7
(replaced) and 1e-5 (kept), Q around the 256-row block, at 9 and 10 column partials, and above 65536 rows (the grid-stride loop).
Backward: gaot_geoembed_from_moments_bwd against fp64 autograd of features_from_moments on the kernel's own moments,
gaot_geoembed_moments_bwd against fp64 autograd of the moments, GeoStatFn end to end against the oracle, separately on every
rank-deficient row.  Host: the feature cache of GeometricEmbedding.forward.  Every entry point is called twice: torch.equal.

Bounds: derived in tests/geoembed_stat_ref.py from the rounding points the kernels document, asserted with a factor 2 (the moments: as
stated there, without it).  Column 0 of the moment adjoint is the kernel's 0: the degree is a count, not a function of the coordinates.
A row whose eigenvalues are not pairwise separated by 1e-3 lambda_max has a basis-dependent eigenvalue adjoint (in the reference as well):
with a random cotangent only its columns 1-2 are compared; with eigenvalue cotangents that the z-score backward maps to ONE value per row
(std_c w, w orthogonal to 1 and to the three z-scored eigenvalue columns: dA = w I in every basis) all of columns 1-11 are.
The sharded result is held within 4 fp32 ulps of the unsharded one, ulp = 2^-23 |y| (the shards' column sums are added in another order,
which can move the fp32 mean or std only where an fp64 sum sits on a rounding boundary; measured: bit-identical).

Measured on an MI355X (profiles/parity_geoembed_stat.txt; "b / p" = worst distance to fp64 as a fraction of the asserted bound / of the
column's peak, the worse of offsets 0 and +100):
  moments        N, Sux..Suz exact; Sd 0.35 / 1.6e-9, Sd2 0.35 / 3.9e-9 (a degree-1..12 bulk row); Sxx..Szz <= 0.09 / 1.0e-15; at +100 the
                 second moments are bit-identical to the reference; split edge list: <= 0.09 / 4.4e-16
  raw            degree exact; d_avg 0.14 / 7.0e-8, d_var 0.02 / 8.1e-8; cen_x 0.47 / 3.6e-8, cen_y 0.47 / 3.9e-8, cen_z 0.50 / 3.6e-8 (the
                 degree-1 row: one fp32 rounding, half of the factor-2 bound by construction); lam0 0.48 / 4.2e-8, lam1 0.43 / 3.3e-8,
                 lam2 0.48 / 4.5e-8; column sums 2.3e-16 of sum|v| (bound 2.2e-14)
  z-scored       from_moments = raw + finalize = the sharded form, element for element (0 of 873 differ): degree 0.11 / 8.0e-8,
                 d_avg 0.07 / 1.4e-7, d_var 0.01 / 1.4e-7, cen_x 0.25 / 1.1e-7 (a bulk row; the coplanar row at +100), cen_y 0.14 / 6.5e-8,
                 cen_z 0.16 / 8.0e-8, lam0 0.17 / 6.3e-8, lam1 0.17 / 7.3e-8, lam2 0.17 / 9.1e-8
  z-score edges  worst over Q = 2, 31, 32, 33, 257, 2049, 2305, 65836, the constant degree and both std cases: 0.33 / 1.1e-7 (cen_y, the
                 constant-degree graph and Q = 32); Q = 65836: <= 0.25 / 1.8e-7
  offset +100    centroid columns: kernels 3.3e-7 from fp64 (both forms), the fp32 oracle 6.8e-5: 208 x closer
  backward       from_moments_bwd <= 8.2e-7 of a column's peak (bar 1e-3), moments_bwd 5.5e-8, GeoStatFn 5.2e-7; the octahedron is the one row
                 whose source admits both branches of the d_var clamp, and the kernel takes the other than torch (0 per edge apart in
                 the coordinates, 1.08 apart in Sd)."""
import os
import sys
import types

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import geoembed_stat_ref as R  # noqa: E402
import test_coord_grad_gpu as cg  # noqa: E402  (FP32_BAR, check, oracle_grads, product_grads, orc)

orc = cg.orc
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32_BAR = cg.FP32_BAR
NAN = float("nan")
COLS = ("degree", "d_avg", "d_var", "cen_x", "cen_y", "cen_z", "lam0", "lam1", "lam2")
MCOLS = ("N", "Sd", "Sd2", "Sux", "Suy", "Suz", "Sxx", "Sxy", "Sxz", "Syy", "Syz", "Szz")


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """the workspaces of these tests stay cached in torch's allocator; later tests that bound the rise of allocated memory are sensitive
    to which cached blocks they are served from, so the cache is handed back when this module is done"""
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- the entry points through the C ABI --------------------------------------------------------------------------------------------------
def _lib_ops():
    from gaot_3d_amd import _lib, ops
    return _lib.load(), ops


def _nan(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def k_moments(src, qry, g):
    lib, ops = _lib_ops()
    mom = _nan((g.num_dst, 12), torch.float64)
    rc = lib.gaot_geoembed_moments(ops._ptr(src), ops._ptr(qry), ops._ptr(g.by_dst.rowptr), ops._ptr(g.by_dst.other), g.num_dst,
                                   ops._ptr(mom), ops._stream())
    assert rc == 0, lib.gaot_last_error()
    return mom


def k_from_moments(mom):
    lib, ops = _lib_ops()
    feat = _nan((mom.shape[0], 9), torch.float32)
    ws = ops._ws(lib.gaot_geoembed_stats_workspace_bytes(), DEV)
    rc = lib.gaot_geoembed_from_moments(ops._ptr(mom), mom.shape[0], ops._ptr(feat), ops._ptr(ws), ws.numel(), ops._stream())
    assert rc == 0, lib.gaot_last_error()
    return feat


def k_raw(src, qry, g, row0=0, row1=None, feat=None):
    """rows row0 .. row1 of the graph (a query shard): -> (their un-normalised features, the 18 column sums)"""
    lib, ops = _lib_ops()
    row1 = g.num_dst if row1 is None else row1
    q = row1 - row0
    feat = _nan((q, 9), torch.float32) if feat is None else feat
    sums = _nan((18,), torch.float64)
    ws = ops._ws(lib.gaot_geoembed_stats_workspace_bytes(), DEV)
    rc = lib.gaot_geoembed_raw(ops._ptr(src), ops._ptr(qry[row0:row1]), ops._ptr(g.by_dst.rowptr[row0:row1 + 1]), ops._ptr(g.by_dst.other),
                               q, ops._ptr(feat), ops._ptr(sums), ops._ptr(ws), ws.numel(), ops._stream())
    assert rc == 0, lib.gaot_last_error()
    return feat, sums


def k_finalize(feat, sums, q_total):
    lib, ops = _lib_ops()
    ws = ops._ws(lib.gaot_geoembed_stats_workspace_bytes(), DEV)
    rc = lib.gaot_geoembed_finalize(ops._ptr(feat), feat.shape[0], ops._ptr(sums), q_total, ops._ptr(ws), ws.numel(), ops._stream())
    assert rc == 0, lib.gaot_last_error()
    return feat


def k_two_sweep(src, qry, g):
    feat, sums = k_raw(src, qry, g)
    return k_finalize(feat, sums, g.num_dst)


def k_from_moments_bwd(mom, gy):
    lib, ops = _lib_ops()
    q = mom.shape[0]
    adj = _nan((q, 12), torch.float64)
    ws = ops._ws(lib.gaot_geoembed_from_moments_bwd_workspace_bytes(q), DEV)
    rc = lib.gaot_geoembed_from_moments_bwd(ops._ptr(mom), ops._ptr(gy), q, ops._ptr(adj), ops._ptr(ws), ws.numel(), ops._stream())
    assert rc == 0, lib.gaot_last_error()
    return adj


def k_moments_bwd(src, qry, g, adj):
    lib, ops = _lib_ops()
    ge, gq = _nan((g.by_dst.num_edges, 3), torch.float32), _nan((g.num_dst, 3), torch.float32)
    rc = lib.gaot_geoembed_moments_bwd(ops._ptr(src), ops._ptr(qry), ops._ptr(g.by_dst.rowptr), ops._ptr(g.by_dst.other), g.num_dst,
                                       ops._ptr(adj), ops._ptr(ge), ops._ptr(gq), ops._stream())
    assert rc == 0, lib.gaot_last_error()
    return ge, gq


def twice(fn, *args):
    """every entry point called twice is torch.equal (NaN compares equal to itself here: Q = 1)"""
    a, b = fn(*args), fn(*args)
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert torch.equal(torch.nan_to_num(x, nan=12345.0), torch.nan_to_num(y, nan=12345.0)), fn.__name__
    return a


def prepare(c, g=None):
    """device copies, the neighbour lists and the fp64 reference of every stage (computed once per graph, left unchanged)"""
    _, ops = _lib_ops()
    c.d_src, c.d_qry = c.src.to(DEV), c.qry.to(DEV)
    c.g = ops.build_graph(c.ei.to(DEV), c.num_src, c.num_q) if g is None else g
    c.mom = R.moments(c.src, c.qry, c.ei)
    c.abs_mom = R.moments(c.src, c.qry, c.ei, abs_sums=True)
    c.raw = R.raw_from_moments(c.mom)
    c.draw = R.rounding_bound_raw(c.raw, c.mom)
    c.y = R.zscore(c.raw)
    c.dy = R.rounding_bound_zscore(c.raw, c.draw)
    c.names = {v: k for k, v in getattr(c, "rows", {}).items()}
    return c


@pytest.fixture(scope="module", params=(0.0, 100.0), ids=["offset0", "offset100"])
def case(request):
    c = prepare(R.case_graph(offset=request.param))
    c.tag = f"offset{int(request.param)}"
    return c


def within(stage, c, got, ref, bound, cols, factor=R.FACTOR, nan_ok=False):
    """one [parity] line per column: the worst distance to fp64 as a fraction of the asserted bound and of the column's peak, and the
    row it occurs in; asserts no NaN and every element within factor x bound"""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (stage, got.shape, ref.shape)
    assert nan_ok or not torch.isnan(got).any(), f"{stage}: NaN left in the output"
    err = (got - ref).abs()
    rat = R.ratio(err, bound, factor)
    for k, name in enumerate(cols):
        i = int(rat[:, k].argmax())
        peak = ref[:, k].abs().max().item()
        print(f"[parity] geoembed_stat/{stage} {name}: max_abs={err[:, k].max().item():.3e} of_bound={rat[i, k].item():.3f} "
              f"of_peak={err[:, k].max().item() / (peak + 1e-300):.3e} worst_row={c.names.get(i, i)}")
    bad = (rat > 1.0).nonzero()
    assert bad.numel() == 0, f"{stage}: beyond the bound at (row, column) {bad[:8].tolist()}, ratios {rat[rat > 1.0][:8].tolist()}"
    return err


def column_peak_bar(stage, got, ref):
    """the project's outer bar (tests/test_fullsize_oracle_gpu.py: 5e-5), applied to every column against that column's own peak"""
    err = (got.detach().double().cpu() - ref).abs().max(0).values
    peak = ref.abs().max(0).values
    assert (err <= 5e-5 * peak).all(), (stage, (err / peak).tolist())


# ---- forward, by stage --------------------------------------------------------------------------------------------------------------------
def test_moments(case):
    c = case
    mom = twice(k_moments, c.d_src, c.d_qry, c.g)
    deg = torch.bincount(c.ei[1], minlength=c.num_q)
    assert torch.equal(mom[:, 0].cpu(), deg.double())                                            # the degree, exactly
    within(f"moments/{c.tag}", c, mom, c.mom, R.rounding_bound_moments(c.abs_mom), MCOLS, factor=1.0)
    assert not mom.cpu()[deg == 0].any()
    # additivity: the edge list split in two, the moments added
    _, ops = _lib_ops()
    half = c.ei.shape[1] // 2 + 3
    parts = [k_moments(c.d_src, c.d_qry, ops.build_graph(e.contiguous().to(DEV), c.num_src, c.num_q)) for e in (c.ei[:, :half], c.ei[:, half:])]
    within(f"moments_split/{c.tag}", c, parts[0] + parts[1], mom.cpu(), R.rounding_bound_moment_order(c.abs_mom), MCOLS, factor=1.0)


def test_raw_features_and_column_sums(case):
    c = case
    feat, sums = twice(k_raw, c.d_src, c.d_qry, c.g)
    assert not torch.isnan(sums).any()
    within(f"raw/{c.tag}", c, feat, R.raw_two_sweep(c.src, c.qry, c.ei), c.draw, COLS)
    f = feat.cpu()
    tiny = torch.tensor(1e-6, dtype=torch.float64).float()
    for lab in ("duplicate", "deg1"):
        r = c.rows[lab]
        assert torch.equal(f[r, 6:9], tiny.expand(3)) and f[r, 2] == 0, (lab, f[r].tolist())
    assert not f[c.mom[:, 0] == 0].any()                                                          # empty rows: exactly 0
    f64 = f.double()
    ref_sums = R.column_sums(f64)
    mag = torch.cat([f64.abs().sum(0), (f64 * f64).sum(0)])
    err = (sums.cpu() - ref_sums).abs()
    print(f"[parity] geoembed_stat/raw_colsums/{c.tag}: worst |sum - fp64 sum of the returned features| / sum|v| = {(err / mag).max().item():.3e} "
          f"(bound {c.num_q * 2.0 ** -52:.3e})")
    # relative to sum|v| (sum v^2), not to the sum itself: the error of an fp64 summation scales with the magnitudes added, and the
    # centroid columns cancel (their sum is a small fraction of sum|v|)
    assert (err <= c.num_q * 2.0 ** -52 * mag).all()


def test_from_moments(case):
    c = case
    feat = twice(k_from_moments, k_moments(c.d_src, c.d_qry, c.g))
    within(f"from_moments/{c.tag}", c, feat, c.y, c.dy, COLS)
    column_peak_bar(f"from_moments/{c.tag}", feat, c.y)


def test_raw_finalize_whole_and_in_query_shards(case):
    c = case
    whole = twice(k_two_sweep, c.d_src, c.d_qry, c.g)
    within(f"raw_finalize/{c.tag}", c, whole, c.y, c.dy, COLS)
    column_peak_bar(f"raw_finalize/{c.tag}", whole, c.y)
    # two shards of unequal size and one without rows; the column sums added as the all-reduce adds them
    cut = 37
    out = _nan((c.num_q, 9), torch.float32)
    shards = [(0, cut), (cut, c.num_q), (c.num_q, c.num_q)]
    sums = [k_raw(c.d_src, c.d_qry, c.g, a, b, out[a:b])[1] for a, b in shards]
    assert torch.equal(sums[2], torch.zeros(18, dtype=torch.float64, device=DEV))                 # over the NaN pre-fill
    total = sums[0] + sums[1] + sums[2]
    for a, b in shards:
        k_finalize(out[a:b], total, c.num_q)
    within(f"raw_finalize_sharded/{c.tag}", c, out, c.y, c.dy, COLS)
    ulp = 2.0 ** -23 * c.y.abs()
    d = (out.double().cpu() - whole.double().cpu()).abs()
    print(f"[parity] geoembed_stat/sharded_vs_whole/{c.tag}: worst difference {R.ratio(d, ulp, 1.0).max().item():.2f} ulps, "
          f"{int((d > 0).sum())} of {d.numel()} elements differ")
    assert (d <= 4.0 * ulp).all()


def test_offset_100_closer_to_fp64_than_the_fp32_oracle():
    """fp64 accumulators: with every coordinate moved by +100 the fp32 oracle loses the centroid columns to cancellation (4.5e-5 on the CPU),
    the kernels do not"""
    c = prepare(R.case_graph(offset=100.0))
    o = (orc.geoembed_stat_features(c.src, c.qry, c.ei).double() - c.y)[:, 3:6].abs().max().item()
    for name, feat in (("from_moments", k_from_moments(k_moments(c.d_src, c.d_qry, c.g))), ("raw_finalize", k_two_sweep(c.d_src, c.d_qry, c.g))):
        k = (feat.double().cpu() - c.y)[:, 3:6].abs().max().item()
        print(f"[parity] geoembed_stat/offset100 centroid columns {name}: kernel max_abs={k:.3e}, fp32 oracle max_abs={o:.3e}, ratio {o / k:.1f}")
        assert k < 2e-6 and 4.0 * k <= o, (name, k, o)


# ---- z-score edges ------------------------------------------------------------------------------------------------------------------------
MIXED = (0, 1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33)


def _one_neighbour_rows(step):
    """four queries at the origin, row i with one neighbour at (step * i, 0, 0): d_avg and cen_x have a std of 1.29 * step"""
    q = 4
    src = torch.zeros(q, 3)
    src[:, 0] = step * torch.arange(q)
    return types.SimpleNamespace(src=src, qry=torch.zeros(q, 3), ei=torch.stack([torch.arange(q), torch.arange(q)]), num_src=q, num_q=q)


def _both_forms(c):
    return (("from_moments", twice(k_from_moments, k_moments(c.d_src, c.d_qry, c.g))), ("raw_finalize", twice(k_two_sweep, c.d_src, c.d_qry, c.g)))


def _edge_case(tag, c):
    prepare(c)
    for form, feat in _both_forms(c):
        within(f"{tag}/{form}", c, feat, c.y, c.dy, COLS)
    return c


def test_zscore_one_row_is_nan_as_torch_std():
    c = prepare(R.degree_graph((3,), 1))
    assert torch.isnan(c.y).all()
    for form, feat in _both_forms(c):
        assert torch.isnan(feat).all(), form


def test_zscore_two_rows():
    _edge_case("q2", R.degree_graph((3, 7), 2))


def test_zscore_all_rows_empty():
    _, ops = _lib_ops()
    none = torch.zeros(1, dtype=torch.int32, device=DEV)                   # (a valid address for a list without edges)
    lists = ops.SortedEdges(torch.zeros(6, dtype=torch.int32, device=DEV), None, none[:0], none, 5)
    c = prepare(R.degree_graph((0,), 5), ops.BipartiteGraph(lists, None, 64, 5))
    assert not c.y.any()
    for form, feat in _both_forms(c):
        assert torch.equal(feat, torch.zeros(5, 9, device=DEV)), form


def test_zscore_constant_degree_column_is_exactly_zero():
    c = _edge_case("const_degree", R.degree_graph((8,), 40))
    for form, feat in _both_forms(c):
        assert not feat[:, 0].any(), form


@pytest.mark.parametrize("step,replaced", [(1e-7, True), (1e-5, False)], ids=["std1e-7_replaced", "std1e-5_kept"])
def test_zscore_std_either_side_of_the_threshold(step, replaced):
    c = _edge_case(f"std_step{step:g}", _one_neighbour_rows(step))
    mean, std, rep = R.column_stats(c.raw)
    sd = c.raw.std(0)
    assert (0.1e-6 if replaced else 10e-6) < sd[1] < (0.13e-6 if replaced else 13e-6) and sd[1] == sd[3]    # a decade from 1e-6
    assert rep.tolist() == [True, replaced, True, replaced, True, True, True, True, True]
    if replaced:                                        # std -> 1: the output is raw - mean (c.y is exactly that)
        assert torch.equal(c.y, c.raw - mean)


@pytest.mark.parametrize("q", [31, 32, 33, 257, 2049, 2305])
def test_zscore_row_counts_around_blocks_and_partial_lanes(q):
    """one and two 256-row blocks; 9 and 10 column partials wrap the 8 partial lanes of k_geo_colfinal / k_geo_colsums"""
    _edge_case(f"q{q}", R.degree_graph(MIXED, q, seed=q))


def test_zscore_above_65536_rows_grid_stride():
    """256 blocks of 256 threads cover 65536 rows: above that k_geo_colpart (and k_geo_bwd_colpart) loop"""
    c = R.degree_graph((0, 1, 2, 3), 16459, tile=4, seed=5)
    assert c.num_q == 65536 + 300 and c.ei.shape[1] < 200_000
    _edge_case("q65836", c)


# ---- backward, by stage -------------------------------------------------------------------------------------------------------------------
def _cotangent(c, common):
    """[Q, 9] fp32, seeded; ``common``: the eigenvalue columns are std_c * w with w orthogonal to 1 and to the z-scored eigenvalue columns, so
    that the z-score backward hands every row ONE eigenvalue cotangent w_r (dA = w_r I whatever the eigenbasis)"""
    gy = torch.randn(c.num_q, 9, dtype=torch.float64, generator=torch.Generator().manual_seed(23))
    if common:
        _, std, _ = R.column_stats(c.raw)
        basis = torch.linalg.qr(torch.cat([torch.ones(c.num_q, 1, dtype=torch.float64), c.y[:, 6:9]], dim=1)).Q
        w = torch.randn(c.num_q, dtype=torch.float64, generator=torch.Generator().manual_seed(29))
        w = w - basis @ (basis.T @ w)
        w = w - basis @ (basis.T @ w)
        gy[:, 6:9] = std[6:9] * w[:, None]
    return gy.float()


def _clamp_branches(m1, m2, n):
    """the branches (True = the gradient passes, input >= 0) that "m[2] * inv - davg * davg" can take as the source is written: evaluated
    in exact rational arithmetic for each contraction -ffp-contract=fast allows (none; an fma over the first product, m2 * inv unrounded; an
    fma over the second, davg * davg unrounded) -- nothing of the kernel's output enters"""
    from fractions import Fraction as F
    inv = 1.0 / n
    davg = m1 * inv
    forms = (F(m2 * inv) - F(davg * davg), F(m2) * F(inv) - F(davg * davg), F(m2 * inv) - F(davg) * F(davg))
    return {float(f) >= 0.0 for f in forms}


def _either_side_of_the_clamp(tag, c, m64, ref, draw_ct, adj):
    """d_var = max(E[d^2] - E[d]^2, 0) has a kink where all neighbours of a row are equidistant (one neighbour, one point listed several
    times, the octahedron): there the sign of a ROUNDING ERROR picks the branch of the clamp.  torch evaluates m2 / n - d_avg^2 with every
    product rounded (exactly 0 on the octahedron: the gradient passes); k_geo_from_moments_bwd (csrc/geoembed.hip, "const double dvar =
    m[2] * inv - davg * davg") may be contracted to one fma, and with the product m2 * inv unrounded the octahedron gives -3.5e-18: blocked,
    consistently with the clamp of the kernel's own forward.  Which branches the source admits is computed from the moments in exact
    arithmetic (_clamp_branches): where it admits one (one neighbour, the duplicate point: every form is exactly 0) the reference keeps
    that branch; where it admits both, the adjoint's columns Sd and Sd2 may be those of either -- and then the two branches must be the
    same function of the coordinates: pushed through the moments' backward, their difference (2 u - 2 d_avg u / d) d_var_cotangent / n
    vanishes on equidistant edges; asserted per edge at the bar.  -> the reference, with the kernel's branch on the rows that admit both"""
    n = m64[:, 0]
    inv = 1.0 / n.clamp(min=1.0)
    davg, ed2 = m64[:, 1] * inv, m64[:, 2] * inv
    slack = ed2 - davg * davg
    kink = (n > 0) & (slack.abs() <= 8.0 * R.EPS64 * ed2)
    delta = torch.zeros_like(ref)                         # passing branch - blocking branch
    delta[:, 1] = -2.0 * davg * inv * draw_ct[:, 2]
    delta[:, 2] = inv * draw_ct[:, 2]
    alt = torch.where((slack >= 0)[:, None], ref - delta, ref + delta)
    use_alt = torch.zeros_like(kink)
    src64, qry64 = c.src.double(), c.qry.double()
    for r in kink.nonzero().reshape(-1).tolist():
        branches = _clamp_branches(m64[r, 1].item(), m64[r, 2].item(), n[r].item())
        if len(branches) == 1:
            use_alt[r] = (slack[r].item() >= 0.0) not in branches
            continue
        use_alt[r] = bool((adj[r] - alt[r])[1:3].abs().sum() < (adj[r] - ref[r])[1:3].abs().sum())
        e = c.ei[1] == r
        u = src64[c.ei[0, e]] - qry64[r]
        g = u * (delta[r, 1] / torch.linalg.vector_norm(u, dim=1) + 2.0 * delta[r, 2])[:, None]
        print(f"[parity] geoembed_stat/from_moments_bwd/{tag} clamp kink, row {c.names.get(r, r)} (degree {int(n[r])}): the source admits both "
              f"branches, the kernel takes {'the other than' if use_alt[r] else 'the same as'} torch; they differ by {g.abs().max().item():.3e} per edge "
              f"in the coordinates, {delta[r, 1].abs().item():.3e} in Sd")
        assert g.abs().max().item() <= FP32_BAR[0] * delta[r, 1].abs().item()
    return torch.where(use_alt[:, None], alt, ref)


def _from_moments_bwd_case(tag, c, common_too=True):
    mom = k_moments(c.d_src, c.d_qry, c.g)
    m64 = mom.cpu()
    n = m64[:, 0]
    lam = c.raw[:, 6:9]
    separated = (n > 0) & (torch.minimum(lam[:, 0] - lam[:, 1], lam[:, 1] - lam[:, 2]) > 1e-3 * lam[:, 0])
    others = (n > 0) & ~separated
    for common in ((False, True) if common_too else (False,)):
        gy = _cotangent(c, common)
        leaf = m64.clone().requires_grad_()
        raw = R.raw_from_moments(leaf)
        raw.retain_grad()
        (R.zscore(raw) * gy.double()).sum().backward()
        adj = twice(k_from_moments_bwd, mom, gy.to(DEV)).cpu()
        assert not torch.isnan(adj).any()
        assert not adj[n == 0].any() and not adj[:, 0].any()                                   # empty rows, and the count's column
        ref = _either_side_of_the_clamp(f"{tag}/{'common' if common else 'random'}", c, m64, leaf.grad, raw.grad, adj)
        kind = "common" if common else "random"
        full = (n > 0) if common else separated
        if full.any():
            for k in range(1, 12):
                name = f"geoembed_stat/from_moments_bwd/{tag}/{kind} cotangent/{int(full.sum())} rows/{MCOLS[k]}"
                if common and k in (7, 8, 10):
                    # dA = w I: the reference's off-diagonal adjoint is zero up to fp64 round-off, so these columns have no peak of their
                    # own; they are held to the bar against the peak of the covariance adjoint they belong to (columns Sxx .. Szz)
                    err, peak = (adj[full, k] - ref[full, k]).abs().max().item(), ref[full][:, 6:12].abs().max().item()
                    print(f"[parity] {name}: max_abs={err:.3e} rel_to_peak_of_the_covariance_adjoint={err / peak:.3e} peak={peak:.3e}")
                    assert err <= FP32_BAR[0] * peak, (name, err, peak)
                else:
                    cg.check(name, adj[full, k], ref[full, k], FP32_BAR)
        if not common and others.any():
            for k in (1, 2):
                cg.check(f"geoembed_stat/from_moments_bwd/{tag}/random cotangent/{int(others.sum())} unseparated rows/{MCOLS[k]}",
                         adj[others, k], ref[others, k], FP32_BAR)
    return separated, others


def test_from_moments_bwd(case):
    c = case
    separated, others = _from_moments_bwd_case(c.tag, c)
    for lab in ("deg1", "deg2", "collinear", "octahedron", "duplicate"):
        assert others[c.rows[lab]], lab
    assert separated[c.rows["deg257"]] and int(separated.sum()) > 40


def test_from_moments_bwd_constant_degree_and_two_rows():
    """a replaced std (the constant degree column; with two degree-1 rows also d_var and the eigenvalues) carries no gradient; with Q = 2 every
    column that keeps its std has a zero adjoint (two z-scored values are +-0.707 wherever the inputs are), so the replaced d_var column is
    what reaches the moments: columns Sd and Sd2.  (A generic two-row graph has no replaced column and hence an adjoint that is zero up to
    round-off, with no peak to hold an error against: the two rows here are the Q = 2 graph whose adjoint is not.)"""
    _from_moments_bwd_case("const_degree", prepare(R.degree_graph((8,), 40)))
    c = prepare(R.degree_graph((1,), 2))
    assert R.column_stats(c.raw)[2][2]
    _from_moments_bwd_case("q2", c, common_too=False)


def test_moments_bwd(case):
    c = case
    adj64 = torch.randn(c.num_q, 12, dtype=torch.float64, generator=torch.Generator().manual_seed(31))
    ge, gq = twice(k_moments_bwd, c.d_src, c.d_qry, c.g, adj64.to(DEV))
    assert not torch.isnan(ge).any() and not torch.isnan(gq).any()
    key, other = c.g.by_dst.key.cpu().long(), c.g.by_dst.other.cpu().long()
    u = (c.src.double()[other] - c.qry.double()[key]).requires_grad_()
    (ge_ref,) = torch.autograd.grad((R.edge_moments(u, key, c.num_q) * adj64).sum(), [u])
    q = c.qry.double().clone().requires_grad_()
    (gq_ref,) = torch.autograd.grad((R.moments(c.src, q, c.ei) * adj64).sum(), [q])
    cg.check(f"geoembed_stat/moments_bwd/{c.tag} per-edge gradient", ge, ge_ref, FP32_BAR)
    cg.check(f"geoembed_stat/moments_bwd/{c.tag} query gradient", gq, gq_ref, FP32_BAR)
    # the coincident edge: d|u|/du = 0 at u = 0 as torch.norm's backward, so the distance adjoint contributes exactly nothing
    e = ((u.detach() == 0).all(1)).nonzero().reshape(-1)
    assert e.numel() == 1 and int(key[e]) == c.rows["coincident"]
    assert torch.equal(ge.cpu()[e[0]], adj64[c.rows["coincident"], 3:6].float())
    assert not gq.cpu()[c.mom[:, 0] == 0].any()                                                  # empty rows


def test_geostatfn_end_to_end_on_the_rank_deficient_rows():
    from gaot_3d_amd.model.layers.geoembed import GeoStatFn
    c = prepare(R.case_graph())
    ref, r = cg.oracle_grads(lambda s, q: orc.geoembed_stat_features(s, q, c.ei), (c.src, c.qry), (0, 1))
    got = cg.product_grads(lambda s, q: GeoStatFn.apply(s, q, c.g), (c.src, c.qry), (0, 1), r)
    again = cg.product_grads(lambda s, q: GeoStatFn.apply(s, q, c.g), (c.src, c.qry), (0, 1), r)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()                          # the isotropic row included
    keep_s, keep_q = torch.ones(c.num_src, dtype=torch.bool), torch.ones(c.num_q, dtype=torch.bool)
    keep_s[c.sources["octahedron"]] = False
    keep_q[c.rows["octahedron"]] = False
    cg.check("geoembed_stat/GeoStatFn d/dsource (isotropic row excluded)", got[0].cpu()[keep_s], ref[0][keep_s], FP32_BAR)
    cg.check("geoembed_stat/GeoStatFn d/dquery (isotropic row excluded)", got[1].cpu()[keep_q], ref[1][keep_q], FP32_BAR)
    for lab in ("deg1", "deg2", "deg3", "collinear", "coplanar", "duplicate", "jittered_line"):
        s, q = c.sources[lab], c.rows[lab]
        cg.check(f"geoembed_stat/GeoStatFn {lab} row: d/d its sources and its query", torch.cat([got[0].cpu()[s], got[1].cpu()[q:q + 1]]),
                 torch.cat([ref[0][s], ref[1][q:q + 1]]), FP32_BAR)


# ---- host: the feature cache of GeometricEmbedding.forward -------------------------------------------------------------------------------
def test_feature_cache_of_the_module():
    from gaot_3d_amd.model.layers.geoembed import GeometricEmbedding, GeoStatFn
    _, ops = _lib_ops()
    c = R.case_graph()
    torch.manual_seed(3)
    ge = GeometricEmbedding(3, 32).to(DEV)
    src, qry, eid = c.src.to(DEV), c.qry.to(DEV), c.ei.to(DEV)
    g = ops.build_graph(eid, c.num_src, c.num_q)

    def call(s, q, graph=g, module=ge):
        torch.cuda.synchronize()
        n0 = ops.launch_count()
        out = module(s, q, eid, graph=graph)
        return out, ops.launch_count() - n0

    def fresh(s, q):
        """a new module with the same weights on new neighbour lists: nothing cached"""
        m = GeometricEmbedding(3, 32).to(DEV)
        m.load_state_dict(ge.state_dict())
        return call(s.clone(), q.clone(), ops.build_graph(eid, c.num_src, c.num_q), m)[0]

    n0 = ops.launch_count()
    ops.geoembed_from_moments(ops.geoembed_moments(src, qry, g))
    n_feats = ops.launch_count() - n0
    assert n_feats >= 2
    first, n_first = call(src, qry)
    ent = g.__dict__["_geo_feats"]
    second, n_second = call(src, qry)
    assert n_second == n_first - n_feats and g.__dict__["_geo_feats"] is ent                     # nothing launched for the features
    assert torch.equal(first, second)
    for moved in (src, qry):                                                                     # in place: the version moves on
        moved.add_(0.015625)
        out, n = call(src, qry)
        assert n == n_first and not torch.equal(out, first)
        assert torch.equal(out, fresh(src, qry))
        assert call(src, qry)[1] == n_first - n_feats
    for s, q in ((src.clone(), qry), (src, qry.clone())):                                         # another tensor object, equal values
        call(src, qry)
        before = call(src, qry)
        assert before[1] == n_first - n_feats
        out, n = call(s, q)
        assert n == n_first and torch.equal(out, before[0])
        assert g.__dict__["_geo_feats"][0] is s and g.__dict__["_geo_feats"][2] is q
    call(src, qry)
    ent = g.__dict__["_geo_feats"]
    sg = src.clone().requires_grad_()                                                            # requires_grad: the cache is bypassed
    out, _ = call(sg, qry)
    assert g.__dict__["_geo_feats"] is ent and out.requires_grad
    assert torch.equal(GeoStatFn.apply(sg, qry, g).detach(), ent[4])                              # the same values on both paths
    assert call(src, qry)[1] == n_first - n_feats                                                # and the cached entry still serves
