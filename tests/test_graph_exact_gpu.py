"""The neighbour search (csrc/graph.hip, csrc/csr_impl.h through gaot_3d_amd/graph.py and ops.csr_build) at exact ties, window
edges and scan / sort boundaries, against references that share no code with it: the int64 lattice reference of
tests/graph_exact_ref.py (coordinates are integers / 8, so fp32 distances are exact and true ties are device ties), fp64 brute
force on the stored coordinates for grids off the lattice, torch.cumsum and torch.sort for the integer machinery.  Every list is
compared with ``torch.equal``; no test compares two device routes with each other.  What the cases contain (tie shares, d == r,
cap cuts through ties, the 64-entry pass boundary inside a shell, decidable perturbations) is asserted on the CPU in
tests/test_graph_exact_cpu.py."""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import graph_exact_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

KNN_KS = (1, 2, 3, 5, 7, 8, 9, 12, 13, 16, 20, 24, 27, 32, 40, 48, 50, 64)     # every register capacity at kout == K and kout < K
MANY_KS = (65, 100, 128)                                                        # passes of 64
UNION_KS = (2, 5, 9, 11, 12, 20, 24, 30, 32)
RADIUS_CASES = (("c5", 1), ("c5", 4), ("c5", 6), ("c5", 12), ("a953", 2), ("a953", 6), ("a953", 10), ("c6", 3), ("c6", 5), ("c6", 8))
FAMILIES = ("grid", "brute")


@functools.lru_cache(maxsize=None)
def _case(name):
    return R.lattice_case(name)


@functools.lru_cache(maxsize=None)
def _order(name):
    """the full (distance, index) order of every query's tokens: computed once, every k is a prefix of it"""
    _, _, t, q, _ = _case(name)
    return R.knn(q, t, t.shape[0])


def _device(name, family):
    from gaot_3d_amd import graph
    from gaot_3d_amd.data import latent_grid
    dims, (lo, hi), t, q, _ = _case(name)
    lat = latent_grid(dims, lo, hi)
    assert torch.equal(lat, R.to_float(t))
    lat = lat.to(DEV)
    return R.to_float(q).to(DEV), (graph.as_latent_grid(lat, dims) if family == "grid" else graph.TokenSet(lat))


def _check_rows(got, rowptr, qi, tk, what):
    assert got.by_src is None and got.by_dst.perm is None
    assert torch.equal(got.by_dst.rowptr.cpu().long(), rowptr), what
    assert torch.equal(got.by_dst.key.cpu().long(), qi), what
    assert torch.equal(got.by_dst.other.cpu().long(), tk), what


# ---- a. kNN order and ties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", ["c5", "a953", "c6"])
def test_knn_order_at_ties(name, family):
    """knn_to_grid returns exactly the reference row, in (distance, token index) order, for every register capacity (k equal to
    it and below it), for two and three passes of 64 and for k == number of tokens"""
    from gaot_3d_amd import graph
    p, g = _device(name, family)
    m = g.num_tokens
    for k in KNN_KS + MANY_KS + (m,):
        if k > m:
            continue
        got = graph.knn_to_grid(p, g, k)
        assert got.dtype == torch.int32 and got.shape == (p.shape[0], k)
        assert torch.equal(got.cpu().long(), _order(name)[:, :k]), (name, family, k)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name,k", [("t2", 8), ("t4", 64), ("t4", 63), ("t2", 7)])
def test_knn_all_tokens_on_the_register_path(name, k, family):
    """k == number of tokens (and one less) at a register capacity: the window has to grow to the whole grid"""
    from gaot_3d_amd import graph
    p, g = _device(name, family)
    assert torch.equal(graph.knn_to_grid(p, g, k).cpu().long(), _order(name)[:, :k])


# ---- b. radius and the strategies at ties -----------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name,r8", RADIUS_CASES)
def test_strategy_edges_at_ties(name, r8, family):
    """encoder and decoder edge lists of 'radius', 'bidirectional' and 'reverse' with tokens at exactly d == r and caps that cut
    through shells of equal distance, both kernel families"""
    from gaot_3d_amd import graph
    _, _, t, q, _ = _case(name)
    p, g = _device(name, family)
    r, k = r8 / R.SCALE, 3
    for strategy in ("radius", "bidirectional"):
        got = graph._encoder_edges(strategy, p, g, r, k)
        assert got.dtype == torch.int32
        assert torch.equal(got.cpu().long(), R.encoder_edges(strategy, q, t, r8 * r8, k)), ("encoder", strategy)
    for strategy in ("radius", "bidirectional", "reverse"):
        got = graph._decoder_edges(strategy, p, g, r, k)
        assert torch.equal(got.cpu().long(), R.decoder_edges(strategy, q, t, r8 * r8, k)), ("decoder", strategy)


# ---- c. the per-query union at every register capacity -------------------------------------------------------------------------
@pytest.mark.parametrize("name,r8", RADIUS_CASES)
def test_query_lists_union_capacities(name, r8):
    """graph.query_lists('bidirectional') against the reference's per-query definition: padded register lists (k below the
    capacities 12, 24, 32), empty / partial / capped radius rows, knn tokens all above the capped radius range and knn tokens all
    inside the radius set (tests/test_graph_exact_cpu.py asserts the cases hold them)"""
    from gaot_3d_amd import graph
    _, _, t, q, _ = _case(name)
    p, g = _device(name, "grid")
    r = r8 / R.SCALE
    _check_rows(graph.query_lists("radius", p, g, r, 1), *R.query_rows("radius", q, t, r8 * r8, 1), ("radius", name, r8))
    for k in UNION_KS:
        _check_rows(graph.query_lists("bidirectional", p, g, r, k), *R.query_rows("bidirectional", q, t, r8 * r8, k), (name, r8, k))


# ---- d. window edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", ["s5", "an17", "d1xx", "dx1x", "dxx1", "one"])
def test_window_edges_on_the_lattice(name, family):
    """points up to 12 cells outside the box, a grid with step ratio 16, one node along an axis (each position) and a one-token
    grid: knn, radius pairs (capped and not) and the per-query union"""
    from gaot_3d_amd import graph
    _, _, t, q, _ = _case(name)
    p, g = _device(name, family)
    m = t.shape[0]
    for k in (1, 2, 3, 5, 8, 12, 16, 25, 32, 64, 68, 100, m):
        if k <= m:
            assert torch.equal(graph.knn_to_grid(p, g, k).cpu().long(), _order(name)[:, :k]), (name, family, k)
    for r8 in (1, 2, 5, 16, 24):
        for cap in (None, R.CAP, 3):
            pt, tk = graph.radius_pairs(p, g, r8 / R.SCALE, cap)
            c, o = R.radius(q, t, r8 * r8, cap)
            assert torch.equal(pt.cpu().long(), c) and torch.equal(tk.cpu().long(), o), (name, family, r8, cap)
        if family == "grid":
            for k in (1, 2, 11, 24):
                if k <= m:
                    _check_rows(graph.query_lists("bidirectional", p, g, r8 / R.SCALE, k),
                                *R.query_rows("bidirectional", q, t, r8 * r8, k), (name, r8, k))


def _row_sets(idx):
    return torch.sort(idx.cpu().long(), dim=1).values


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("side", [-1, 1])
@pytest.mark.parametrize("w", [1, 2])
def test_window_proof_holds_for_every_accepted_grid(axis, side, w):
    """A grid off the lattice: the first token the window of half-width w excludes is moved inward by 0.99 of the deviation
    ``as_latent_grid`` accepts and truly displaces the nominal k-th neighbour (by half that amount; >= 16 fp32 spacings, asserted
    on the CPU).  The device result must equal fp64 brute force on the stored coordinates.  At 1.5 x the accepted deviation the
    token set is no grid any more and ``get_neighbor_strategy`` answers through the brute-force kernels -- the same reference."""
    from gaot_3d_amd import graph
    from gaot_3d_amd._lib import GaotError
    dims = tuple(9 if a == axis else 3 for a in range(3))
    tol = graph.grid_deviation_bound(dims) * 0.25
    _, tok, q, k, moved, kth = R.perturbed_case(axis, side, w, tol)
    ref, _ = R.knn_fp64(q, tok, k)
    assert moved in ref[0].tolist() and kth not in ref[0].tolist()
    g = graph.as_latent_grid(tok.to(DEV), dims)
    got = graph.knn_to_grid(q.to(DEV), g, k)
    print("device", got.cpu().tolist(), "reference", ref.tolist())
    assert torch.equal(_row_sets(got), _row_sets(ref))
    _, tok, q, k, moved, kth = R.perturbed_case(axis, side, w, tol, frac=1.5)
    ref, _ = R.knn_fp64(q, tok, k)
    assert moved in ref[0].tolist()
    with pytest.raises(GaotError):
        graph.as_latent_grid(tok.to(DEV), dims)
    e = graph.get_neighbor_strategy("knn", q.to(DEV), None, tok.to(DEV), None, 0.1, k, False, latent_dims=dims)
    assert torch.equal(e[0].cpu().long(), torch.arange(2).repeat_interleave(k))
    assert torch.equal(_row_sets(e[1].view(2, k)), _row_sets(ref))


def test_grid_beyond_fp32_resolution_takes_the_brute_force_route():
    """256 nodes on [100, 103]: fp32 holds the nodes to 6.5e-4 of a step only, beyond the window's slack, so the token set is no
    grid; get_neighbor_strategy still returns the reference edges (fp64 brute force on the stored coordinates; the queries sit
    0.3 of a step from a node, every distance involved is separated by 0.4 of a step)"""
    from gaot_3d_amd import graph
    from gaot_3d_amd._lib import GaotError
    from gaot_3d_amd.data import latent_grid
    dims = (256, 1, 1)
    tok = (latent_grid(dims, (-1.0, 0.0, 0.0), (1.0, 0.0, 0.0)) + 1.0) / 2.0 * 3.0 + 100.0
    with pytest.raises(GaotError):
        graph.as_latent_grid(tok.to(DEV), dims)
    step = 3.0 / 255
    q = tok[::5].clone()
    q[:, 0] += 0.3 * step
    k = 3
    ref, ds = R.knn_fp64(q, tok, k + 1)
    assert float(((ds[:, 1:k + 1] - ds[:, :k]) / ds[:, 1:k + 1]).min()) > 0.05       # decidable in fp32
    e = graph.get_neighbor_strategy("knn", q.to(DEV), None, tok.to(DEV), None, 0.1, k, False, latent_dims=dims)
    assert torch.equal(e[1].view(-1, k).cpu().long(), ref[:, :k])
    r = 1.5 * step
    d = ((q.double()[:, None] - tok.double()[None]) ** 2).sum(-1)
    assert float(((d - r * r).abs() / (r * r)).min()) > 0.05
    c, o = torch.nonzero(d <= r * r, as_tuple=True)
    e = graph.get_neighbor_strategy("radius", q.to(DEV), None, tok.to(DEV), None, r, k, True, latent_dims=dims)
    assert torch.equal(e.cpu().long(), torch.stack([o, c]))


# ---- e. the exclusive scan -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2047, 2048, 2049, 524_287, 524_288, 524_289, 1_048_583])
def test_exclusive_scan(n):
    """one, two and 257+ block sums (the carry loop of k_scan_blocksums starts beyond 256 tiles of 2048 = 524 288 entries)"""
    from gaot_3d_amd import graph
    g = torch.Generator().manual_seed(n)
    inputs = {"random": torch.randint(0, 41, (n,), generator=g, dtype=torch.int32), "zeros": torch.zeros(n, dtype=torch.int32),
              "ones": torch.ones(n, dtype=torch.int32)}
    if n:
        first, last = torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)
        first[0], last[-1] = 7, 9
        inputs.update(first=first, last=last)
    for what, x in inputs.items():
        got = graph.exclusive_scan(x.to(DEV))
        want = torch.zeros(n + 1, dtype=torch.int64)
        want[1:] = torch.cumsum(x.long(), 0)
        assert got.dtype == torch.int32 and got.shape == (n + 1,)
        assert torch.equal(got.cpu().long(), want), (n, what)


# ---- f. the sort at tile edges -------------------------------------------------------------------------------------------------------
def _keys(pattern, e, q):
    i = torch.arange(e, dtype=torch.int64)
    if pattern == "equal_low":
        return torch.zeros(e, dtype=torch.int64)
    if pattern == "equal_high":
        return torch.full((e,), q - 1, dtype=torch.int64)
    up = i if q >= e else i * q // e          # strictly ascending where the rows allow it, otherwise runs of equal keys
    if pattern == "sorted":
        return up
    assert pattern == "descending"
    return up.flip(0)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("pattern", ["equal_low", "equal_high", "descending", "sorted"])
def test_csr_build_at_tile_edges(pattern, dtype):
    """ops.csr_build with E on either side of one and two sort tiles (4096 keys), all-equal, descending (strictly wherever
    Q >= E) and already sorted keys, 1 to 65 537 rows: the assertions of test_csr_build"""
    from gaot_3d_amd import ops
    for q in (1, 2, 256, 257, 65_536, 65_537):
        for e in (4095, 4096, 4097, 8192, 8193):
            key = _keys(pattern, e, q)
            if pattern == "descending" and q >= e:
                assert bool((key[1:] < key[:-1]).all())
            other = (torch.arange(e, dtype=torch.int64) * 7919) % 100_003
            ei = torch.stack([other, key]).to(dtype)
            s = ops.csr_build(ei.to(DEV), 1, q)
            order = torch.sort(key, stable=True).indices
            rowptr = torch.zeros(q + 1, dtype=torch.long)
            rowptr[1:] = torch.cumsum(torch.bincount(key, minlength=q), 0)
            assert torch.equal(s.rowptr.cpu().long(), rowptr), (q, e)
            assert torch.equal(s.perm.cpu().long(), order), (q, e)
            assert torch.equal(s.key.cpu().long(), key[order]), (q, e)
            assert torch.equal(s.other.cpu().long(), other[order]), (q, e)


# ---- g. query counts around one block ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_query_counts_around_one_block(n):
    from gaot_3d_amd import graph
    _, _, t, q, _ = _case("c5")
    p, g = _device("c5", "grid")
    sel = torch.arange(n) * 2                     # nodes, midpoints and centres alike
    q, p = q[sel], p[sel.to(DEV)]
    for fam in (g, graph.TokenSet(g.pos)):
        for k in (5, 70):
            got = graph.knn_to_grid(p, fam, k)
            assert got.shape == (n, k) and torch.equal(got.cpu().long(), _order("c5")[sel, :k])
        for r8, cap in ((6, R.CAP), (12, R.CAP), (6, None)):
            pt, tk = graph.radius_pairs(p, fam, r8 / R.SCALE, cap)
            c, o = R.radius(q, t, r8 * r8, cap)
            assert torch.equal(pt.cpu().long(), c) and torch.equal(tk.cpu().long(), o)
    for strategy, k in (("radius", 1), ("bidirectional", 5), ("bidirectional", 11)):
        _check_rows(graph.query_lists(strategy, p, g, 0.75, k), *R.query_rows(strategy, q, t, 36, k), (strategy, k, n))
