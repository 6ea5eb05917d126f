"""The exact lattice reference (tests/graph_exact_ref.py) and the cases built on it, checked on the CPU: the reference agrees
with the brute-force oracle wherever the oracle can decide, the grids reproduce the lattice bit for bit, and the tie / boundary
cases the GPU tests (tests/test_graph_exact_gpu.py) rely on really contain what they are for.  Also the grid acceptance rule of
``graph.as_latent_grid`` ("Grid acceptance"): what must stay a grid stays one."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import graph_exact_ref as R  # noqa: E402
import graph_oracle as gorc  # noqa: E402  (checker only)

KNN_KS = (1, 2, 3, 5, 7, 8, 9, 12, 13, 16, 20, 24, 27, 32, 40, 48, 50, 64)      # the register path of the GPU tests
TIE_GRIDS = ("c5", "a953", "c6")
MIN_TIE_SHARE = 0.4          # of all rows, for every k above: the k-th and (k+1)-th nearest tokens at the same distance


@pytest.mark.parametrize("name", sorted(R.LATTICE_GRIDS))
def test_grids_reproduce_the_lattice_bit_for_bit(name):
    """data.latent_grid (torch.linspace in fp32) returns exactly integers / 8, and the device-side grid test accepts them"""
    from gaot_3d_amd import graph
    from gaot_3d_amd.data import latent_grid
    dims, (lo, hi), t, q, kind = R.lattice_case(name)
    lat = latent_grid(dims, lo, hi)
    assert lat.dtype == torch.float32 and torch.equal(lat, R.to_float(t))
    assert torch.equal(R.to_float(q).double() * R.SCALE, q.double())
    assert q.shape[0] <= 4000 and t.shape[0] <= 729
    g = graph.as_latent_grid(lat, dims)
    assert g.lo == lo and g.hi == hi


def test_case_kinds_and_outside_points():
    for name in TIE_GRIDS:
        dims, _, t, q, kind = R.lattice_case(name)
        for kd in range(5):
            assert int((kind == kd).sum()) >= 6, (name, kd)
    dims, lo, step = R.LATTICE_GRIDS["s5"]
    q = R.lattice_case("s5")[3]
    assert R.max_cells_outside(q, dims, lo, step) == 12
    for a in range(3):       # 12 cells outside on both sides of every axis
        assert int(q[:, a].min()) == lo[a] - 12 * step[a] and int(q[:, a].max()) == lo[a] + (dims[a] - 1 + 12) * step[a]
    dims, lo, step = R.LATTICE_GRIDS["an17"]
    assert max(step) // min(step) >= 16


def _oracle_tokens(which):
    if which == "grid":      # odd, unequal steps: few symmetric ties
        return R.grid_ints((3, 4, 5), (-16, -15, -14), (13, 9, 7)), 2
    g = torch.Generator().manual_seed(1)
    return torch.unique(torch.randint(-R.LIMIT, R.LIMIT + 1, (30, 3), generator=g), dim=0), 3


@pytest.mark.parametrize("which", ["grid", "scattered"])
def test_reference_agrees_with_oracle_where_there_is_no_tie(which):
    """random lattice queries against lattice tokens with few symmetric ties (a grid with odd, unequal steps; scattered tokens): on
    rows whose first k + 1 distances are all different the oracle's fp64 brute force decides, and the integer reference returns
    the same lists"""
    t, k = _oracle_tokens(which)
    g = torch.Generator().manual_seed(7)
    q = torch.randint(-R.LIMIT, R.LIMIT + 1, (600, 3), generator=g)
    tf, qf = R.to_float(t), R.to_float(q)
    s = torch.sort(R.d2(q, t), dim=1).values[:, : k + 1]
    clear = (s[:, 1:] != s[:, :-1]).all(dim=1)
    assert float(clear.float().mean()) >= 0.9, float(clear.float().mean())
    ref = gorc.knn(qf, tf, k)[1].view(-1, k)
    assert torch.equal(R.knn(q, t, k)[clear], ref[clear])
    # radius: a threshold no squared distance attains (integer + 1/2), so no row has d == r and every row qualifies
    for r2 in (40, 150):
        assert not bool((R.d2(q, t) * 2 == 2 * r2 + 1).any())
        r = (r2 + 0.5) ** 0.5 / R.SCALE
        for strategy in ("radius", "bidirectional", "reverse"):
            qq, kk = (q, k) if strategy == "radius" else (q[clear], k)
            assert torch.equal(R.decoder_edges(strategy, qq, t, r2, kk), gorc.decoder_edges(strategy, R.to_float(qq), tf, r, kk)), strategy
            if strategy != "reverse":
                assert torch.equal(R.encoder_edges(strategy, qq, t, r2, kk), gorc.encoder_edges(strategy, R.to_float(qq), tf, r, kk)), strategy
        rp, qi, tk = R.query_rows("bidirectional", q[clear], t, r2, k)
        by_query = gorc.decoder_edges("bidirectional", R.to_float(q[clear]), tf, r, k)
        order = torch.sort(by_query[1], stable=True).indices
        assert torch.equal(torch.stack([tk, qi]), by_query[:, order])
        assert torch.equal(rp[1:] - rp[:-1], torch.bincount(qi, minlength=int(clear.sum())))


@pytest.mark.parametrize("name", TIE_GRIDS)
def test_knn_cases_hold_ties_at_the_cut(name):
    _, _, t, q, kind = R.lattice_case(name)
    for k in KNN_KS:
        share = R.kth_tie_share(q, t, k)
        print(name, k, round(share, 3))
        assert share >= MIN_TIE_SHARE, (name, k, share)
    for k in (65, 100):
        assert R.kth_tie_share(q, t, k) >= MIN_TIE_SHARE, (name, k)


def test_multi_pass_boundary_falls_inside_a_tie_shell():
    """k > 64 runs in passes of 64 (k_knn_brute_pass): entry 64 must split a shell of equal distances, so that the next pass has
    to resume INSIDE a tie by token index"""
    _, _, t, q, kind = R.lattice_case("c5")
    centre = torch.tensor([0, 0, 0])
    assert R.shell_sizes(centre, t)[:7] == [1, 7, 19, 27, 33, 57, 81]
    inside = 0
    for name in TIE_GRIDS:
        _, _, t, q, kind = R.lattice_case(name)
        s = torch.sort(R.d2(q, t), dim=1).values
        split = s[:, 63] == s[:, 64]
        for kd in range(4):      # node, edge-midpoint, face-centre and cell-centre queries
            assert float(split[kind == kd].float().mean()) >= 0.25, (name, kd)
        if t.shape[0] > 128:
            assert float((s[:, 127] == s[:, 128]).float().mean()) >= 0.25, name
        inside += int(split.sum())
    assert inside > 1000


# (grid, 8 * radius): the radii of the GPU tests
RADIUS_CASES = (("c5", 1), ("c5", 4), ("c5", 6), ("c5", 12), ("a953", 2), ("a953", 6), ("a953", 10), ("c6", 3), ("c6", 5), ("c6", 8))


def test_radius_cases_hold_exact_hits_and_cut_ties():
    seen_cut = {"decoder": 0, "encoder": 0}
    for name, r8 in RADIUS_CASES:
        _, _, t, q, kind = R.lattice_case(name)
        d = R.d2(q, t)
        on = (d == r8 * r8).any(dim=1)
        if r8 > 1:
            assert float(on.float().mean()) >= 0.1, (name, r8)        # rows with a token at exactly d == r
        for dd, what in ((d, "decoder"), (d.t(), "encoder")):          # centres = queries / centres = tokens
            hit = dd <= r8 * r8
            cut = hit.sum(1) > R.CAP
            if not bool(cut.any()):
                continue
            # the cap cuts THROUGH a shell of equal distances: some candidate at a distance is kept, another at the same one dropped
            kept = hit & (torch.cumsum(hit.long(), dim=1) <= R.CAP)
            dropped = hit & ~kept
            has_kept = torch.zeros(dd.shape[0], r8 * r8 + 1, dtype=torch.bool)
            has_dropped = torch.zeros_like(has_kept)
            has_kept[kept.nonzero(as_tuple=True)[0], dd[kept]] = True
            has_dropped[dropped.nonzero(as_tuple=True)[0], dd[dropped]] = True
            tied = (has_kept & has_dropped).any(dim=1)
            assert not bool((tied & ~cut).any())
            print(name, r8, what, int(cut.sum()), int(tied.sum()))
            seen_cut[what] += int(tied.sum())
    assert seen_cut["decoder"] >= 50 and seen_cut["encoder"] >= 50, seen_cut
    counts = {(n, r): (R.d2(R.lattice_case(n)[3], R.lattice_case(n)[2]) <= r * r).sum(1) for n, r in RADIUS_CASES}
    assert any(bool((c == 0).any()) for c in counts.values())                    # empty rows
    assert any(bool(((c > 0) & (c <= R.CAP)).any()) for c in counts.values())    # partial rows
    assert any(bool((c > R.CAP).any()) for c in counts.values())                 # capped rows


UNION_KS = (2, 5, 9, 11, 12, 20, 24, 30, 32)


def test_union_cases_hold_disjoint_and_nested_rows():
    above = nested = 0
    for name, r8 in RADIUS_CASES:
        _, _, t, q, kind = R.lattice_case(name)
        c, o = R.radius(q, t, r8 * r8)
        member = torch.zeros(q.shape[0], t.shape[0], dtype=torch.bool)
        member[c, o] = True
        capped = (R.d2(q, t) <= r8 * r8).sum(1) > R.CAP
        top = torch.where(member, torch.arange(t.shape[0])[None], torch.full((1, 1), -1)).max(dim=1).values
        for k in UNION_KS:
            nn = R.knn(q, t, k)
            above += int((capped & (nn.min(dim=1).values > top)).sum())      # every knn token above the capped radius range
            nested += int(member.gather(1, nn).all(dim=1).sum())             # every knn token is a radius token as well
    assert above >= 20 and nested >= 200, (above, nested)


# ---- the grid acceptance rule ---------------------------------------------------------------------------------------------------
def test_full_size_grids_stay_grids():
    """the benchmark's and ``sample``'s grids keep the cell-lookup kernels: data.latent_grid at (64, 64, 32) and its fp32 rescaled
    copies onto shifted boxes are accepted"""
    from gaot_3d_amd import graph
    from gaot_3d_amd.data import latent_grid
    dims = (64, 64, 32)
    lat = latent_grid(dims)
    assert graph.as_latent_grid(lat, dims).dims == dims
    for lo, hi in (((-1.16, -1.2, 0.0), (4.21, 1.19, 1.77)), ((0.5, 0.5, 0.5), (2.5, 2.5, 2.5)), ((3.0, -7.0, 5.0), (5.0, -4.0, 6.0)),
                   ((100.0, 100.0, 100.0), (103.0, 103.0, 103.0))):
        lo, hi = torch.tensor(lo), torch.tensor(hi)
        moved = (lat + 1.0) / 2.0 * (hi - lo) + lo
        assert moved.dtype == torch.float32
        assert graph.as_latent_grid(moved, dims).num_tokens == lat.shape[0]


def test_acceptance_bound_is_in_units_of_the_smallest_step():
    from gaot_3d_amd import graph
    from gaot_3d_amd._lib import GaotError
    from gaot_3d_amd.data import latent_grid
    u = 2.0 ** -24
    for dims in ((9, 3, 3), (64, 64, 32), (256, 256, 256)):
        c = max(dims) - 1
        b = graph.grid_deviation_bound(dims)
        assert b == pytest.approx((1.5 - 5 * u * c) * (1e-4 - 8 * u) - 5 * u * c, rel=1e-12)
        assert 0 < b < 1.5e-4
    assert graph.grid_deviation_bound((502, 1, 1)) <= 0 < graph.grid_deviation_bound((500, 1, 1))
    # a strongly anisotropic grid: a deviation that is small against the span but not against the smallest step is refused
    dims = (17, 2, 2)
    lat = latent_grid(dims, (0.0, 0.0, 0.0), (1.0, 16.0, 16.0))
    assert graph.as_latent_grid(lat, dims).dims == dims
    tol = graph.grid_deviation_bound(dims) * (1.0 / 16)
    for frac, ok in ((0.9, True), (1.5, False)):
        bad = lat.clone()
        bad[5 * 4 + 1, 0] += frac * tol            # 1e-4 * span would be 1.6e-3: 170 x this amount
        if ok:
            graph.as_latent_grid(bad, dims)
        else:
            with pytest.raises(GaotError):
                graph.as_latent_grid(bad, dims)
    # 256 nodes per axis far from the origin: fp32 cannot hold the nodes to the bound -> not a grid (brute-force route)
    far = (latent_grid((256, 2, 2)) + 1.0) / 2.0 * 3.0 + 100.0
    with pytest.raises(GaotError):
        graph.as_latent_grid(far, (256, 2, 2))
    with pytest.raises(GaotError):
        graph.as_latent_grid(latent_grid((502, 1, 1)), (502, 1, 1))


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("side", [-1, 1])
@pytest.mark.parametrize("w", [1, 2])
def test_perturbed_grids_are_accepted_and_decidable(axis, side, w):
    """the window-edge family of the GPU tests: the moved token is accepted at 0.99 of the bound and refused at 1.5 of it, truly
    displaces the nominal k-th neighbour, and the two competing squared distances are >= 16 fp32 spacings apart"""
    from gaot_3d_amd import graph
    from gaot_3d_amd._lib import GaotError
    dims = tuple(9 if a == axis else 3 for a in range(3))
    tol = graph.grid_deviation_bound(dims) * 0.25
    dims2, tok, q, k, moved, kth = R.perturbed_case(axis, side, w, tol)
    assert dims2 == dims and k == 2 * w + 1
    graph.as_latent_grid(tok, dims)
    ids, ds = R.knn_fp64(q, tok, k)
    assert moved in ids[0].tolist() and kth not in ids[0].tolist()
    nominal = R.perturbed_case(axis, side, w, tol, frac=0.0)
    ids0, _ = R.knn_fp64(q, nominal[1], k)
    assert kth in ids0[0].tolist() and moved not in ids0[0].tolist()
    for row in range(2):
        gap = R.ulps_apart(float(ds[row, k - 1]), float(ds[row, k]))
        print(axis, side, w, row, gap)
        assert gap >= 16
    with pytest.raises(GaotError):
        graph.as_latent_grid(R.perturbed_case(axis, side, w, tol, frac=1.5)[1], dims)
