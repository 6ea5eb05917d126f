"""The fp64 stage reference of the statistical GeoEmbed features (tests/geoembed_stat_ref.py) held to account without a GPU:
(a) its composition equals the oracle's restatement of geoembed.py:99-182 evaluated in fp64, (b) its two forms of the raw features agree,
(c) an fp32 emulation of the kernels' documented rounding points stays within half of every asserted bound (the bounds are not
vacuous, and the reference alone passes them), (d) its fp64 autograd agrees with central finite differences in every coordinate of
the case graph except the isotropic row's (whose eigenvalue adjoint depends on the eigenbasis)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
import gaot_oracle as orc  # noqa: E402
import geoembed_stat_ref as R  # noqa: E402

OFFSETS = (0.0, 100.0)


@pytest.fixture(scope="module", params=OFFSETS, ids=["offset0", "offset100"])
def case(request):
    c = R.case_graph(offset=request.param)
    c.mom = R.moments(c.src, c.qry, c.ei)
    c.raw = R.raw_from_moments(c.mom)
    return c


def test_case_graph_holds_the_rows_it_promises():
    c = R.case_graph()
    deg = torch.bincount(c.ei[1], minlength=c.num_q)
    for d in R.DEGREES:
        assert int(deg[c.rows[f"deg{d}"]]) == d
    for lab, d in zip(R.CRAFTED, (5, 6, 6, 5, 12, 4)):
        assert int(deg[c.rows[lab]]) == d, lab
    raw = R.raw_from_moments(R.moments(c.src, c.qry, c.ei))
    lam = raw[:, 6:9]
    assert torch.equal(lam[c.rows["octahedron"]], torch.full((3,), 0.25 ** 2 / 3 + 1e-6, dtype=torch.float64))     # isotropic, exactly
    assert torch.equal(lam[c.rows["duplicate"]], torch.full((3,), 1e-6, dtype=torch.float64)) and raw[c.rows["duplicate"], 2] == 0
    assert lam[c.rows["collinear"], 1] < 1.001e-6 < 0.05 < lam[c.rows["collinear"], 0]                               # rank 1
    assert lam[c.rows["coplanar"], 2] < 1.001e-6 and lam[c.rows["coplanar"], 1] > 1e-3                               # rank 2
    assert lam[c.rows["jittered_line"], 0] / (lam[c.rows["jittered_line"], 1] - 1e-6) > 1e6
    e = (c.ei[1] == c.rows["coincident"]).nonzero().reshape(-1)
    assert int((c.src[c.ei[0, e]] == c.qry[c.rows["coincident"]]).all(1).sum()) == 1                                # distance exactly 0
    heavy = torch.tensor([c.rows[f"deg{d}"] for d in R.DEGREES if d >= 31])
    assert len(set((heavy // 32).tolist())) > 1                    # the heavy rows do not share one 32-row block
    c100, c3 = R.case_graph(offset=100.0), R.case_graph(tile=3)
    assert torch.equal(c100.ei, c.ei) and c100.src.min() > 98.0
    assert c3.num_q == 3 * c.num_q and c3.ei.shape[1] == 3 * c.ei.shape[1] and c3.rows == c.rows


def test_a_composition_equals_the_oracle_in_fp64(case):
    got = R.zscore(case.raw)
    ref = orc.geoembed_stat_features(case.src.double(), case.qry.double(), case.ei)
    for col in range(R.NF):
        err = (got[:, col] - ref[:, col]).abs().max().item()
        peak = ref[:, col].abs().max().item()
        print(f"[parity] geoembed_stat_ref/oracle col{col}: max_abs={err:.3e} rel_to_peak={err / peak:.3e}")
        assert err <= 1e-12 * peak, (col, err, peak)
    assert torch.equal(R.features_from_moments(case.mom), got)


def test_b_two_sweep_equals_from_moments(case):
    two = R.raw_two_sweep(case.src, case.qry, case.ei)
    for col in range(R.NF):
        err = (two[:, col] - case.raw[:, col]).abs().max().item()
        peak = case.raw[:, col].abs().max().item()
        print(f"[parity] geoembed_stat_ref/two_sweep col{col}: max_abs={err:.3e} rel_to_peak={err / peak:.3e}")
        assert err <= 1e-12 * peak, (col, err, peak)
    empty = case.mom[:, 0] == 0
    assert int(empty.sum()) >= 2 and not two[empty].any() and not case.raw[empty].any()
    sums = R.column_sums(case.raw)
    assert torch.allclose(R.zscore(case.raw, case.num_q, sums), R.zscore(case.raw), rtol=0, atol=1e-11)


def test_c_fp32_emulation_stays_within_half_of_every_bound(case):
    draw = R.rounding_bound_raw(case.raw, case.mom)
    dz = R.rounding_bound_zscore(case.raw, draw)
    x32, y32 = R.emulate_fp32(case.raw)
    r_raw = R.ratio((x32.double() - case.raw).abs(), draw).max(0).values
    r_z = R.ratio((y32.double() - R.zscore(case.raw)).abs(), dz).max(0).values
    print(f"[parity] geoembed_stat_ref/emulation worst error / asserted bound: raw {r_raw.max().item():.3f} "
          f"per column {[round(v, 3) for v in r_raw.tolist()]}; z-score {r_z.max().item():.3f} per column {[round(v, 3) for v in r_z.tolist()]}")
    assert torch.isfinite(dz).all() and (dz > 0).all()
    assert r_raw.max().item() <= 0.5 and r_z.max().item() <= 0.5
    # a stage bound is no wider than the project's outer bar (5e-5 of the column's peak) allows
    assert (R.FACTOR * dz).max(0).values.div(R.zscore(case.raw).abs().max(0).values).max().item() < 5e-5


def test_d_autograd_agrees_with_central_differences():
    """every coordinate of every source and query except the isotropic row and its six sources; fp64, h = 1e-6: the truncation
    h^2 f''' / 6 (f''' is largest where a null-space eigenvalue bends: the collinear row) and the round-off 2^-53 |f| / h stay below 1e-7 of the
    gradient's peak here; asserted at 1e-6 of the peak, over all coordinates and again on each rank-deficient row by itself"""
    c = R.case_graph()
    gy = torch.randn(c.num_q, R.NF, dtype=torch.float64, generator=torch.Generator().manual_seed(7))

    def loss(s, q):
        return (R.features_from_moments(R.moments(s, q, c.ei)) * gy).sum()

    s0, q0 = c.src.double(), c.qry.double()
    s, q = s0.clone().requires_grad_(), q0.clone().requires_grad_()
    gs, gq = torch.autograd.grad(loss(s, q), [s, q])
    assert torch.isfinite(gs).all() and torch.isfinite(gq).all()
    h = 1e-6
    keep_s = torch.ones(c.num_src, dtype=torch.bool)
    keep_s[c.sources["octahedron"]] = False
    keep_q = torch.ones(c.num_q, dtype=torch.bool)
    keep_q[c.rows["octahedron"]] = False
    with torch.no_grad():
        def fd(which, n, keep):
            out = torch.zeros(n, 3, dtype=torch.float64)
            for i in keep.nonzero().reshape(-1).tolist():
                for k in range(3):
                    a, b = (s0.clone(), q0.clone()), (s0.clone(), q0.clone())
                    a[which][i, k] += h
                    b[which][i, k] -= h
                    out[i, k] = (loss(*a) - loss(*b)) / (2 * h)
            return out
        fs, fq = fd(0, c.num_src, keep_s), fd(1, c.num_q, keep_q)
    for name, g, f, keep in (("source", gs, fs, keep_s), ("query", gq, fq, keep_q)):
        err = (g - f)[keep].abs().max().item()
        peak = g[keep].abs().max().item()
        print(f"[parity] geoembed_stat_ref/finite_differences d/d{name}: max_abs={err:.3e} rel_to_peak={err / peak:.3e} peak={peak:.3e}")
        assert err <= 1e-6 * peak, (name, err, peak)
    for lab in ("deg1", "deg2", "deg3", "collinear", "coplanar", "duplicate", "jittered_line", "coincident"):
        rows_s = c.sources[lab]
        err = max((gs - fs)[rows_s].abs().max().item(), (gq - fq)[c.rows[lab]].abs().max().item())
        peak = max(gs[rows_s].abs().max().item(), gq[c.rows[lab]].abs().max().item())
        print(f"[parity] geoembed_stat_ref/finite_differences {lab}: max_abs={err:.3e} rel_to_peak={err / peak:.3e}")
        assert peak > 0 and err <= 1e-6 * peak, (lab, err, peak)
