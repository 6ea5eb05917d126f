"""CPU: the rounding model of tests/gno_ref.py and its acceptance rule (Report.model of tests/block_ref.py) have teeth.

  * the restated GELU coefficients are those of csrc/common.h;
  * the model with rounding switched off and erf-GELU is the pinned oracle (oracle/gaot_oracle.py) and its autograd, to 1e-12;
  * the condition on the inputs: on every small case of tests/test_gno_bf16_fp64_gpu.py the three fp32 realisations F sit within
    1/12 (rms) and 2/3 (max) of the yardstick R - E (the large cases: profiles/gno_bf16_fp64_parity.txt, `python tests/gno_ref.py`);
  * an undamaged F passes the rule, and each fault a kernel could have without today's tolerances noticing is rejected: a tile
    whose last edge never reaches a sum, a mean over deg + 1, a bias dropped for one hidden unit, truncation for rounding, 1/deg
    applied twice, the coordinates of one tile swapped in dW_0, and no rounding at all.

What the rule cannot see: anything below about a quarter of the model's own bf16 error spread over a whole tensor -- erf for the
polynomial GELU (9e-6 absolute on h), f16 round-to-nearest for round-toward-zero on G' (2^-12 relative, one-sided, on a factor of
dz), another order of the fp32 sums, a fault confined to a query row of thousands of edges whose mean averages it away (the mean
over deg + 1 is caught on a row of typical degree, not on the 2000-edge row), and a fault in a tensor element whose own error is
far below the tensor's largest."""
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
import block_ref as B  # noqa: E402
import gno_ref as G  # noqa: E402
import gaot_oracle as orc  # noqa: E402  (checker only)


def test_gelu_coefficients_match_common_h():
    text = open(os.path.join(HERE, "..", "gaot_3d_amd", "csrc", "common.h")).read()
    num = r"(-?[0-9]+\.?[0-9]*(?:[eE][-+]?[0-9]+)?)f?\b"
    assert float(re.search(r"GELU_A_MAX\s*=\s*" + num, text).group(1)) == G.GELU_A_MAX
    for k in range(5):
        assert float(re.search(rf"GELU_P{k}\s*=\s*" + num, text).group(1)) == G.GELU_P[k], k
    for k in range(1, 5):    # Q_k = ln 2 * k * P_k, written out in the header with the same literals
        m = re.search(rf"GELU_Q{k}\s*=\s*\(float\)\(\s*{num}\s*\*\s*{num}\s*\*\s*{num}\s*\)", text)
        assert [float(v) for v in m.groups()] == [0.6931471805599453, float(k), G.GELU_P[k]], k
    # the restated function against erf-GELU: the header's 9.3e-6 / 3.7e-5
    x = torch.linspace(-12, 12, 48001, dtype=torch.float64)
    g, gp = G.gelu_poly(x)
    ge, gpe = G.gelu_erf(x)
    assert (g - ge).abs().max().item() < 1.0e-5 and (gp - gpe).abs().max().item() < 4.0e-5


@pytest.mark.parametrize("nh", [1, 3])
def test_unrounded_model_is_the_oracle(nh):
    c = G.gno_case("mid", 2003, nh)
    got = G.gno_forms(c, "R", rounding=False, gelu="erf")
    exact = G.gno_forms(c, "E")
    sd = {}
    for i, (w, b) in enumerate(zip(c["ws"], c["bs"])):
        sd[f"channel_mlp.fcs.{i}.weight"] = w.double().requires_grad_(True)
        sd[f"channel_mlp.fcs.{i}.bias"] = b.double().requires_grad_(True)
    y, x, f = (c[k].double().requires_grad_(True) for k in ("y", "x", "f"))
    out = orc.integral_transform(sd, "", y, x, c["ei"].long(), f)
    (out * c["gout"].double()).sum().backward()
    ref = {"out": out.detach(), "grad_f": f.grad, "grad_y": y.grad, "grad_x": x.grad}
    for i in range(nh + 1):
        ref[f"dW{i}"], ref[f"db{i}"] = sd[f"channel_mlp.fcs.{i}.weight"].grad, sd[f"channel_mlp.fcs.{i}.bias"].grad
    assert set(ref) == set(got)
    for name, r in ref.items():
        peak = r.abs().max().item()
        for res in (got, exact):
            assert (res[name] - r).abs().max().item() <= 1e-12 * max(peak, 1.0), name


def test_unrounded_mlp_is_autograd():
    c = G.mlp_case(300, 128, 3, True)
    got = G.mlp_forms(c, "E")
    x, w1, b1, w2, b2 = (c[k].double().requires_grad_(True) for k in ("x", "w1", "b1", "w2", "b2"))
    out = torch.nn.functional.linear(torch.nn.functional.gelu(torch.nn.functional.linear(x, w1, b1)), w2, b2)
    (out * c["dout"].double()).sum().backward()
    for name, r in (("out", out.detach()), ("dx", x.grad), ("dW1", w1.grad), ("db1", b1.grad), ("dW2", w2.grad)):
        assert (got[name] - r).abs().max().item() <= 1e-12 * max(r.abs().max().item(), 1.0), name


# ---- the condition on the inputs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,e,nh", G.SMALL_GNO, ids=lambda v: str(v))
def test_input_condition_gno(kind, e, nh):
    c = G.gno_case(kind, e, nh)
    G.floors(c["tag"], G.gno_forms, c).done()


@pytest.mark.parametrize("rows,hidden,oc,with_b2", G.SMALL_MLP, ids=lambda v: str(v))
def test_input_condition_mlp(rows, hidden, oc, with_b2):
    c = G.mlp_case(rows, hidden, oc, with_b2)
    G.floors(c["tag"], G.mlp_forms, c).done()


# ---- the rule's teeth ---------------------------------------------------------------------------------------------------------------
TEETH = {"e17": ("tail", 17, 3), "e129": ("tail", 129, 3), "mid": ("mid", 20011, 3)}
_cache = {}


def _forms(key):
    if key not in _cache:
        c = G.gno_case(*TEETH[key])
        _cache[key] = (c, G.gno_forms(c, "R"), G.gno_forms(c, "E"))
    return _cache[key]


def _judge(key, got, tag):
    """-> the names of the tensors of ``got`` the rule rejects"""
    _c, r, e = _forms(key)
    rep = B.Report(f"teeth/{key}/{tag}")
    return {name for name in r if not rep.model(name, got[name], r[name], e[name])}


ALL = lambda nh: {"out", "grad_f", "grad_y", "grad_x"} | {f"dW{l}" for l in range(nh + 1)} | {f"db{l}" for l in range(nh + 1)}  # noqa: E731


@pytest.mark.parametrize("key", list(TEETH))
def test_undamaged_passes(key):
    c, _r, _e = _forms(key)
    for seed in G.SEEDS:
        assert _judge(key, G.gno_forms(c, "F", seed=seed), f"F{seed}") == set()


@pytest.mark.parametrize("key", ["e17", "e129"])
def test_last_edge_missing(key):
    """the tile's last edge reaches no sum (the degrees still count it): every tensor is rejected"""
    c, _r, _e = _forms(key)
    short = dict(c, ei=c["ei"][:, :-1])
    deg = torch.bincount(c["ei"][1].long(), minlength=c["n_dst"])
    assert _judge(key, G.gno_forms(short, "F", damage={"deg": deg}), "last edge missing") == ALL(3)


@pytest.mark.parametrize("key", list(TEETH))
def test_mean_over_deg_plus_one(key):
    """one output row of typical (median) degree divided by deg + 1"""
    c, _r, _e = _forms(key)
    deg = torch.bincount(c["ei"][1].long(), minlength=c["n_dst"])
    med = deg[deg > 0].median()
    q = int((deg == med).nonzero()[0])
    got = G.gno_forms(c, "F")
    got["out"][q] *= float(deg[q]) / float(deg[q] + 1)
    assert _judge(key, got, "mean over deg + 1") == {"out"}


@pytest.mark.parametrize("key", list(TEETH))
def test_bias_dropped_for_one_unit(key):
    c, _r, _e = _forms(key)
    bs = [b.clone() for b in c["bs"]]
    bs[1][5] = 0.0
    bad = _judge(key, G.gno_forms(dict(c, bs=bs), "F"), "b_1[5] dropped")
    assert {"out", "grad_f", "dW1", "db1", "dW2"} <= bad


@pytest.mark.parametrize("key", list(TEETH))
def test_truncation_for_rounding(key):
    c, _r, _e = _forms(key)
    bad = _judge(key, G.gno_forms(c, "F", damage={"round_h": G.trunc_bf16}), "h truncated")
    assert {"out", "grad_f", "dW3", "dW2", "db2"} <= bad


@pytest.mark.parametrize("key", list(TEETH))
def test_inverse_degree_twice(key):
    """dk of one query row of typical degree carries 1 / deg twice"""
    c, _r, _e = _forms(key)
    deg = torch.bincount(c["ei"][1].long(), minlength=c["n_dst"])
    cand = deg[deg > 1]
    q = int((deg == cand.median()).nonzero()[0])
    scale = torch.ones(c["n_dst"])
    scale[q] = 1.0 / float(deg[q])
    bad = _judge(key, G.gno_forms(c, "F", damage={"dk_scale": scale}), "1/deg twice")
    assert {"dW3", "db3", "dW0", "grad_y"} <= bad and not ({"out", "grad_f"} & bad)


@pytest.mark.parametrize("key", list(TEETH))
def test_coordinates_swapped_in_one_tile(key):
    c, _r, _e = _forms(key)
    tile = (c["ei"].shape[1] - 1) // 16 // 2
    assert _judge(key, G.gno_forms(c, "F", damage={"swap_tile": tile}), "y, x swapped in dW_0") == {"dW0"}


@pytest.mark.parametrize("key", list(TEETH))
def test_exact_form_is_not_this_kernel(key):
    _c, _r, e = _forms(key)
    assert _judge(key, e, "no rounding") == ALL(3)


def test_zero_rule_and_shapes():
    rep = B.Report("teeth")
    z = torch.zeros(4, 32, dtype=torch.float64)
    r = z.clone()
    r[1] = 1.0
    e = r * (1 + 1e-3)
    assert rep.model("row without edges", r.float(), r, e)
    got = r.float()
    got[3, 7] = 1e-30
    assert not rep.model("row without edges written", got, r, e)
    assert not rep.model("empty graph written", got, z, z) and rep.model("empty graph", z.float(), z, z)
    assert not rep.model("nan", torch.full_like(got, float("nan")), r, e)
    assert not rep.model("shape", got[:3], r, e)
