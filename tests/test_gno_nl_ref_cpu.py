"""The teeth of tests/gno_nl_ref.py (the rounding model of the fused 'nonlinear' / 'nonlinear_kernelonly' GNO transform):
  * its exact form E is the oracle's integral_transform(..., transform_type=...) and its autograd;
  * the fp32 realisations F of the rounding model R sit within 1/12 (rms) and 2/3 (max) of the yardstick R - E on every small case
    of tests/test_gno_nonlinear_bf16_fp64_gpu.py, over three shuffle seeds -- the margin under the kernels' rule (1/4 and 2)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import block_ref as B  # noqa: E402
import gno_nl_ref as N  # noqa: E402


def _oracle(case):
    import gaot_oracle as orc
    c = case
    leaf = {}
    for i, (w, b) in enumerate(zip(c["ws"], c["bs"])):
        leaf[f"it.channel_mlp.fcs.{i}.weight"] = w.double().requires_grad_()
        leaf[f"it.channel_mlp.fcs.{i}.bias"] = b.double().requires_grad_()
    y, x, f = (c[k].double().requires_grad_() for k in ("y", "x", "f"))
    out = orc.integral_transform(leaf, "it.", y, x, c["ei"].long(), f, transform_type=c["mode"])
    gs = torch.autograd.grad((out * c["gout"].double()).sum(), [y, x, f] + list(leaf.values()), allow_unused=True)
    cd, nh = y.shape[1], len(c["ws"]) - 1
    res = {"out": out.detach(), "grad_y": gs[0], "grad_x": gs[1], "grad_f": gs[2]}
    gw = {k: g for k, g in zip(leaf, gs[3:])}
    res["dW0c"], res["dW0f"] = gw["it.channel_mlp.fcs.0.weight"][:, :2 * cd], gw["it.channel_mlp.fcs.0.weight"][:, 2 * cd:]
    res["db0"] = gw["it.channel_mlp.fcs.0.bias"]
    for l in range(1, nh + 1):
        res[f"dW{l}"], res[f"db{l}"] = gw[f"it.channel_mlp.fcs.{l}.weight"], gw[f"it.channel_mlp.fcs.{l}.bias"]
    return res


ORACLE_CASES = [("tail", m, 129, 2, 32, 32, 64, 3) for m in N.MODES] + [("mid", m, *a[1:]) for m in N.MODES for a in N.SHAPES[m]]


@pytest.mark.parametrize("args", ORACLE_CASES, ids=lambda a: "-".join(str(v) for v in a))
def test_exact_form_is_the_oracle(args):
    c = N.nl_case(args[0], args[1], *args[2:])
    e, ref = N.nl_forms(c, "E"), _oracle(c)
    rep = B.Report(c["tag"])
    for name, t in ref.items():
        rep.fp32(name, e[name], t, bound=1e-11)
    rep.done()
    # dt is not a tensor of the oracle: it is pinned through dW_0f = dt^T f and grad_f above, and by its definition here
    assert e["dt"].shape == (c["n_src"], c["ws"][0].shape[0])


def test_sources_without_an_edge_have_zero_rows():
    c = N.nl_case("mid", "nonlinear", 2003, 2)
    hit = torch.zeros(c["n_src"], dtype=torch.bool)
    hit[c["ei"][0].long()] = True
    assert (~hit).any()
    r = N.nl_forms(c, "R")
    assert float(r["dt"][~hit].abs().max()) == 0.0 and float(r["grad_f"][~hit].abs().max()) == 0.0


_SMALL = N.small_cases()


@pytest.mark.parametrize("chunk", range(8))
def test_fp32_realisations_pass_the_rule_on_every_small_case(chunk):
    """every tensor of F (three seeds) against (R, E) at 1/12 (rms) and 2/3 (max) of the yardstick, the small cases in 8 chunks"""
    lines = []
    for args in _SMALL[chunk::8]:
        c = N.nl_case(args[0], args[1], *args[2:])
        rep, _ = N.floors(c)
        lines += rep.failures
    assert not lines, "\n".join(lines)
