"""Single-pass thin fp32 linears (csrc/rowlinear.hip: gaot_rowlin_fwd / gaot_rowlin_bwd) behind GF.linear / GF.cat_linear at
precision 0: the per-point and per-token linears around the GNOs (reference magno.py:494,571-575,771-775: torch.cat + nn.Linear;
geoembed.py: the statistics MLP).

Reference: the same expression in fp64 on the CPU (torch.nn.functional.linear).  The bound is not invented: the GEMM route the
library took before (ops.gemm / ops.colsum / ops.act_bwd, still what every ineligible call takes; ops.ROWLIN["enabled"] = False
selects it) runs on the same inputs, and for every output the new kernels' rms and max error against fp64 may be at most 2x that
route's -- a different fp32 summation order moves the error by a factor of order one -- plus one fp32 ulp of the output's peak
for outputs where both errors are (nearly) zero.  Every comparison prints its achieved ratios as a `[parity]` line.

Row counts: a wave takes 32 rows, a workgroup 128 per pass, the forward's grid is capped at 512 workgroups -- 1, 127 / 128 / 129,
128 * 512 + 1 (one workgroup takes a second, ragged pass) -- and the backward walks the row ranges of the weight-gradient GEMM's
split-K plan, which begins to split at 4 096 rows (4 095 / 4 096; 65 537 and 70 001 rows are 32 ragged ranges)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS_PER_PASS, GRID_CAP = 128, 512

# name -> (input widths, N, ReLU, the "input needs a gradient" combinations the model produces)
SHAPES = {
    "lifting": ((3, 3), 32, False, [(False, False), (True, False)]),       # pos | c; pos needs one in the coordinate-gradient step
    "recovery": ((32, 32), 32, False, [(True, True)]),                      # enc | geo, dec | geo
    "geo1": ((9,), 64, True, [(False,), (True,)]),                           # GeoEmbed statistics -> 64, ReLU
    "geo2": ((64,), 32, False, [(True,)]),
    "ragged": ((5, 7, 1), 17, False, [(True, False, True)]),
}
CASES = [(name, need) for name, (_ks, _n, _relu, needs) in SHAPES.items() for need in needs]


@pytest.fixture(autouse=True)
def _fp32_mode():
    import gaot_3d_amd
    from gaot_3d_amd import ops
    gaot_3d_amd.set_precision("fp32")
    prev = ops.ROWLIN["enabled"]
    ops.ROWLIN["enabled"] = True
    yield
    ops.ROWLIN["enabled"] = prev
    ops.defer_reductions(False)


def _inputs(name, m, bias, seed=0):
    ks, n, relu, _ = SHAPES[name]
    g = torch.Generator().manual_seed(seed + 1000 * m % 7919)
    xs = [torch.randn(m, k, generator=g) for k in ks]
    w = torch.randn(n, sum(ks), generator=g) / np.sqrt(sum(ks))
    b = torch.randn(n, generator=g) if bias else None
    dy = torch.randn(m, n, generator=g)
    return xs, w, b, dy, relu


def _run(xs, w, b, dy, relu, need, new_route, defer=False):
    """forward + backward through GF.linear / GF.cat_linear on the GPU -> {name: tensor}, and the route counters' increments"""
    from gaot_3d_amd import functional as GF, ops
    ops.ROWLIN["enabled"] = new_route
    prev = ops.defer_reductions(defer)
    try:
        f0, b0 = ops.ROWLIN["fwd"], ops.ROWLIN["bwd"]
        xg = [x.to(DEV).requires_grad_(nd) for x, nd in zip(xs, need)]
        wg = w.to(DEV).requires_grad_(True)
        bg = None if b is None else b.to(DEV).requires_grad_(True)
        if len(xg) == 1:
            y = GF.linear(xg[0], wg, bg, act="relu" if relu else None, precision=0)
        else:
            y = GF.cat_linear(xg, wg, bg, precision=0)
        y.backward(dy.to(DEV))
        assert ops.deferred_pending() == 0
        torch.cuda.synchronize()
        out = {"y": y.detach(), "dW": wg.grad}
        if bg is not None:
            out["db"] = bg.grad
        for i, x in enumerate(xg):
            if need[i]:
                out[f"dx{i}"] = x.grad
            else:
                assert x.grad is None
        return out, (ops.ROWLIN["fwd"] - f0, ops.ROWLIN["bwd"] - b0)
    finally:
        ops.defer_reductions(prev)
        ops.ROWLIN["enabled"] = True


def _fp64(xs, w, b, dy, relu, need):
    xd = [x.double().requires_grad_(nd) for x, nd in zip(xs, need)]
    wd = w.double().requires_grad_(True)
    bd = None if b is None else b.double().requires_grad_(True)
    y = torch.nn.functional.linear(torch.cat(xd, dim=1), wd, bd)
    if relu:
        y = torch.relu(y)
    y.backward(dy.double())
    out = {"y": y.detach(), "dW": wd.grad}
    if bd is not None:
        out["db"] = bd.grad
    for i, x in enumerate(xd):
        if need[i]:
            out[f"dx{i}"] = x.grad
    return out


def _errs(a, ref):
    d = a.double().cpu() - ref
    if d.numel() == 0:
        return 0.0, 0.0
    return float(d.pow(2).mean().sqrt()), float(d.abs().max())


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("m", [1, ROWS_PER_PASS - 1, ROWS_PER_PASS, ROWS_PER_PASS + 1, 4095, 4096, ROWS_PER_PASS * GRID_CAP + 1])
@pytest.mark.parametrize("name,need", CASES, ids=[f"{n}-{''.join('g' if x else 'n' for x in nd)}" for n, nd in CASES])
def test_rowlinear_against_fp64_and_the_gemm_route(name, need, m, bias):
    xs, w, b, dy, relu = _inputs(name, m, bias)
    ref = _fp64(xs, w, b, dy, relu, need)
    new, took = _run(xs, w, b, dy, relu, need, True)
    old, took_old = _run(xs, w, b, dy, relu, need, False)
    assert took == (1, 1) and took_old == (0, 0), (took, took_old)
    assert set(new) == set(old) == set(ref)
    for k in sorted(ref):
        assert tuple(new[k].shape) == tuple(ref[k].shape), (k, new[k].shape, ref[k].shape)
        assert torch.isfinite(new[k]).all(), k
        rms_n, max_n = _errs(new[k], ref[k])
        rms_o, max_o = _errs(old[k], ref[k])
        floor = float(np.spacing(np.float32(ref[k].abs().max().item())))
        print(f"[parity] rowlinear {name} need={need} M={m} bias={bias} {k}: rms new/old {rms_n:.3e}/{rms_o:.3e} = "
              f"{rms_n / max(rms_o, 1e-300):.2f}, max new/old {max_n:.3e}/{max_o:.3e} = {max_n / max(max_o, 1e-300):.2f} (ulp of peak {floor:.1e})")
        assert rms_n <= 2 * rms_o + floor, f"{k}: rms error {rms_n:.3e} against the GEMM route's {rms_o:.3e}"
        assert max_n <= 2 * max_o + floor, f"{k}: max error {max_n:.3e} against the GEMM route's {max_o:.3e}"
    # more than the bound asks: the kernels keep the GEMM route's summation order, so a step computes what it computed before
    for k in sorted(ref):
        assert torch.equal(new[k], old[k]), f"{k}: differs from the GEMM route by {(new[k] - old[k]).abs().max().item():.3e}"


@pytest.mark.parametrize("name,need", CASES, ids=[f"{n}-{''.join('g' if x else 'n' for x in nd)}" for n, nd in CASES])
def test_no_rows(name, need):
    xs, w, b, dy, relu = _inputs(name, 0, True)
    out, took = _run(xs, w, b, dy, relu, need, True)
    assert took == (1, 1)
    assert out["y"].shape == (0, w.shape[0])
    assert out["dW"].shape == w.shape and not out["dW"].any() and not out["db"].any()
    for i, nd in enumerate(need):
        if nd:
            assert out[f"dx{i}"].shape == xs[i].shape


@pytest.mark.parametrize("name,need", [("lifting", (True, False)), ("recovery", (True, True)), ("geo1", (True,)), ("geo2", (True,)),
                                       ("ragged", (True, False, True))])
def test_rows_do_not_depend_on_m(name, need):
    """sharded rows are compared with unsharded ones: the first 300 rows of a 70 001-row call are those of a 300-row call, bit for bit"""
    xs, w, b, dy, relu = _inputs(name, 70001, True)
    big, _ = _run(xs, w, b, dy, relu, need, True)
    small, _ = _run([x[:300] for x in xs], w, b, dy[:300], relu, need, True)
    for k in small:
        if k == "y" or k.startswith("dx"):
            assert torch.equal(big[k][:300], small[k]), k


@pytest.mark.parametrize("name,need", [("lifting", (False, False)), ("recovery", (True, True)), ("geo1", (False,)), ("ragged", (True, False, True))])
def test_reruns_and_deferred_completion_are_bit_identical(name, need):
    xs, w, b, dy, relu = _inputs(name, ROWS_PER_PASS * GRID_CAP + 1, True)
    a, _ = _run(xs, w, b, dy, relu, need, True)
    c, _ = _run(xs, w, b, dy, relu, need, True)
    d, took = _run(xs, w, b, dy, relu, need, True, defer=True)
    assert took == (1, 1)
    for k in a:
        assert torch.equal(a[k], c[k]), f"{k}: rerun differs"
        assert torch.equal(a[k], d[k]), f"{k}: deferred completion differs from the in-call one"


def test_deferral_is_taken_and_saves_the_launch():
    """with the deferral on, dW and db of the backward are completed by the end-of-pass launch: the backward is ONE launch of the library
    plus that one"""
    from gaot_3d_amd import functional as GF, ops
    xs, w, b, dy, _ = _inputs("recovery", 1000, True)
    counts = {}
    for defer in (False, True):
        prev = ops.defer_reductions(defer)
        try:
            xg = [x.to(DEV).requires_grad_(True) for x in xs]
            wg, bg = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
            y = GF.cat_linear(xg, wg, bg, precision=0)
            seen = []
            xg[0].register_hook(lambda g: seen.append(ops.deferred_pending()))     # runs right behind the node's backward
            ops.launch_count_reset()
            y.backward(dy.to(DEV))
            counts[defer] = ops.launch_count()
            assert seen == [2 if defer else 0], seen                                  # dW and db wait for the end of the pass
            assert ops.deferred_pending() == 0
        finally:
            ops.defer_reductions(prev)
    assert counts[False] == 2 and counts[True] == 2, counts      # kernel + one reduction of both tables, in the call or at the end


def test_mlp2_deferred_completion_is_bit_identical():
    """the projection MLP's three weight-gradient tables: ONE reduction launch in the call, or entries of the end-of-pass launch --
    the same bits; rows = 128 * 256 + 1 gives one workgroup of the backward a second pass"""
    import gaot_3d_amd
    from gaot_3d_amd import functional as GF, ops
    g = torch.Generator().manual_seed(11)
    m = 128 * 256 + 1
    x = torch.randn(m, 32, generator=g).to(DEV)
    ws = [torch.randn(256, 32, generator=g) / 6, torch.randn(256, generator=g), torch.randn(1, 256, generator=g) / 16, torch.randn(1, generator=g)]
    dy = torch.randn(m, 1, generator=g).to(DEV)
    got = {}
    gaot_3d_amd.set_precision("bf16")
    try:
        for defer in (False, True):
            prev = ops.defer_reductions(defer)
            try:
                xg = x.clone().requires_grad_(True)
                ps = [w.to(DEV).requires_grad_(True) for w in ws]
                seen = []
                xg.register_hook(lambda grad: seen.append(ops.deferred_pending()))
                ops.launch_count_reset()
                GF.Mlp2Fn.apply(xg, *ps).backward(dy)
                n = ops.launch_count()
                assert ops.deferred_pending() == 0
                torch.cuda.synchronize()
                assert seen == [3 if defer else 0], seen
                got[defer] = ([xg.grad] + [p.grad for p in ps], n)
            finally:
                ops.defer_reductions(prev)
    finally:
        gaot_3d_amd.set_precision("fp32")
    assert got[False][1] == got[True][1], (got[False][1], got[True][1])     # one reduction launch either way
    for a, b in zip(got[False][0], got[True][0]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("defer", [False, True], ids=["in-call", "deferred"])
def test_graph_capture_replays_the_eager_result(defer):
    from gaot_3d_amd import functional as GF, ops
    ops.defer_reductions(defer)          # (the autouse fixture switches it off again)
    xs, w, b, dy, _ = _inputs("geo1", 1000, True)
    xs2, w2, b2, _, _ = _inputs("geo2", 1000, True, seed=5)
    x = xs[0].to(DEV)
    dyd = torch.randn(1000, 32, generator=torch.Generator().manual_seed(3)).to(DEV)
    params = [t.to(DEV).requires_grad_(True) for t in (w, b, w2, b2)]

    def step():
        for p in params:
            p.grad = None
        h = GF.linear(x, params[0], params[1], act="relu", precision=0)
        y = GF.linear(h, params[2], params[3], precision=0)
        y.backward(dyd)
        return [y.detach()] + [p.grad for p in params]

    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                       # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for t in outs:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, r in zip(eager, outs):
        assert torch.equal(a, r)


def test_ineligible_calls_take_the_gemm_route():
    """K = 128, a residual, the same tensor twice, bf16 mode: today's code runs (route counters unchanged) and gives its result"""
    from gaot_3d_amd import functional as GF, ops
    g = torch.Generator().manual_seed(7)
    m = 257

    def both(fn):
        f0, b0 = ops.ROWLIN["fwd"], ops.ROWLIN["bwd"]
        got = fn()
        assert (ops.ROWLIN["fwd"], ops.ROWLIN["bwd"]) == (f0, b0), "an ineligible call took the single-pass kernels"
        ops.ROWLIN["enabled"] = False
        try:
            want = fn()
        finally:
            ops.ROWLIN["enabled"] = True
        for a, r in zip(got, want):
            assert torch.equal(a, r)

    x128, w128 = torch.randn(m, 128, generator=g).to(DEV), torch.randn(32, 128, generator=g).to(DEV)
    x32, w32, res = torch.randn(m, 32, generator=g).to(DEV), torch.randn(32, 32, generator=g).to(DEV), torch.randn(m, 32, generator=g).to(DEV)
    w64, dy = torch.randn(32, 64, generator=g).to(DEV), torch.randn(m, 32, generator=g).to(DEV)

    def run(make):
        def fn():
            leaves, y = make()
            y.backward(dy)
            return [y.detach()] + [t.grad for t in leaves]
        return fn

    def wide():
        w = w128.clone().requires_grad_(True)
        return [w], GF.linear(x128, w, None, precision=0)

    def residual():
        w, x = w32.clone().requires_grad_(True), x32.clone().requires_grad_(True)
        return [w, x], GF.linear(x, w, None, precision=0, residual=res)

    def twice():
        w, x = w64.clone().requires_grad_(True), x32.clone().requires_grad_(True)
        return [w, x], GF.cat_linear([x, x], w, None, precision=0)

    def bf16_mode():
        w, x = w32.clone().requires_grad_(True), x32.clone().requires_grad_(True)
        return [w, x], GF.linear(x, w, None, precision=1)

    for make in (wide, residual, twice, bf16_mode):
        both(run(make))
    # and an eligible call of the same family does take them
    f0 = ops.ROWLIN["fwd"]
    GF.linear(x32, w32, None, precision=0)
    assert ops.ROWLIN["fwd"] == f0 + 1
