"""The fused projection-tangent kernel (csrc/mlp2_jvp.hip: gaot_mlp2_jvp) behind ``jvp_rows(..., fused=, out=)`` and ``sample_jacobian``.

  * value: torch.equal to ``forward_rows`` in fp32 mode for both MLP classes, hidden in {64, 128, 256}, out in {1, 3, 4}, with and
    without the second bias, at 1 .. 1000 rows and at one full sweep of the kernel's grid plus a partial tile;
  * tangents: the fp32 bar of tests/test_field_jacobian_gpu.py (max error <= 1e-3 of the reference's peak, cosine >= 0.99999) against
    the closed-form fp64 reference tests/mlp_jvp_ref.py for 1, 2 and 3 planes, the chain's figures printed beside them;
  * a plane does not depend on the planes beside it, a zero plane gives exact zeros, a row does not depend on the other rows (alone,
    in two slices, permuted, beside a NaN row and a +-1e30 row);
  * ``out=`` writes [N, out] and [N, out, T] views in place and leaves guard rows alone;
  * dispatch: eligible modules take one mlp2_jvp launch, ineligible ones and fused=False the chain, fused=True on an ineligible
    module raises before any launch;
  * sample_jacobian on the knn and on the row-list route runs the kernel, pred torch.equal to sample, jac within the bar of autograd,
    chunkings bit-identical;
  * peak memory of the fused call stays below one [N, 256] hidden tensor; a captured call replays to the eager result bit for bit."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_jvp_ref as REF  # noqa: E402
import test_field_jacobian_gpu as jb  # noqa: E402  (check() and its bar, the model fixture, the watchers)
import test_field_jacobian_rows_gpu as jr  # noqa: E402  (the row-list model fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID_CAP, TILE_ROWS = 512, 128                   # csrc/mlp2_jvp.hip: JV_GRID_CAP workgroups of JV_ROWS rows
SWEEP_PLUS = GRID_CAP * TILE_ROWS + 33           # one full sweep of the grid, then one full wave tile and one row
ROWS = (1, 31, 32, 33, 127, 128, 129, 1000, SWEEP_PLUS)


def _mlp(kind, hidden=256, oc=4, bias2=True, seed=5):
    from gaot_3d_amd.model.layers.mlp import ChannelMLP, LinearChannelMLP
    torch.manual_seed(seed + hidden + oc)
    mlp = LinearChannelMLP([32, hidden, oc]) if kind == "linear" else ChannelMLP(32, oc, hidden, n_layers=2)
    if not bias2:
        mlp.fcs[1].bias = None
    return mlp.to(DEV).eval()


_DATA = {}


def _data(n=1000, seed=6):
    """x [n, 32] and three tangent planes on the device, made once per (n, seed) and never modified"""
    if (n, seed) not in _DATA:
        gen = torch.Generator().manual_seed(seed)
        x = torch.randn(n, 32, generator=gen)
        dxs = [torch.randn(n, 32, generator=gen) for _ in range(3)]
        _DATA[(n, seed)] = (x.to(DEV), [d.to(DEV) for d in dxs])
    return _DATA[(n, seed)]


# ---- value ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [64, 128, 256])
@pytest.mark.parametrize("kind", ["linear", "channel"])
def test_value_is_forward_rows_bit_for_bit(kind, hidden):
    xall, dall = _data(SWEEP_PLUS, seed=7)
    for oc in (1, 3, 4):
        for bias2 in (True, False):
            mlp = _mlp(kind, hidden, oc, bias2)
            for n in ROWS:
                x, dxs = xall[:n], [d[:n] for d in dall]
                y, dys = mlp.jvp_rows(x, dxs, fused=True)
                with torch.no_grad():
                    ref = mlp.forward_rows(x)
                assert y.shape == (n, oc) and len(dys) == 3 and all(d.shape == (n, oc) and d.is_contiguous() for d in dys)
                assert not y.requires_grad and not dys[0].requires_grad
                assert torch.equal(y, ref), (kind, hidden, oc, bias2, n, (y - ref).abs().max().item())
                if n == 1000:           # the value does not depend on the planes that ride along
                    assert torch.equal(mlp.jvp_rows(x, [], fused=True)[0], ref)
                    assert torch.equal(mlp.jvp_rows(x, dxs[:1], fused=True)[0], ref)


def test_value_in_bf16_mode_is_the_fp32_value():
    mlp = _mlp("linear")
    x, dxs = _data()
    y, dys = mlp.jvp_rows(x, dxs)
    with jb._precision("bf16"):
        yb, dyb = mlp.jvp_rows(x, dxs)
    assert torch.equal(y, yb) and all(torch.equal(a, b) for a, b in zip(dys, dyb))


# ---- tangents ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [64, 128, 256])
@pytest.mark.parametrize("kind", ["linear", "channel"])
def test_tangents_meet_the_fp32_bar(kind, hidden):
    x, dxs = _data()
    for oc, bias2 in ((4, True), (3, False), (1, True)):
        mlp = _mlp(kind, hidden, oc, bias2)
        yr, refs = REF.mlp_jvp(*REF.weights_of(mlp), x.cpu(), [d.cpu() for d in dxs])
        for t in (1, 2, 3):
            y, dys = mlp.jvp_rows(x, dxs[:t], fused=True)
            yc, dyc = mlp.jvp_rows(x, dxs[:t], fused=False)
            assert len(dys) == t and torch.equal(y, yc)
            assert torch.allclose(y.cpu().double(), yr, rtol=1e-4, atol=1e-5)
            for d in range(t):
                name = f"jvp_rows/{kind}/h{hidden}/out{oc}/T{t}/direction{d}"
                err, peak, cos = jb.measure(dyc[d], refs[d])
                print(f"[parity] {name} fused=False: rel_to_peak={err / peak:.3e} cosine={cos:.7f}")
                jb.check(name + " fused=True", dys[d], refs[d])


def test_saturated_gelu_rows_meet_the_bar():
    """rows scaled so that |z| reaches 6-10 (gelu' is 0 or 1 there) beside ordinary rows"""
    mlp = _mlp("linear", 256, 4)
    x, dxs = _data()
    x = x.clone()
    x[::3] *= 8.0
    yr, refs = REF.mlp_jvp(*REF.weights_of(mlp), x.cpu(), [d.cpu() for d in dxs])
    y, dys = mlp.jvp_rows(x, dxs, fused=True)
    with torch.no_grad():
        assert torch.equal(y, mlp.forward_rows(x))
    for d in range(3):
        jb.check(f"jvp_rows/saturated/direction{d}", dys[d], refs[d])


def test_a_plane_does_not_depend_on_the_others():
    x, dxs = _data()
    for hidden in (64, 256):
        mlp = _mlp("linear", hidden, 3)
        _, one = mlp.jvp_rows(x, dxs[:1], fused=True)
        _, three = mlp.jvp_rows(x, dxs, fused=True)
        _, swapped = mlp.jvp_rows(x, [dxs[0], dxs[2], dxs[1]], fused=True)
        assert torch.equal(one[0], three[0]) and torch.equal(swapped[0], three[0])
        assert torch.equal(swapped[1], three[2]) and torch.equal(swapped[2], three[1])


def test_a_zero_plane_gives_exact_zeros():
    x, dxs = _data()
    mlp = _mlp("channel", 128, 4)
    _, full = mlp.jvp_rows(x, dxs, fused=True)
    for z in range(3):
        planes = [torch.zeros_like(d) if i == z else d for i, d in enumerate(dxs)]
        _, got = mlp.jvp_rows(x, planes, fused=True)
        assert torch.equal(got[z], torch.zeros_like(got[z])) and (got[z] == 0).all()
        for i in range(3):
            if i != z:
                assert torch.equal(got[i], full[i]), (z, i)


def test_a_row_does_not_depend_on_the_other_rows():
    x, dxs = _data()
    n = x.shape[0]
    mlp = _mlp("linear", 256, 4)
    y, dys = mlp.jvp_rows(x, dxs, fused=True)
    whole = torch.stack([y, *dys])                                              # [4, N, out]

    def run(xx, dd):
        yy, dy = mlp.jvp_rows(xx.contiguous(), [d.contiguous() for d in dd], fused=True)
        return torch.stack([yy, *dy])
    alone = torch.cat([run(x[i:i + 1], [d[i:i + 1] for d in dxs]) for i in range(n)], dim=1)
    assert torch.equal(alone, whole)
    pieces = torch.cat([run(x[:517], [d[:517] for d in dxs]), run(x[517:], [d[517:] for d in dxs])], dim=1)
    assert torch.equal(pieces, whole)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(8)).to(DEV)
    shuffled = run(x[perm], [d[perm] for d in dxs])
    assert torch.equal(shuffled, whole[:, perm])
    # one row of NaN and one of +-1e30 beside the others
    xb, db = x.clone(), [d.clone() for d in dxs]
    xb[5] = float("nan")
    db[1][5] = float("nan")
    sign = torch.where(torch.arange(32, device=DEV) % 2 == 0, 1.0, -1.0)
    xb[700] = 1e30 * sign
    db[0][700] = -1e30 * sign
    bad = run(xb, db)
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[5] = keep[700] = False
    assert torch.equal(bad[:, keep], whole[:, keep])
    assert torch.isnan(bad[0, 5]).all()


# ---- out= -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
def test_out_views_are_written_in_place_and_guards_stay(fused):
    x, dxs = _data()
    n, guard, sentinel = x.shape[0], 7, -12345.0
    for oc, t in ((4, 3), (1, 3), (3, 2), (2, 1), (4, 0)):
        mlp = _mlp("linear", 256, oc)
        y, dys = mlp.jvp_rows(x, dxs[:t], fused=fused)
        pred = torch.full((n + 2 * guard, oc), sentinel, device=DEV)
        jac = torch.full((n + 2 * guard, oc, t), sentinel, device=DEV)
        pv, jv = pred[guard:guard + n], jac[guard:guard + n]
        y2, dy2 = mlp.jvp_rows(x, dxs[:t], fused=fused, out=(pv, jv))
        assert y2.data_ptr() == pv.data_ptr() and len(dy2) == t
        assert torch.equal(pv, y)
        for d in range(t):
            assert dy2[d].data_ptr() == jv[:, :, d].data_ptr() and dy2[d].shape == (n, oc)
            assert torch.equal(jv[:, :, d], dys[d]), (oc, t, d)            # layout [n, out, T]
        for buf in (pred, jac):
            assert (buf[:guard] == sentinel).all() and (buf[guard + n:] == sentinel).all()
    from gaot_3d_amd._lib import GaotError
    mlp = _mlp("linear", 256, 4)
    with pytest.raises(GaotError, match="out must be"):
        mlp.jvp_rows(x, dxs, out=(torch.empty(n, 4, device=DEV), torch.empty(n, 4, 2, device=DEV)))
    if fused:               # a destination whose planes overlap (an expanded view) is refused by the library
        with pytest.raises(GaotError, match="non-positive stride"):
            mlp.jvp_rows(x, dxs, fused=True, out=(torch.empty(n, 4, device=DEV), torch.empty(n, 4, 1, device=DEV).expand(n, 4, 3)))


# ---- dispatch ---------------------------------------------------------------------------------------------------------------------------
def _run_watched(fn):
    """-> (result, timing keys, launches) of fn()"""
    from gaot_3d_amd import ops
    torch.cuda.synchronize()
    ops.timing_reset(True)
    try:
        n0 = ops.launch_count()
        res = fn()
        launches = ops.launch_count() - n0
        torch.cuda.synchronize()
        keys = set(ops.timing_summary())
    finally:
        ops.timing_reset(False)
    return res, keys, launches


def _ineligible():
    from gaot_3d_amd.model.layers.mlp import ChannelMLP, LinearChannelMLP
    torch.manual_seed(9)
    return {
        "three_layers": (LinearChannelMLP([32, 64, 64, 4]), 32),
        "relu": (LinearChannelMLP([32, 256, 4], non_linearity="relu"), 32),
        "in48": (ChannelMLP(48, 4, 256, n_layers=2), 48),
        "hidden96": (LinearChannelMLP([32, 96, 4]), 32),
        "out5": (LinearChannelMLP([32, 256, 5]), 32),
    }


def _fp64_jvp(mlp, x, dxs):
    """fp64 autograd reference of any MLP of the two classes (the ineligible ones have no closed form in mlp_jvp_ref)"""
    ws = [(fc.weight[:, :, 0] if fc.weight.dim() == 3 else fc.weight).detach().double().cpu() for fc in mlp.fcs]
    bs = [fc.bias.detach().double().cpu() for fc in mlp.fcs]
    act = {"gelu": torch.nn.functional.gelu, "relu": torch.relu}[mlp.non_linearity]

    def f(h):
        for i, (w, b) in enumerate(zip(ws, bs)):
            h = h @ w.t() + b
            if i + 1 < len(ws):
                h = act(h)
        return h
    return [torch.autograd.functional.jvp(f, x.double().cpu(), d.double().cpu()) for d in dxs]


def test_dispatch():
    from gaot_3d_amd._lib import GaotError
    x, dxs = _data()
    for kind in ("linear", "channel"):
        mlp = _mlp(kind, 256, 4)
        (y, dys), keys, launches = _run_watched(lambda: mlp.jvp_rows(x, dxs))
        assert any(k.startswith("mlp2_jvp") for k in keys) and not any("gemm" in k for k in keys), keys
        assert launches == 1
        (yc, dyc), keys, launches = _run_watched(lambda: mlp.jvp_rows(x, dxs, fused=False))
        assert not any(k.startswith("mlp2_jvp") for k in keys) and launches > 1, (keys, launches)
        assert torch.equal(y, yc)
        yr, refs = REF.mlp_jvp(*REF.weights_of(mlp), x.cpu(), [d.cpu() for d in dxs])
        for d in range(3):
            jb.check(f"dispatch/{kind}/chain/direction{d}", dyc[d], refs[d], quiet=True)
    gen = torch.Generator().manual_seed(10)
    for name, (mlp, cin) in _ineligible().items():
        mlp = mlp.to(DEV).eval()
        xi = torch.randn(500, cin, generator=gen).to(DEV)
        di = [torch.randn(500, cin, generator=gen).to(DEV) for _ in range(3)]
        (y, dys), keys, launches = _run_watched(lambda: mlp.jvp_rows(xi, di))
        assert not any(k.startswith("mlp2_jvp") for k in keys) and launches > 1, (name, keys, launches)
        with torch.no_grad():
            assert torch.equal(y, mlp.forward_rows(xi)), name
        for d, (yr, dr) in enumerate(_fp64_jvp(mlp, xi, di)):
            assert torch.allclose(y.cpu().double(), yr, rtol=1e-4, atol=1e-5), name
            jb.check(f"dispatch/{name}/direction{d}", dys[d], dr, quiet=True)
        _, keys, launches = _run_watched(lambda: pytest.raises(GaotError, mlp.jvp_rows, xi, di, fused=True))
        assert launches == 0 and not keys, (name, keys, launches)
    # operands outside the kernel's set on an eligible module: four planes, a strided plane, no first bias
    mlp = _mlp("linear", 256, 4)
    four = dxs + [dxs[0]]
    strided = [d.t().contiguous().t() for d in dxs]
    for planes in (four, strided):
        (y, dys), keys, launches = _run_watched(lambda: mlp.jvp_rows(x, planes))
        assert not any(k.startswith("mlp2_jvp") for k in keys) and launches > 1 and len(dys) == len(planes)
        _, keys, launches = _run_watched(lambda: pytest.raises(GaotError, mlp.jvp_rows, x, planes, fused=True))
        assert launches == 0
    mlp.fcs[0].bias = None
    _, keys, launches = _run_watched(lambda: pytest.raises(GaotError, mlp.jvp_rows, x, dxs, fused=True))
    assert launches == 0
    (y, dys), keys, launches = _run_watched(lambda: mlp.jvp_rows(x, dxs))
    assert not any(k.startswith("mlp2_jvp") for k in keys) and launches > 1


def test_bad_arguments_raise_before_any_launch():
    import ctypes as C
    from gaot_3d_amd import _lib, ops
    from gaot_3d_amd._lib import GaotError
    lib = _lib.load()
    x, dxs = _data()
    n = x.shape[0]
    w1, b1, w2, b2 = (t.to(DEV) for t in REF.weights_of(_mlp("linear", 256, 4)))
    y, jac = torch.empty(n, 4, device=DEV), torch.empty(n, 4, 3, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)
    torch.cuda.synchronize()
    n0 = ops.launch_count()

    def call(xp=ptr(x), d0=ptr(dxs[0]), t=3, rows=n, cin=32, hid=256, oc=4, w1p=ptr(w1), yp=ptr(y), ldy=4, jp=ptr(jac), js=(12, 3, 1)):
        _lib.check(lib.gaot_mlp2_jvp(xp, d0, ptr(dxs[1]), ptr(dxs[2]), t, rows, cin, hid, oc, w1p, ptr(b1), ptr(w2), ptr(b2), yp, ldy, jp,
                                     js[0], js[1], js[2], null), "gaot_mlp2_jvp")
    for kw, msg in ((dict(xp=null), "null pointer"), (dict(w1p=null), "null pointer"), (dict(yp=null), "null pointer"),
                    (dict(d0=null), "tangent plane"), (dict(jp=null), "null Jacobian"), (dict(js=(12, 3, 0)), "non-positive stride"),
                    (dict(ldy=3), "ldy"), (dict(rows=-1), "negative size"), (dict(xp=C.c_void_p(x.data_ptr() + 4)), "aligned"),
                    (dict(hid=96), "supported shapes"), (dict(cin=48), "supported shapes"), (dict(oc=5), "supported shapes"),
                    (dict(t=4), "supported shapes")):
        with pytest.raises(GaotError, match="gaot_mlp2_jvp: .*" + msg):
            call(**kw)
        assert ops.launch_count() == n0, kw
    call(rows=0)                                                # no rows: a successful no-op
    assert ops.launch_count() == n0
    call()
    assert ops.launch_count() == n0 + 1
    torch.cuda.synchronize()
    got = ops.mlp2_jvp(x, dxs, w1, b1, w2, b2)
    assert torch.equal(y, got[0]) and torch.equal(jac, got[1])


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def _end_to_end(model, batch, tokens, q, key, monkeypatch, **kw):
    with torch.no_grad():
        lat = model.latent(batch, tokens)
        smp = model.sample(lat, q)
    got = {}
    for chunk in (None, 700):
        with jb._watch(monkeypatch) as seen:
            got[chunk] = model.sample_jacobian(lat, q, chunk_points=chunk, **kw)
        assert any(k.startswith("mlp2_jvp") for k in seen["keys"]), seen
    pred, jac = got[None]
    assert torch.equal(pred, smp)
    assert torch.equal(got[700][0], pred) and torch.equal(got[700][1], jac)
    ref_p, ref_j = jb._autograd_jacobian((key, "random"), model, batch, tokens, q)
    assert torch.allclose(pred, ref_p, rtol=1e-4, atol=1e-5)
    jb.check(f"sample_jacobian/fused projection/{key}", jac, ref_j)


def test_sample_jacobian_knn_route_runs_the_kernel(monkeypatch):
    model, batch, tokens = jb._setup()
    _end_to_end(model, batch, tokens, jb._queries("random", batch), "cfg0", monkeypatch)


def test_sample_jacobian_row_list_route_runs_the_kernel(monkeypatch):
    key, (model, batch, tokens) = jr._model("radius")
    _end_to_end(model, batch, tokens, jb._queries("random", batch), key, monkeypatch, row_lists=True)


# ---- memory, graph replay ---------------------------------------------------------------------------------------------------------------
def test_fused_call_stays_below_one_hidden_tensor():
    n = 200000
    mlp = _mlp("linear", 256, 4)
    x, dxs = _data(n, seed=12)
    pred, jac = torch.empty(n, 4, device=DEV), torch.empty(n, 4, 3, device=DEV)
    hidden = n * 256 * 4
    fused = jb._rise(lambda: mlp.jvp_rows(x, dxs, fused=True, out=(pred, jac)))
    chain = jb._rise(lambda: mlp.jvp_rows(x, dxs, fused=False, out=(pred, jac)))
    print(f"[memory] jvp_rows at {n} rows, out=: fused {fused / 2**20:.2f} MiB, chain {chain / 2**20:.2f} MiB; one hidden tensor "
          f"{hidden / 2**20:.2f} MiB")
    assert fused < hidden, (fused, hidden)


def test_graph_replay_equals_eager():
    mlp = _mlp("channel", 256, 4)
    x, dxs = _data()
    x2, dxs2 = _data(1000, seed=13)
    n = x.shape[0]
    bx, bd = x.clone(), [d.clone() for d in dxs]
    pred, jac = torch.empty(n, 4, device=DEV), torch.empty(n, 4, 3, device=DEV)
    copies = lambda res: [res[0].clone(), *[d.clone() for d in res[1]]]
    e1 = copies(mlp.jvp_rows(bx, bd, fused=True, out=(pred, jac)))          # the eager call
    e2 = copies(mlp.jvp_rows(x2, dxs2, fused=True))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mlp.jvp_rows(bx, bd, fused=True, out=(pred, jac))
    pred.zero_()
    jac.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(pred, e1[0]) and all(torch.equal(jac[:, :, d], e1[1 + d]) for d in range(3))
    bx.copy_(x2)
    for b, d in zip(bd, dxs2):
        b.copy_(d)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(pred, e2[0]) and all(torch.equal(jac[:, :, d], e2[1 + d]) for d in range(3))
    assert not torch.equal(e1[0], e2[0])
