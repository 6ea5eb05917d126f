"""gaot_mlp2_bwd_f32 (csrc/mlp2_bwd_f32.hip, ops.mlp2_backward_f32): the projection's backward in exact fp32, one launch --
d_x, d_W1, d_b1, d_W2 of y = W2 gelu(W1 x + b1) + b2 against fp64 autograd of the same MLP on the CPU.

rows in {1, 31, 32, 33, 127, 128, 129, 257, 1000} (below one 32-row sub-tile, on and around it, on and around the 128-row workgroup
tile, several workgroups) x hidden in {64, 128, 256} x out in {1, 2, 3, 4}; operands scaled so that z = W1 x + b1 spans about +-4
(both tails of the erf-GELU and its bend); the four outputs pre-filled with NaN through the C ABI.

Bars: the project's bar for fp32 derivatives (tests/test_coord_grad_gpu.py FP32_BAR: max error <= 1e-3 of the reference's peak, cosine
>= 0.99999), every peak asserted > 0; and, as tests/test_field_adjoint_gpu.py holds a new kernel beside an old one, each result's
distance to fp64 at most max(4 x the GEMM chain's on the same operands, 1e-6 of the peak) -- both sum the same fp32 terms in other
orders.  Two calls are torch.equal; d_x[:33] of rows = 33 is torch.equal to d_x[:33] of rows = 1000 (a row's d_x depends on that row
alone); rows = 0 gives zeros without a launch; shapes outside the family report 0 and raise GaotError before any launch.

Measured on an MI355X, worst over the shapes, as a fraction of the peak (the GEMM chain's figure at that shape in brackets): hidden 64
d_x 3.1e-7 (3.1e-7), d_w1 4.9e-7 (4.9e-7), d_b1 3.2e-7 (1.8e-7), d_w2 4.8e-7 (4.8e-7); hidden 128 2.5e-7 (4.8e-7), 4.8e-7 (4.8e-7),
2.5e-7 (2.5e-7), 4.0e-7 (3.3e-7); hidden 256 2.7e-7 (4.8e-7), 4.4e-7 (5.0e-7), 2.7e-7 (2.4e-7), 4.8e-7 (7.7e-7).  The test prints them."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_coord_grad_gpu as cg  # noqa: E402  (FP32_BAR)
import test_field_hessian_gpu as hb  # noqa: E402  (check, measure)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32_BAR = cg.FP32_BAR
ROWS = (1, 31, 32, 33, 127, 128, 129, 257, 1000)
HIDDEN = (64, 128, 256)
OUTS = (1, 2, 3, 4)
NAMES = ("d_x", "d_w1", "d_b1", "d_w2")


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """the workspaces and chunk tensors of these tests stay cached in torch's allocator; later tests that bound the rise of allocated
    memory are sensitive to which cached blocks they are served from, so the cache is handed back when this module is done"""
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _operands(hidden, oc):
    """1000 rows; a smaller case takes the first rows of the same tensors"""
    gen = torch.Generator().manual_seed(1000 * hidden + oc)
    x = torch.randn(1000, 32, generator=gen)
    w1 = torch.randn(hidden, 32, generator=gen) * (1.3 / 32 ** 0.5)
    b1 = torch.randn(hidden, generator=gen) * 0.5
    w2 = torch.randn(oc, hidden, generator=gen) / hidden ** 0.5
    g = torch.randn(1000, oc, generator=gen)
    return x, w1, b1, w2, g


def _fp64(x, w1, b1, w2, g):
    x, w1, b1, w2 = (t.double().requires_grad_(True) for t in (x, w1, b1, w2))
    z = x @ w1.t() + b1
    y = torch.nn.functional.gelu(z) @ w2.t()
    return torch.autograd.grad((y * g.double()).sum(), [x, w1, b1, w2]), z.detach()


def _raw(x, w1, b1, w2, g):
    """gaot_mlp2_bwd_f32 through the C ABI into results pre-filled with NaN"""
    from gaot_3d_amd import _lib, ops
    lib = _lib.load()
    rows, hid, oc = x.shape[0], w1.shape[0], w2.shape[0]
    outs = [torch.full(s, float("nan"), dtype=torch.float32, device=DEV) for s in ((rows, 32), (hid, 32), (hid,), (oc, hid))]
    ws = ops._ws(lib.gaot_mlp2_bwd_f32_workspace_bytes(hid, oc), DEV)
    rc = lib.gaot_mlp2_bwd_f32(ops._ptr(x), rows, 32, hid, oc, ops._ptr(w1), ops._ptr(b1), ops._ptr(w2), ops._ptr(g), *(ops._ptr(o) for o in outs),
                               ops._ptr(ws), ws.numel(), ops._stream())
    assert rc == 0, lib.gaot_last_error()
    return outs


def _chain(x, w1, b1, w2, g):
    """the same five products on the GEMM / activation kernels (precision 0), as MAGNODecoder._project_bwd runs them"""
    from gaot_3d_amd import ops
    m, hid, oc = x.shape[0], w1.shape[0], w2.shape[0]
    h, z = ops.gemm(x, w1, m, hid, 32, 32, 32, False, True, b1, ops.ACT["gelu"], want_preact=True, precision=0)
    dw2 = ops.gemm_dw(h, g, hid, 1, m, hid, 1, precision=0).view(1, hid) if oc == 1 else ops.gemm_dw(g, h, oc, hid, m, oc, hid, precision=0)
    a = ops.gemm(g, w2, m, hid, oc, oc, hid, False, False, precision=0)
    dz = ops.act_bwd(z, a, ops.ACT["gelu"])
    dw1 = ops.gemm_dw(dz, x, hid, 32, m, hid, 32, precision=0)
    db1 = ops.colsum(dz, m, hid, hid)
    dx = ops.gemm(dz, w1, m, 32, hid, hid, 32, False, False, precision=0)
    return dx, dw1, db1, dw2


def _dist(got, ref):
    return (got.detach().double().cpu() - ref).abs().max().item()


@pytest.mark.parametrize("hidden", HIDDEN)
def test_against_fp64_and_the_gemm_chain(hidden):
    from gaot_3d_amd import ops
    assert ops.mlp2_bwd_f32_supported(32, hidden, 1, ops.ACT["gelu"])
    worst = {n: (0.0, 0.0) for n in NAMES}
    for oc in OUTS:
        full = _operands(hidden, oc)
        dev_full = [t.to(DEV) for t in full]
        first33 = {}
        for rows in ROWS:
            x, w1, b1, w2, g = (t[:rows].contiguous() if t.shape[0] == 1000 else t for t in full)
            xd, w1d, b1d, w2d, gd = (t[:rows].contiguous() if t.shape[0] == 1000 else t for t in dev_full)
            refs, z = _fp64(x, w1, b1, w2, g)
            if rows == 1000:
                assert z.min() < -3.5 and z.max() > 3.5, (z.min(), z.max())
            got = _raw(xd, w1d, b1d, w2d, gd)
            n0 = ops.launch_count()
            again = ops.mlp2_backward_f32(xd, w1d, b1d, w2d, gd)
            assert ops.launch_count() == n0 + 2, (rows, oc)                       # the kernel and the fixed-order completion
            chain = _chain(xd, w1d, b1d, w2d, gd)
            for name, a, b, c, ref in zip(NAMES, got, again, chain, refs):
                assert not torch.isnan(a).any(), (name, rows, oc)
                assert torch.equal(a, b), (name, rows, oc)                        # two calls, bit for bit
                hb.check(f"mlp2_bwd_f32/h{hidden}/o{oc}/rows{rows}/{name}", a, ref, bar=FP32_BAR, quiet=True)
                peak = ref.abs().max().item()
                d_new, d_old = _dist(a, ref), _dist(c, ref)
                if d_new / peak >= worst[name][0]:
                    worst[name] = (d_new / peak, d_old / peak)
                assert d_new <= max(4.0 * d_old, 1e-6 * peak), (name, rows, oc, d_new, d_old, peak)
            if rows in (33, 1000):
                first33[rows] = got[0][:33].clone()
        assert torch.equal(first33[33], first33[1000]), oc                         # a row's d_x depends on that row alone
    for name in NAMES:
        print(f"[mlp2_bwd_f32] hidden {hidden} {name}: worst |kernel - fp64| = {worst[name][0]:.3e} of the peak "
              f"(the GEMM chain there: {worst[name][1]:.3e})")


def test_zero_rows_launch_nothing_and_give_zeros():
    from gaot_3d_amd import _lib, ops
    lib = _lib.load()
    assert lib.gaot_mlp2_bwd_f32_parts(0) == 0
    for hidden, oc in ((64, 1), (256, 4)):
        x, w1, b1, w2, g = (t.to(DEV) for t in _operands(hidden, oc))
        torch.cuda.synchronize()
        n0 = ops.launch_count()
        dx, dw1, db1, dw2 = ops.mlp2_backward_f32(x[:0], w1, b1, w2, g[:0])
        raw = _raw(x[:0], w1, b1, w2, g[:0])                                       # over the NaN pre-fill
        assert ops.launch_count() == n0
        assert dx.shape == (0, 32)
        for t, r, w in ((dw1, raw[1], w1), (db1, raw[2], b1), (dw2, raw[3], w2)):
            assert torch.equal(t, torch.zeros_like(w)) and torch.equal(r, torch.zeros_like(w))


def test_shapes_outside_the_family_are_refused_before_any_launch():
    from gaot_3d_amd import ops
    from gaot_3d_amd._lib import GaotError
    gelu = ops.ACT["gelu"]
    for hidden in HIDDEN:
        for oc in OUTS:
            assert ops.mlp2_bwd_f32_supported(32, hidden, oc, gelu)
    for bad in ((16, 256, 1, gelu), (64, 256, 1, gelu), (32, 96, 1, gelu), (32, 512, 1, gelu), (32, 32, 1, gelu), (32, 256, 0, gelu),
                (32, 256, 5, gelu), (32, 256, 1, ops.ACT["relu"]), (32, 256, 1, ops.ACT["none"]), (32, 256, 1, ops.ACT["gelu_tanh"])):
        assert not ops.mlp2_bwd_f32_supported(*bad), bad
    x, w1, b1, w2, g = (t.to(DEV) for t in _operands(256, 2))
    x = x[:100].contiguous()
    g = g[:100].contiguous()
    torch.cuda.synchronize()
    n0 = ops.launch_count()
    calls = [
        lambda: ops.mlp2_backward_f32(x, torch.zeros(96, 32, device=DEV), torch.zeros(96, device=DEV), torch.zeros(2, 96, device=DEV), g),
        lambda: ops.mlp2_backward_f32(x[:, :16].contiguous(), w1[:, :16].contiguous(), b1, w2, g),
        lambda: ops.mlp2_backward_f32(x, w1, b1, torch.zeros(5, 256, device=DEV), torch.zeros(100, 5, device=DEV)),
        lambda: ops.mlp2_backward_f32(x, w1, b1, w2, g[:50].contiguous()),                 # cotangent rows
        lambda: ops.mlp2_backward_f32(x, w1, b1[:100].contiguous(), w2, g),                # bias length
        lambda: ops.mlp2_backward_f32(x.double(), w1, b1, w2, g),                          # dtype
        lambda: ops.mlp2_backward_f32(x, w1.t(), b1, w2, g),                               # layout
        lambda: ops.mlp2_backward_f32(x.cpu(), w1, b1, w2, g),                             # host tensor
    ]
    for i, call in enumerate(calls):
        with pytest.raises(GaotError):
            call()
        assert ops.launch_count() == n0, i
