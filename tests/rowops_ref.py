"""fp64 restatements of the row / element kernels of csrc/rowops.hip and of the activation table of csrc/common.h (gaot_act_fwd /
gaot_act_grad), for tests/test_rowops_fp64_gpu.py.  Plain torch on the CPU, no GPU.  Every backward is written out as a formula (the
kernels' formulas, not autograd): tests/test_rowops_ref_cpu.py holds them against fp64 autograd of the forward formulas.

Inputs are taken as they are (fp32 tensors are widened, never re-rounded); results are fp64."""
from __future__ import annotations

import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_ref as BR  # noqa: E402

Tensor = torch.Tensor


def _d(t: Tensor) -> Tensor:
    return t.detach().double().cpu()


# ---- activations: ops.ACT name -> (f, f'), torch's default parameters --------------------------------------------------------------
ACT_NAMES = ("none", "gelu", "relu", "silu", "tanh", "leaky_relu", "elu", "sigmoid", "softplus", "selu", "relu6", "hardswish", "mish",
             "gelu_tanh")
PIECEWISE = ("relu", "leaky_relu", "relu6", "hardswish")     # no transcendental: exact up to a product's rounding
SELU_SCALE = 1.0507009873554804934193349852946
SELU_ALPHA = 1.6732632423543772848170429916717
GELU_TANH_K = math.sqrt(2.0 / math.pi)
GELU_TANH_C = 0.044715
SOFTPLUS_THRESHOLD = 20.0


def _sigmoid(v: Tensor) -> Tensor:
    return torch.sigmoid(v)                         # fp64: 1 / (1 + exp(-v)) keeps its relative accuracy in both tails


def _softplus(v: Tensor) -> Tensor:
    """F.softplus(beta=1, threshold=20): v itself above the threshold"""
    return torch.where(v > SOFTPLUS_THRESHOLD, v, torch.log1p(torch.exp(torch.clamp(v, max=SOFTPLUS_THRESHOLD))))


def act_grid() -> Tensor:
    """the points the activations are checked at (fp32): 4001 on [-20, 20], then the planted kinks, thresholds and tails -- +-0, +-1e-30,
    +-3 (hardswish), 6 (relu6), 20 and the next float above it (softplus's threshold), +-88 (exp at the end of fp32's range).
    n = 4012 is no multiple of the 256-thread block"""
    planted = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 3.0, -3.0, 6.0, 20.0, 0.0, 88.0, -88.0], dtype=torch.float32)
    planted[8] = torch.nextafter(torch.tensor(20.0), torch.tensor(float("inf")))
    return torch.cat([torch.linspace(-20.0, 20.0, 4001, dtype=torch.float32), planted])


def act(name: str, v: Tensor) -> Tensor:
    v = v.double()
    zero = torch.zeros_like(v)
    if name == "none":
        return v.clone()
    if name == "gelu":
        return 0.5 * v * torch.erfc(-v / math.sqrt(2.0))          # 1 + erf(t) = erfc(-t): no cancellation in the negative tail
    if name == "relu":
        return torch.where(v > 0, v, zero)
    if name == "silu":
        return v * _sigmoid(v)
    if name == "tanh":
        return torch.tanh(v)
    if name == "leaky_relu":
        return torch.where(v > 0, v, 0.01 * v)
    if name == "elu":
        return torch.where(v > 0, v, torch.expm1(torch.clamp(v, max=0.0)))
    if name == "sigmoid":
        return _sigmoid(v)
    if name == "softplus":
        return _softplus(v)
    if name == "selu":
        return SELU_SCALE * torch.where(v > 0, v, SELU_ALPHA * torch.expm1(torch.clamp(v, max=0.0)))
    if name == "relu6":
        return torch.where(v > 0, torch.where(v < 6, v, torch.full_like(v, 6.0)), zero)
    if name == "hardswish":
        return torch.where(v <= -3, zero, torch.where(v >= 3, v, v * (v + 3.0) / 6.0))
    if name == "mish":
        return v * torch.tanh(_softplus(v))
    if name == "gelu_tanh":
        u = GELU_TANH_K * (v + GELU_TANH_C * v ** 3)
        return v * _sigmoid(2.0 * u)                               # 0.5 (1 + tanh u) = sigmoid(2u)
    raise KeyError(name)


def act_grad(name: str, v: Tensor) -> Tensor:
    """d act / dv with torch autograd's choices at the kinks: relu'(0) = 0, leaky_relu'(0) = 0.01, elu'(0) = selu'(0)/scale/alpha = 1
    (the exponential branch), relu6' = 1 on the OPEN interval (0, 6), hardswish' = (2v + 3)/6 on the OPEN interval (-3, 3) (0 at -3,
    1 at 3: the outer one-sided values), softplus' = 1 above the threshold only"""
    v = v.double()
    one, zero = torch.ones_like(v), torch.zeros_like(v)
    if name == "none":
        return one
    if name == "gelu":
        return 0.5 * torch.erfc(-v / math.sqrt(2.0)) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)
    if name == "relu":
        return torch.where(v > 0, one, zero)
    if name == "silu":
        s = _sigmoid(v)
        return s * (1.0 + v * (1.0 - s))
    if name == "tanh":
        return 1.0 / torch.cosh(v) ** 2
    if name == "leaky_relu":
        return torch.where(v > 0, one, 0.01 * one)
    if name == "elu":
        return torch.where(v > 0, one, torch.exp(torch.clamp(v, max=0.0)))
    if name == "sigmoid":
        return _sigmoid(v) * _sigmoid(-v)
    if name == "softplus":
        return torch.where(v > SOFTPLUS_THRESHOLD, one, _sigmoid(v))
    if name == "selu":
        return SELU_SCALE * torch.where(v > 0, one, SELU_ALPHA * torch.exp(torch.clamp(v, max=0.0)))
    if name == "relu6":
        return torch.where((v > 0) & (v < 6), one, zero)
    if name == "hardswish":
        return torch.where(v <= -3, zero, torch.where(v >= 3, one, (2.0 * v + 3.0) / 6.0))
    if name == "mish":
        sp = _softplus(v)
        t = torch.tanh(sp)
        dsp = torch.where(v > SOFTPLUS_THRESHOLD, one, _sigmoid(v))
        return t + v * dsp / torch.cosh(sp) ** 2
    if name == "gelu_tanh":
        u = GELU_TANH_K * (v + GELU_TANH_C * v ** 3)
        du = GELU_TANH_K * (1.0 + 3.0 * GELU_TANH_C * v * v)
        s = _sigmoid(2.0 * u)
        return s + v * 2.0 * s * (1.0 - s) * du
    raise KeyError(name)


def act_bar(ref: Tensor, v: Tensor, abs_term: float = 4e-7) -> Tensor:
    """the activation bar: |got - ref| <= 4e-6 |ref| + 4e-7 max(1, |v|).  Relative part: __expf at |v| <= 20 (20 log2(e) 2^-24 = 1.7e-6
    on the exponent, used up to twice) plus a few ulps; absolute part: the cancellation in 1 + erf / 1 + tanh in the negative tail"""
    return 4e-6 * ref.abs() + abs_term * torch.clamp(v.double().abs(), min=1.0)


def linear_fwd(x: Tensor, w: Tensor, b: Tensor | None, name: str):
    """y = act(x W^T + b) -> (y, z)"""
    z = _d(x) @ _d(w).t()
    if b is not None:
        z = z + _d(b)
    return act(name, z), z


def linear_bwd(x: Tensor, w: Tensor, z: Tensor, dy: Tensor, name: str):
    """-> dx, dW, db of y = act(x W^T + b) from the pre-activation z"""
    dz = _d(dy) * act_grad(name, z)
    return dz @ _d(w), dz.t() @ _d(x), dz.sum(0)


# ---- RMSNorm -----------------------------------------------------------------------------------------------------------------------
def rmsnorm_fwd(x: Tensor, w: Tensor, eps: float):
    """-> (y, 1/rms); tests/block_ref.py states the op"""
    return BR.norm(_d(x), _d(w), eps)


def rmsnorm_bwd(x: Tensor, w: Tensor, eps: float, dy: Tensor, dx_add: Tensor | None = None, dx_add2: Tensor | None = None):
    """dx = r w dy - x r^3 mean(x w dy), then (dx + dx_add) + dx_add2 in the kernel's order; dw = sum over the rows of dy x r"""
    x, w, dy = _d(x), _d(w), _d(dy)
    r = torch.rsqrt(x.square().mean(-1, keepdim=True) + eps)
    c = (x * w * dy).sum(-1, keepdim=True) * r ** 3 / x.shape[-1]
    dx = r * w * dy - x * c
    if dx_add is not None:
        dx = dx + _d(dx_add)
    if dx_add2 is not None:
        dx = dx + _d(dx_add2)
    return dx, (dy * x * r).sum(0)


# ---- SwiGLU on a fused [rows, 2F] buffer: a = columns 0..F-1, g = columns F..2F-1 ---------------------------------------------------
def swiglu_fwd(ag: Tensor, f: int) -> Tensor:
    ag = _d(ag)
    a, g = ag[:, :f], ag[:, f:]
    return a * _sigmoid(a) * g


def swiglu_bwd(ag: Tensor, du: Tensor, f: int) -> Tensor:
    """-> d(a | g) = (du g silu'(a) | du silu(a))"""
    ag, du = _d(ag), _d(du)
    a, g = ag[:, :f], ag[:, f:]
    s = _sigmoid(a)
    return torch.cat([du * g * s * (1.0 + a * (1.0 - s)), du * a * s], dim=1)


# ---- RoPE --------------------------------------------------------------------------------------------------------------------------
def rope_freqs(head_dim: int) -> Tensor:
    """rotary_embedding_torch's fp32 frequencies 1 / 10000^(2i / head_dim)"""
    return 1.0 / (10000 ** (torch.arange(0, head_dim, 2).float() / head_dim))


def rope(x: Tensor, ld: int, col0: int, nheads: int, head_dim: int, seq_len: int, freqs: Tensor, inverse: bool = False) -> Tensor:
    """x [rows, ld]: the nheads heads of head_dim columns from col0 rotated pairwise (columns 2p, 2p + 1) by the angle of position
    row % seq_len; every other column untouched.  The angle is formed as the kernel and the reference form it -- fp32(pos) * fp32(freq),
    one fp32 product -- its cosine / sine and the rotation are fp64"""
    rows = x.shape[0]
    assert x.shape[1] == ld and freqs.dtype == torch.float32 and freqs.numel() == head_dim // 2
    out = _d(x).clone()
    pos = (torch.arange(rows) % seq_len).to(torch.float32)
    ang = (pos[:, None] * freqs.cpu()[None, :]).double()                    # fp32 product, widened
    cs, sn = torch.cos(ang)[:, None, :], torch.sin(ang)[:, None, :]
    if inverse:
        sn = -sn
    span = out[:, col0:col0 + nheads * head_dim].reshape(rows, nheads, head_dim // 2, 2)
    v0, v1 = span[..., 0], span[..., 1]
    rot = torch.stack([v0 * cs - v1 * sn, v1 * cs + v0 * sn], dim=-1)
    out[:, col0:col0 + nheads * head_dim] = rot.reshape(rows, nheads * head_dim)
    return out


def rope_pair_mass(x: Tensor, ld: int, col0: int, nheads: int, head_dim: int) -> Tensor:
    """|x0| + |x1| of the pair an element belongs to ([rows, ld]; 0 outside the rotated span)"""
    rows = x.shape[0]
    m = torch.zeros(rows, ld, dtype=torch.float64)
    span = _d(x)[:, col0:col0 + nheads * head_dim].reshape(rows, -1, 2).abs().sum(-1, keepdim=True)
    m[:, col0:col0 + nheads * head_dim] = span.expand(-1, -1, 2).reshape(rows, -1)
    return m


# ---- patchify (reference gaot_3d.py:199-202, 218-220) -------------------------------------------------------------------------------
def patchify(grid: Tensor, b: int, d: int, h: int, w: int, p: int, c: int) -> Tensor:
    """grid [b, d h w, c] -> tokens [b, (d/p)(h/p)(w/p), p^3 c] by view / permute"""
    return grid.reshape(b, d // p, p, h // p, p, w // p, p, c).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(b, -1, p ** 3 * c)


def unpatchify(tok: Tensor, b: int, d: int, h: int, w: int, p: int, c: int) -> Tensor:
    return tok.reshape(b, d // p, h // p, w // p, p, p, p, c).permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(b, d * h * w, c)


# ---- MSE, column sums, scale mix, axpy ---------------------------------------------------------------------------------------------
def mse_fwd(pred: Tensor, target: Tensor) -> Tensor:
    return (_d(pred) - _d(target)).square().mean()


def mse_bwd(pred: Tensor, target: Tensor, upstream: float) -> Tensor:
    return (_d(pred) - _d(target)) * (2.0 / pred.numel()) * upstream


def colsum(x: Tensor, n: int):
    """x [M, ld] -> (column sums of the first n columns, sum |x| of the same: the mass the error bound scales with)"""
    x = _d(x)[:, :n]
    return x.sum(0), x.abs().sum(0)


def colsum_chain(m: int) -> int:
    """the longest addition chain of gaot_colsum's two-stage order: a row lane adds every 8th row of its chunk (ceil(rpc / 8)), 8 row
    lanes are added in order (7), a part lane of k_reduce_parts adds every 32nd chunk (ceil(chunks / 32)), 32 part lanes in order
    (31, counting the additions to the zero the sums start from as exact).  chunks and rpc as gaot_colsum computes them"""
    chunks = min(256, max(1, -(-m // 64)))
    rpc = -(-m // chunks)
    return -(-rpc // 8) + 7 + -(-chunks // 32) + 31


def scale_mix_fwd(logits: Tensor, xs):
    """out = sum_s softmax(logits)_s x_s (reference magno.py:590-594) -> (out, weights)"""
    w = torch.softmax(_d(logits), dim=-1)
    return sum(w[:, s:s + 1] * _d(x) for s, x in enumerate(xs)), w


def scale_mix_bwd(logits: Tensor, xs, dout: Tensor):
    """-> (dlogits, [dx_s]): dx_s = w_s dout, dlogits_s = w_s (<dout, x_s> - sum_t w_t <dout, x_t>)"""
    w = torch.softmax(_d(logits), dim=-1)
    dout = _d(dout)
    gs = torch.stack([(dout * _d(x)).sum(-1) for x in xs], dim=-1)
    tot = (w * gs).sum(-1, keepdim=True)
    return w * (gs - tot), [w[:, s:s + 1] * dout for s in range(len(xs))]


def axpy(a: Tensor, b: Tensor, alpha: float, period: int) -> Tensor:
    """out[i] = a[i] + alpha b[i % period], alpha as the fp32 the kernel receives"""
    a, b = _d(a).flatten(), _d(b).flatten()
    al = float(torch.tensor(alpha, dtype=torch.float32))
    return (a + al * b[torch.arange(a.numel()) % period]).view(a.shape)
