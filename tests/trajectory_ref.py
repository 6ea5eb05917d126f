"""Multi-step training trajectories of the CPU oracle and the metrics that compare a trajectory with the fp64 one (helpers of
tests/test_trajectory_gpu.py; their teeth: tests/test_trajectory_cpu.py).

The case is BASELINE configs[0] in shape (knn 8, latent 8 x 8 x 8, L = 2, rope, heads 8 / 8, F = 1024) on the learnable target of
test_training_loop_loss_decreases.  One step is zero_grad -> forward -> MSE -> backward (oracle/gaot_oracle.train_step_grads, unchanged)
-> torch.optim.AdamW(lr, weight_decay=1e-5, foreach=False); the learning rate of step k is the 'mix' schedule's for a run of ``steps``
steps (lr_list, a plain restatement checked against the reference's golden); with attention dropout the oracle is handed the masks of the
seed words [k L, (k + 1) L) of dropout_seed_sequence(1234, steps L) in block call order.

Reference: the oracle in fp64 (state dict, the batch's float tensors and the tokens cast to double).  Metrics of a trajectory against it:
  L = max over the steps of |loss - loss64| / loss64
  G = sqrt(sum_t ||theta_K - theta64_K||^2 / sum_t ||theta64_K - theta_0||^2)   over the trainable tensors t: error of the displacement
  W = max over t of ||theta_K - theta64_K|| / ||theta64_K - theta_0||
  Gm, Gv = sqrt(sum_t ||s_K - s64_K||^2 / sum_t ||s64_K||^2) for the two AdamW moments

Yardsticks (all CPU oracle trajectories):
  noise0 / noise1   fp64 whose gradients carry, in every step and tensor, uniform noise in +-1e-5 x that tensor's peak (two realisations of
                    a fixed generator): the project's one-step fp32 gradient bar (test_cfg0_vs_oracle) propagated through the reference
                    optimizer.  Bound of an fp32 trajectory: the larger of the two, per metric.
  wround            fp64 with every weight matrix (dim >= 2) rounded to bf16 for forward and backward, fp64 master copy
  seed99 / seed5    fp64 with another dropout seed
                    Bound of a bf16 trajectory: min(4 x wround, 0.5 x the smaller other-seed value), per metric.
Faults the metrics must reject: stale_lr (the learning rate never updated), step_ahead (step counter one ahead), eps (1e-6), wd
(weight_decay 1e-2), swap_masks (first block: backward through another mask than the forward's)."""
from __future__ import annotations

import contextlib
import math
import os
import sys
import time
import types
from typing import List, Optional

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import gaot_oracle as orc  # noqa: E402

Tensor = torch.Tensor

K = 20                                  # steps of the GPU case
LAYERS = 2
HEADS = 8
SEED = 1234
P_DROP = 0.1
LR_ARGS = (1e-3, 3e-3, 1e-4, 5e-5)      # initial, max, min, final learning rate of the 'mix' schedule
WEIGHT_DECAY = 1e-5
NOISE = 1e-5                            # the one-step fp32 gradient bar, relative to the tensor's peak
LATENT = (8, 8, 8)
METRICS = ("L", "G", "W", "Gm", "Gv")


# ---- schedule ---------------------------------------------------------------------------------------------------------------------
def lr_list(total: int, initial_lr: float, max_lr: float, min_lr: float, final_lr: float, n: Optional[int] = None) -> List[float]:
    """learning rates of scheduler steps 0 .. n-1 (default n = total) of the reference's 'mix' schedule: 2 % linear warm-up initial -> max,
    90 % cosine max -> min, the rest exponential min -> final, the warm-up and the exponential phase at least one step each (taken from
    the cosine phase); past the end the exponential continues"""
    warm, cos = int(0.02 * total), int(0.90 * total)
    exp = total - warm - cos
    if warm == 0:
        warm, cos = 1, cos - 1
    if exp == 0:
        exp, cos = 1, cos - 1
    out = []
    for e in range(total if n is None else n):
        if e < warm:
            out.append(initial_lr + (max_lr - initial_lr) * (e / max(1, warm - 1)))
        elif e < warm + cos:
            out.append(min_lr + (max_lr - min_lr) * (1.0 + math.cos(math.pi * (e - warm) / cos)) / 2.0)
        else:
            out.append(min_lr * (final_lr / min_lr) ** ((e - warm - cos) / max(1, exp - 1)))
    return out


# ---- the case ---------------------------------------------------------------------------------------------------------------------
def config(dropout: float):
    from gaot_3d_amd.model.layers.attn import AttentionConfig, FFNConfig, TransformerConfig
    from gaot_3d_amd.model.layers.magno import MAGNOConfig
    return types.SimpleNamespace(
        magno=MAGNOConfig(gno_coord_dim=3, lifting_channels=32, encoder_feature_attr="pos", mlp_type="linear",
                          use_geoembed=[True, False], neighbor_strategy="knn", k_neighbors=8, precompute_edges=True),
        transformer=TransformerConfig(patch_size=2, hidden_size=256, num_layers=LAYERS, positional_embedding="rope",
                                      attn_config=AttentionConfig(hidden_size=256, num_heads=HEADS, num_kv_heads=HEADS,
                                                                  atten_dropout=dropout),
                                      ffn_config=FFNConfig(hidden_size=1024)),
        latent_tokens=LATENT)


_CASES: dict = {}


def case(n_points: int = 8192):
    """-> namespace(n_points, sd0 (fp32 state dict of the seeded initial model), batch (CPU), tokens, names (trainable tensors))"""
    if n_points not in _CASES:
        from gaot_3d_amd.data import make_synthetic_sample
        from gaot_3d_amd.model import init_model
        cfg = config(0.0)
        torch.manual_seed(0)
        model = init_model(3, 1, "gaot_3d", cfg)
        batch, tokens = make_synthetic_sample(n_points, cfg.latent_tokens, k=8, in_normals=False, surface=False, seed=0)
        p = batch.pos
        batch.x = (torch.sin(3.0 * p[:, :1]) * torch.cos(2.0 * p[:, 1:2]) + 0.5 * p[:, 2:3]).contiguous()
        sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
        names = [k for k, q in model.named_parameters() if q.requires_grad]
        oracle_names = [k for k, v in sd0.items()
                        if v.is_floating_point() and k != "latent_tokens" and not k.endswith("rotary_emb.freqs")]
        assert sorted(names) == sorted(oracle_names), set(names) ^ set(oracle_names)
        _CASES[n_points] = types.SimpleNamespace(n_points=n_points, sd0=sd0, batch=batch, tokens=tokens, names=names)
    return _CASES[n_points]


def dropout_masks(seed: int, steps: int, k: int):
    """keep masks of step k's LAYERS attention calls after set_dropout_seed(seed): seed words [k L, (k + 1) L)"""
    from gaot_3d_amd.functional import dropout_seed_sequence
    s = (LATENT[0] // 2) * (LATENT[1] // 2) * (LATENT[2] // 2)
    words = dropout_seed_sequence(seed, steps * LAYERS)[k * LAYERS:(k + 1) * LAYERS]
    return [orc.dropout_keep_mask(w, 1, HEADS, s, P_DROP) for w in words]


# ---- trajectories -----------------------------------------------------------------------------------------------------------------
class Trajectory:
    """losses (python floats), theta0 / params / exp_avg / exp_avg_sq ({name: fp64 CPU tensor}), step (the optimizer's counter)"""

    def __init__(self, losses, theta0, params, exp_avg, exp_avg_sq, step, seconds=0.0):
        self.losses, self.theta0, self.params = [float(v) for v in losses], theta0, params
        self.exp_avg, self.exp_avg_sq, self.step, self.seconds = exp_avg, exp_avg_sq, float(step), seconds


def _d(t: Tensor) -> Tensor:
    return t.detach().double().cpu()


class _MaskMul(torch.autograd.Function):
    """att * fwd in the forward, the gradient through ``bwd``: a backward that regenerates another mask than its forward used"""

    @staticmethod
    def forward(ctx, att, fwd, bwd):
        ctx.save_for_backward(bwd)
        return att * fwd

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None


@contextlib.contextmanager
def _swapped_mask_sdpa():
    """orc.sdpa that accepts keep = (forward mask, backward mask)"""
    plain = orc.sdpa

    def sdpa(q, k, v, keep=None, p_drop=0.0):
        if not isinstance(keep, tuple):
            return plain(q, k, v, keep, p_drop)
        att = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(q.shape[-1]), dim=-1)
        return _MaskMul.apply(att, keep[0].to(att.dtype) / (1.0 - p_drop), keep[1].to(att.dtype) / (1.0 - p_drop)) @ v
    orc.sdpa = sdpa
    try:
        yield
    finally:
        orc.sdpa = plain


def oracle_trajectory(cs, steps: int, dtype=torch.float64, dropout: float = 0.0, seed: int = SEED, lrs=None, noise: Optional[int] = None,
                      round_weights: bool = False, eps: float = 1e-8, weight_decay: float = WEIGHT_DECAY, step_offset: int = 0,
                      swap_masks: bool = False) -> Trajectory:
    """``steps`` training steps of the oracle in ``dtype``.  noise: None, or the realisation index of the gradient noise (uniform in
    +-NOISE x the tensor's peak, generator seeded 1000 + index); round_weights: the wround yardstick; lrs / eps / weight_decay /
    step_offset / swap_masks: the faults."""
    t0 = time.perf_counter()
    cfg = config(dropout)
    lrs = lr_list(steps, *LR_ARGS) if lrs is None else lrs
    params = {k: cs.sd0[k].to(dtype).clone().requires_grad_(True) for k in cs.names}
    fixed = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in cs.sd0.items() if k not in params}
    batch = cs.batch.to("cpu")
    for k in batch.keys():
        v = getattr(batch, k)
        if torch.is_tensor(v) and v.is_floating_point():
            setattr(batch, k, v.to(dtype))
    tokens = cs.tokens.to(dtype)
    opt = torch.optim.AdamW(list(params.values()), lr=lrs[0], eps=eps, weight_decay=weight_decay, foreach=False)
    if step_offset:
        for q in params.values():
            opt.state[q] = dict(step=torch.tensor(float(step_offset)), exp_avg=torch.zeros_like(q), exp_avg_sq=torch.zeros_like(q))
    gen = torch.Generator().manual_seed(1000 + noise) if noise is not None else None
    p_eff = orc.dropout_threshold(P_DROP) / 65536.0
    losses = []
    with (_swapped_mask_sdpa() if swap_masks else contextlib.nullcontext()):
        for k in range(steps):
            sd = dict(fixed)
            for name, q in params.items():
                w = q.detach()
                sd[name] = w.to(torch.bfloat16).to(dtype) if (round_weights and w.dim() >= 2) else w
            drop = None
            if dropout > 0.0:
                masks = dropout_masks(seed, steps, k)
                if swap_masks:
                    masks[0] = (masks[0], dropout_masks(seed + 1, steps, k)[0])
                drop = (masks, p_eff)
            _, loss, grads = orc.train_step_grads(sd, cfg, batch, tokens, drop=drop)
            for name, q in params.items():
                g = grads.get(name)
                if g is not None and gen is not None:
                    u = torch.rand(g.shape, generator=gen, dtype=torch.float64).to(g.dtype) * 2.0 - 1.0
                    g = g + u * (NOISE * float(g.abs().max()))
                q.grad = g
            for group in opt.param_groups:
                group["lr"] = lrs[k]
            opt.step()
            losses.append(float(loss))
    st = {name: opt.state[q] for name, q in params.items() if q in opt.state and len(opt.state[q])}
    return Trajectory(losses, {k: _d(cs.sd0[k]) for k in cs.names}, {k: _d(q) for k, q in params.items()},
                      {k: _d(s["exp_avg"]) for k, s in st.items()}, {k: _d(s["exp_avg_sq"]) for k, s in st.items()},
                      max((float(s["step"]) for s in st.values()), default=0.0), time.perf_counter() - t0)


_KINDS = {
    "fp64": {},
    "fp32": dict(dtype=torch.float32),
    "noise0": dict(noise=0),
    "noise1": dict(noise=1),
    "wround": dict(round_weights=True),
    "seed99": dict(seed=99),
    "seed5": dict(seed=5),
    "stale_lr": dict(lrs="stale"),
    "step_ahead": dict(step_offset=1),
    "eps": dict(eps=1e-6),
    "wd": dict(weight_decay=1e-2),
    "swap_masks": dict(swap_masks=True),
}
_TRAJ: dict = {}


def trajectory(kind: str, n_points: int, steps: int, dropout: float) -> Trajectory:
    """the oracle trajectory ``kind`` (a key of _KINDS) of the case, computed once per process"""
    key = (kind, n_points, steps, dropout)
    if key not in _TRAJ:
        kw = dict(_KINDS[kind])
        if kw.get("lrs") == "stale":
            kw["lrs"] = [lr_list(steps, *LR_ARGS)[0]] * steps
        _TRAJ[key] = oracle_trajectory(case(n_points), steps, dropout=dropout, **kw)
    return _TRAJ[key]


# ---- metrics ----------------------------------------------------------------------------------------------------------------------
def _ratio(num: float, den: float) -> float:
    return 0.0 if num == 0.0 else (num / den if den > 0.0 else float("inf"))


def metrics(traj: Trajectory, ref: Trajectory) -> dict:
    """-> dict(L, G, W, Gm, Gv, loss_rel (per step), per_tensor {name: ||err|| / ||displacement||}, worst (the tensor of W))"""
    assert len(traj.losses) == len(ref.losses), (len(traj.losses), len(ref.losses))
    loss_rel = [abs(a - b) / b if math.isfinite(a) else float("inf") for a, b in zip(traj.losses, ref.losses)]
    e2 = d2 = 0.0
    per = {}
    for k, r in ref.params.items():
        err = float((traj.params[k] - r).norm()) if bool(torch.isfinite(traj.params[k]).all()) else float("inf")
        disp = float((r - ref.theta0[k]).norm())
        e2, d2 = e2 + err * err, d2 + disp * disp
        per[k] = _ratio(err, disp)
    out = dict(L=max(loss_rel), G=_ratio(math.sqrt(e2), math.sqrt(d2)), W=max(per.values()), loss_rel=loss_rel, per_tensor=per,
               worst=max(per, key=per.get))
    for key, got, want in (("Gm", traj.exp_avg, ref.exp_avg), ("Gv", traj.exp_avg_sq, ref.exp_avg_sq)):
        assert set(got.keys()) == set(want.keys()), set(got.keys()) ^ set(want.keys())
        e2 = sum(float((got[k] - want[k]).norm()) ** 2 for k in want)
        out[key] = _ratio(math.sqrt(e2), math.sqrt(sum(float(want[k].norm()) ** 2 for k in want)))
        if not math.isfinite(out[key]):
            out[key] = float("inf")
    return out


def fmt(m: dict) -> str:
    return " ".join(f"{k}={m[k]:.3e}" for k in METRICS)


def noise_yardstick(n_points: int, steps: int, dropout: float) -> dict:
    """bound of an fp32 trajectory: per metric the larger of the two gradient-noise realisations"""
    ref = trajectory("fp64", n_points, steps, dropout)
    ms = [metrics(trajectory(f"noise{i}", n_points, steps, dropout), ref) for i in (0, 1)]
    return {k: max(m[k] for m in ms) for k in METRICS}


def bf16_yardstick(n_points: int, steps: int, dropout: float) -> dict:
    """bound of a bf16 trajectory: min(4 x wround, 0.5 x the smaller other-seed value) per metric; also returns the two parts"""
    ref = trajectory("fp64", n_points, steps, dropout)
    yw = metrics(trajectory("wround", n_points, steps, dropout), ref)
    ys = [metrics(trajectory(s, n_points, steps, dropout), ref) for s in ("seed99", "seed5")]
    out = {k: min(4.0 * yw[k], 0.5 * min(m[k] for m in ys)) for k in METRICS}
    out["wround"] = {k: yw[k] for k in METRICS}
    out["other_seed"] = {k: min(m[k] for m in ys) for k in METRICS}
    return out


class Report:
    """the checks of one trajectory, in the style of block_ref.Report: every metric prints one ``[train]`` line with the achieved value
    and its bound, done() fails with the list of every metric that missed"""

    def __init__(self, tag: str):
        self.tag, self.failures = tag, []

    def line(self, text: str):
        print(f"[train] {self.tag}: {text}")

    def check(self, m: dict, bound: dict, keys=METRICS):
        for k in keys:
            ok = m[k] <= bound[k]
            extra = f" worst tensor {m['worst']}" if k == "W" else ""
            text = f"[train] {self.tag}/{k}: {m[k]:.3e} (bound {bound[k]:.3e}){extra}{'' if ok else '  MISSED'}"
            print(text)
            if not ok:
                self.failures.append(text)
        for i, v in enumerate(m["loss_rel"]):   # every step's loss within the bound on L (the same condition as L, named step by step)
            if not v <= bound["L"]:
                self.failures.append(f"[train] {self.tag}/loss[{i}]: rel err {v:.3e} (bound {bound['L']:.3e})  MISSED")

    def tensors(self, m: dict, top: int = 5):
        worst = sorted(m["per_tensor"].items(), key=lambda kv: -kv[1])[:top]
        self.line("largest per-tensor ||err|| / ||displacement||: " + ", ".join(f"{k} {v:.3e}" for k, v in worst))

    def done(self):
        assert not self.failures, f"{len(self.failures)} check(s) missed:\n" + "\n".join(self.failures)
