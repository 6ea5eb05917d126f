"""Teeth of tests/trajectory_ref.py, on the CPU: the criteria tests/test_trajectory_gpu.py applies to the HIP trajectories accept the
reference's own arithmetic and reject every optimizer / schedule / mask fault they are there for.  Reduced case: 4096 points (the
Transformer is unchanged: 64 tokens, L = 2), K = 10 steps, attention dropout 0.1; one pass of the file is twelve oracle trajectories
(17 s wall on 16 threads; printed as a ``[train]`` line when the module finishes).

The 0.5 x other-seed cap of the bf16 criterion is the fragile part of it on L: L is a maximum over the steps of a quantity that depends
on how the two mask sequences happen to differ at the loss spike of step 5.  Measured other-seed L, K = 10: 1.8e-2 / 2.5e-2 at 4096
points, but 3.6e-3 / 3.6e-2 at 2048 points (seeds 99 / 5) -- there the cap (1.8e-3) falls below the weight-rounded oracle's own L
(4.5e-3), which is why the reduced case is not smaller.  G and W of another seed are stable (0.37 - 0.40, 1.0 - 1.2 in all four).

Known blind spot: weight_decay 0 against 1e-5 is invisible to these metrics at K = 20 on the full case (G = 3e-6, far below the fp32
oracle's own 4.4e-5): lr x wd x K ~ 4e-7 of a weight.  The weight-decay term is pinned by test_fused_adamw_matches_torch (wd 1e-2)."""
import os
import sys
import time

import pytest
import torch

import golden_io as gio

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trajectory_ref as T  # noqa: E402

N, STEPS, DROP = 4096, 10, T.P_DROP
_T0 = time.perf_counter()


@pytest.fixture(scope="module", autouse=True)
def _threads():
    """the oracle's fp64 step is fastest on 16 threads (more only adds synchronisation on small tensors)"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)
    print(f"[train] trajectory cpu: {time.perf_counter() - _T0:.1f} s wall for the file")


def _ref():
    return T.trajectory("fp64", N, STEPS, DROP)


def _m(kind):
    return T.metrics(T.trajectory(kind, N, STEPS, DROP), _ref())


def test_schedule_restatement_equals_golden():
    """lr_list against the reference's per-epoch learning rates (golden lr_mix.npz) for the golden's own arguments, and against the
    product's MixLRScheduler for the arguments of the trajectory tests"""
    from gaot_3d_amd.schedule import MixLRScheduler
    meta, g = gio.load("lr_mix")
    for total in meta["totals"]:
        want = g["out"][f"lr_{total}"].double()
        got = T.lr_list(total, meta["lr"], meta["max_lr"], meta["min_lr"], meta["final_lr"], n=total + 2)
        assert torch.allclose(torch.tensor(got, dtype=torch.float64), want, rtol=1e-12, atol=0), total
    for total in (STEPS, T.K):
        opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=T.LR_ARGS[0])
        sch = MixLRScheduler(opt, total, *T.LR_ARGS)
        got = []
        for _ in range(total):
            got.append(opt.param_groups[0]["lr"])
            opt.step()
            sch.step()
        assert got == pytest.approx(T.lr_list(total, *T.LR_ARGS), rel=1e-12, abs=0)
        assert got[0] == T.LR_ARGS[0] and got[1] == T.LR_ARGS[1]     # one warm-up step, then the cosine phase starts at the maximum
    assert got[-1] == pytest.approx(T.LR_ARGS[3], rel=1e-12)        # K = 20: two exponential steps, the last at the final rate


def test_reference_trajectory_is_a_training_run():
    ref = _ref()
    assert ref.step == STEPS and len(ref.losses) == STEPS
    assert ref.losses[-1] < 0.8 * ref.losses[0], ref.losses
    assert set(ref.exp_avg.keys()) == set(ref.params.keys()) == set(T.case(N).names)
    assert all(float((ref.params[k] - ref.theta0[k]).norm()) > 0.0 for k in ref.params)     # every tensor moves: W is defined
    same = T.metrics(ref, ref)
    assert all(same[k] == 0.0 for k in T.METRICS)


def test_fp32_oracle_passes_the_fp32_criterion():
    """criterion (a) accepts the reference's own arithmetic in fp32"""
    y = T.noise_yardstick(N, STEPS, DROP)
    m = _m("fp32")
    rep = T.Report("cpu fp32 oracle vs fp64")
    rep.line("yardstick " + T.fmt(y))
    rep.check(m, y)
    rep.done()


def test_weight_rounded_oracle_passes_the_bf16_criterion():
    """criterion (b) accepts the class of bf16 rounding it is built from, and is far below what another dropout seed does"""
    y = T.bf16_yardstick(N, STEPS, DROP)
    m = _m("wround")
    rep = T.Report("cpu weight-rounded oracle vs fp64")
    rep.line("wround " + T.fmt(y["wround"]) + " | other seed " + T.fmt(y["other_seed"]))
    rep.check(m, y)
    rep.done()
    for k in ("L", "G", "W"):
        assert y[k] < y["other_seed"][k]


@pytest.mark.parametrize("fault", ["stale_lr", "step_ahead", "eps", "wd", "swap_masks"])
def test_faults_are_rejected_by_the_fp32_criterion(fault):
    """a learning rate that never reaches the step, a step counter one ahead, eps 1e-6, weight_decay 1e-2 (asserted through W only: decay acts on
    the norm weights, values near 1 that training moves little; G stays below the yardstick), a backward through another mask than its forward's"""
    y = T.noise_yardstick(N, STEPS, DROP)
    m = _m(fault)
    print(f"[train] cpu fault {fault}: {T.fmt(m)} | yardstick {T.fmt(y)} | worst tensor {m['worst']}")
    if fault == "wd":
        assert m["W"] > y["W"], (m["W"], y["W"])
    else:
        for k in ("L", "G", "W"):
            assert m[k] > y[k], (k, m[k], y[k])


def test_faults_are_rejected_by_the_bf16_criterion():
    """the wider bf16 bound still rejects the optimizer and mask faults (weight_decay 1e-2 is below it: an fp32-criterion catch only)"""
    y = T.bf16_yardstick(N, STEPS, DROP)
    for fault in ("stale_lr", "step_ahead", "eps", "swap_masks"):
        m = _m(fault)
        print(f"[train] cpu fault {fault} vs bf16 bound: {T.fmt(m)} | bound {T.fmt(y)}")
        assert any(m[k] > y[k] for k in ("L", "G", "W")), (fault, T.fmt(m), T.fmt(y))


def test_fused_adamw_state_dict_gives_every_parameter_its_own_step():
    """the live state of gaot_3d_amd.optim.AdamW shares ONE counter between all parameters (the device scalar the kernel reads);
    its state_dict must not: torch.optim.AdamW advances the ``step`` tensor of every parameter, so a shared one would count
    len(params) per step and feed each parameter another bias correction.  (The fused step itself needs the GPU:
    test_trajectory_gpu.py::test_checkpoint_resume_equals_uninterrupted.)"""
    from gaot_3d_amd.optim import AdamW
    gen = torch.Generator().manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(5, 3, generator=gen)) for _ in range(4)]
    opt = AdamW(ps, lr=1e-3, weight_decay=T.WEIGHT_DECAY)
    counter = torch.tensor([3.0])
    for q in ps:     # what three steps leave behind
        opt.state[q] = dict(step=counter, exp_avg=torch.randn(5, 3, generator=gen), exp_avg_sq=torch.rand(5, 3, generator=gen))
    sd = opt.state_dict()
    steps = [st["step"] for st in sd["state"].values()]
    assert all(s.dim() == 0 and s.dtype == torch.float32 and float(s) == 3.0 for s in steps)
    assert len({s.untyped_storage().data_ptr() for s in steps}) == len(ps)
    assert all(opt.state[q]["step"] is counter for q in ps)                      # the live state is untouched
    for st, q in zip(sd["state"].values(), ps):
        assert st["exp_avg"] is opt.state[q]["exp_avg"] and st["exp_avg_sq"] is opt.state[q]["exp_avg_sq"]
    a = [torch.nn.Parameter(q.detach().clone()) for q in ps]
    b = [torch.nn.Parameter(q.detach().clone()) for q in ps]
    want = torch.optim.AdamW(a, lr=1e-3, weight_decay=T.WEIGHT_DECAY, foreach=False)
    for q, src in zip(a, ps):     # the same state written the way torch does
        want.state[q] = dict(step=torch.tensor(3.0), exp_avg=opt.state[src]["exp_avg"].clone(), exp_avg_sq=opt.state[src]["exp_avg_sq"].clone())
    got = torch.optim.AdamW(b, lr=1e-3, weight_decay=T.WEIGHT_DECAY, foreach=False)
    got.load_state_dict(sd)
    for qa, qb in zip(a, b):
        qa.grad = torch.randn(5, 3, generator=gen)
        qb.grad = qa.grad.clone()
    want.step()
    got.step()
    for qa, qb in zip(a, b):
        assert float(got.state[qb]["step"]) == 4.0
        assert torch.equal(qa, qb)
