"""K = 20 training steps of the drop-in model (HIP forward / backward, fused gaot_3d_amd.optim.AdamW, MixLRScheduler) against the
fp64 oracle trajectory (tests/trajectory_ref.py: the case, the metrics L / G / W / Gm / Gv and the yardsticks are defined there; their
teeth are in tests/test_trajectory_cpu.py), eager and as a replayed whole-step hipGraph, and through a checkpoint.

What only matters from the second step on, and is covered here: the device-resident step counter and learning rate of the fused AdamW
on the model's own gradients, AdamW.sync_lr() under graph replay, the dropout seed stream through K L attention calls (reserved per
Transformer.forward), the bf16 weight images and packs cached beside parameters the optimizer updates in place, the plain single-GPU
whole-step replay bench.py times, and the fused optimizer's own checkpoint.

Bounds:
  (a) fp32 mode: every metric <= the fp64 oracle's with uniform gradient noise of +-1e-5 x peak in every step and tensor (the larger of
      two realisations), margin 1x.
  (b) bf16 mode: every metric <= min(4 x weight-rounded fp64 oracle, 0.5 x the smaller of two other-seed fp64 trajectories).
  (c) replay == eager bit for bit (losses of every step, parameters, both moments); without sync_lr() the parameters differ.
  (d) checkpoint after K / 2 steps, fresh objects, resume == the uninterrupted run bit for bit; torch.optim.AdamW continues from the
      same file.

Achieved on the MI355X (the [train] lines of the parity log), beside the bound and the yardsticks of the same run; cpu32 = the fp32 CPU
oracle against the same fp64 trajectory, and the ratio of the HIP value to it:
                                     L         G         W         Gm        Gv
  (a) fp32, dropout 0     hip        7.49e-6   1.02e-4   1.44e-4   4.85e-5   5.47e-5
                          bound      4.94e-5   4.76e-3   1.23e-2   5.81e-4   1.70e-4
                          cpu32      1.33e-6   5.62e-5   1.29e-3   1.32e-5   3.54e-6
                          hip/cpu32  5.6x      1.8x      0.1x      3.7x      15.5x
  (a) fp32, dropout 0.1   hip        1.34e-5   8.12e-5   1.07e-4   4.54e-5   4.94e-5
                          bound      1.12e-4   4.57e-3   1.16e-2   6.50e-4   1.89e-4
                          cpu32      7.80e-7   4.27e-5   9.76e-4   1.78e-5   3.59e-6
                          hip/cpu32  17.2x     1.9x      0.1x      2.6x      13.8x
  (b) bf16, dropout 0.1   hip        5.91e-3   9.44e-2   2.91e-1   2.82e-2   1.26e-2
                          bound      1.18e-2   2.32e-1   3.88e-1   7.29e-2   3.69e-2
                          wround     4.38e-3   5.89e-2   9.69e-2   2.56e-2   9.23e-3     (the bound's 4 x part)
                          other seed 2.37e-2   4.65e-1   1.05e+0   1.46e-1   9.16e-2     (the bound's 0.5 x part: binds on L, G, Gm)
                          hip/cpu32  7575x     2212x     298x      1590x     3516x
      worst tensors of W in bf16: the decoder block's k_proj 0.291 and q_proj 0.268, then its w3 / w1 / w2 at 0.08 - 0.11.
  (c) fp32 and bf16: losses of all 20 steps, 48 parameter tensors and both moments bit-identical; without sync_lr() all 48 differ.
  (d) both halves' losses, parameters and moments bit-identical; torch.optim.AdamW's step K / 2 within the fused optimizer's bars.
The moments' bound in (b) is the same formula applied to Gm and Gv."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trajectory_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, K = 8192, T.K


@pytest.fixture(scope="module", autouse=True)
def _threads():
    """the oracle's fp64 step is fastest on 16 threads"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)


# ---- the HIP side -----------------------------------------------------------------------------------------------------------------
def _make(dropout):
    from gaot_3d_amd.model import init_model
    from gaot_3d_amd.optim import AdamW
    from gaot_3d_amd.schedule import MixLRScheduler
    cs = T.case(N)
    model = init_model(3, 1, "gaot_3d", T.config(dropout))
    model.load_state_dict(cs.sd0, strict=True)
    model = model.to(DEV).train()
    opt = AdamW(model.parameters(), lr=T.LR_ARGS[0], weight_decay=T.WEIGHT_DECAY)
    sch = MixLRScheduler(opt, K, *T.LR_ARGS)
    return model, opt, sch


def _step_fn(model, opt):
    """one training step as bench.py's: neighbour lists rebuilt, zero_grad, forward, MSE, backward, fused AdamW -> detached loss"""
    import gaot_3d_amd
    from gaot_3d_amd import functional as GF
    cs = T.case(N)
    batch, tokens = cs.batch.to(DEV), cs.tokens.to(DEV)

    def step():
        gaot_3d_amd.clear_graph_cache(batch)
        opt.zero_grad(set_to_none=True)
        loss = GF.mse_loss(model(batch=batch, tokens_pos=tokens), batch.x)
        loss.backward()
        loss = loss.detach()      # nothing of the step's autograd graph outlives the step
        opt.step()
        return loss
    return step


def _collect(model, opt, losses):
    """-> Trajectory (fp64 copies for the metrics) carrying .raw: the fp32 tensors themselves for the bit comparisons"""
    torch.cuda.synchronize()
    cs = T.case(N)
    named = {k: q for k, q in model.named_parameters() if q.requires_grad}
    assert list(named.keys()) == cs.names
    raw = dict(losses=torch.stack([v.reshape(()) for v in losses]).cpu(), params={k: q.detach().cpu().clone() for k, q in named.items()},
               exp_avg={k: opt.state[q]["exp_avg"].cpu().clone() for k, q in named.items()},
               exp_avg_sq={k: opt.state[q]["exp_avg_sq"].cpu().clone() for k, q in named.items()})
    steps = {float(opt.state[q]["step"]) for q in named.values()}
    assert len(steps) == 1, steps
    tr = T.Trajectory(raw["losses"].double().tolist(), {k: cs.sd0[k].double() for k in cs.names},
                      {k: v.double() for k, v in raw["params"].items()}, {k: v.double() for k, v in raw["exp_avg"].items()},
                      {k: v.double() for k, v in raw["exp_avg_sq"].items()}, steps.pop())
    tr.raw = raw
    return tr


def _run_eager(precision, dropout, first=0, last=K, objs=None):
    """steps [first, last) eagerly; ``objs`` = (model, opt, sch) to continue with (the dropout seed is then the caller's)"""
    import gaot_3d_amd
    from gaot_3d_amd import functional as GF
    model, opt, sch = objs if objs is not None else _make(dropout)
    if objs is None:
        GF.set_dropout_seed(T.SEED, DEV)
    step = _step_fn(model, opt)
    losses = []
    gaot_3d_amd.set_precision(precision)
    try:
        for _ in range(first, last):
            losses.append(step().clone())
            sch.step()
        torch.cuda.synchronize()
    finally:
        gaot_3d_amd.set_precision("fp32")
    return model, opt, sch, losses


def _run_graph(precision, dropout, sync_lr=True):
    """bench.measure's launch mode: step 0 eagerly on a side stream (allocates the optimizer state), ONE step captured, steps 1 .. K-1
    replayed; the host schedule reaches the captured step through sync_lr() only"""
    import gaot_3d_amd
    from gaot_3d_amd import functional as GF
    model, opt, sch = _make(dropout)
    GF.set_dropout_seed(T.SEED, DEV)
    step = _step_fn(model, opt)
    losses = []
    gaot_3d_amd.set_precision(precision)
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            losses.append(step().clone())
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        sch.step()
        if sync_lr:
            opt.sync_lr()
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph, capture_error_mode="global"):     # no try / except: a failed capture fails the test
            loss = step()
        graph.instantiate()
        torch.cuda.synchronize()
        assert float(next(iter(opt.state.values()))["step"]) == 1.0     # the capture recorded the step, it did not run it
        for _ in range(1, K):
            graph.replay()
            losses.append(loss.clone())
            sch.step()
            if sync_lr:
                opt.sync_lr()
        torch.cuda.synchronize()
    finally:
        gaot_3d_amd.set_precision("fp32")
    tr = _collect(model, opt, losses)
    del graph
    return tr


_EAGER: dict = {}


def _eager(precision, dropout):
    """the all-eager HIP trajectory, run once per process"""
    key = (precision, dropout)
    if key not in _EAGER:
        model, opt, _sch, losses = _run_eager(precision, dropout)
        _EAGER[key] = _collect(model, opt, losses)
    return _EAGER[key]


def _same(rep, name, got, want):
    """bit equality of two {name: tensor} sets (or two tensors); names the tensors that differ"""
    if torch.is_tensor(got):
        got, want = {"": got}, {"": want}
    bad = [k for k in want if not torch.equal(got[k], want[k])]
    ok = not bad
    text = f"[train] {rep.tag}/{name}: " + ("bit-identical" if ok else f"DIFFER in {len(bad)} of {len(want)}: " + ", ".join(
        f"{k or name} max|diff|={(got[k].double() - want[k].double()).abs().max().item():.3e}" for k in bad[:4]))
    print(text)
    if not ok:
        rep.failures.append(text)


# ---- (a), (b): eager against the fp64 oracle ------------------------------------------------------------------------------------------
def _against_oracle(tag, precision, dropout, bound, extra=""):
    ref = T.trajectory("fp64", N, K, dropout)
    cpu32 = T.metrics(T.trajectory("fp32", N, K, dropout), ref)
    hip = _eager(precision, dropout)
    m = T.metrics(hip, ref)
    rep = T.Report(tag)
    rep.line("fp64 losses " + " ".join(f"{v:.4f}" for v in ref.losses))
    rep.line("hip  losses " + " ".join(f"{v:.4f}" for v in hip.losses))
    rep.line("hip " + T.fmt(m))
    rep.line("bound " + T.fmt(bound) + extra)
    rep.line("fp32 cpu oracle " + T.fmt(cpu32))
    rep.line("hip / fp32 cpu oracle " + " ".join(f"{k}={m[k] / max(cpu32[k], 1e-300):.1f}x" for k in T.METRICS))
    rep.tensors(m)
    assert hip.step == K
    rep.check(m, bound)
    rep.done()


@pytest.mark.parametrize("dropout", [0.0, T.P_DROP], ids=["drop0", "drop0.1"])
def test_fp32_trajectory_vs_fp64_oracle(dropout):
    """(a): the fp32-mode trajectory stays within what the accepted one-step gradient error, propagated through the reference optimizer,
    does to the fp64 trajectory -- losses of every step, final parameters, both moments"""
    _against_oracle(f"traj fp32 drop{dropout:g}", "fp32", dropout, T.noise_yardstick(N, K, dropout))


def test_bf16_trajectory_vs_fp64_oracle():
    """(b): bf16 arithmetic moves training by at most four weight-rounding classes and by less than half of what another dropout seed does"""
    y = T.bf16_yardstick(N, K, T.P_DROP)
    _against_oracle(f"traj bf16 drop{T.P_DROP:g}", "bf16", T.P_DROP, y,
                    extra=" | weight-rounded " + T.fmt(y["wround"]) + " | other seed " + T.fmt(y["other_seed"]))


# ---- (c): whole-step replay ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_whole_step_graph_replay_equals_eager(precision):
    """(c): the single-GPU launch mode bench.py times computes the eager trajectory bit for bit: the counter, the learning rate (through
    sync_lr), the seed stream and every cached weight image follow the replays"""
    eager = _eager(precision, T.P_DROP)
    got = _run_graph(precision, T.P_DROP)
    rep = T.Report(f"traj replay {precision}")
    _same(rep, "losses", got.raw["losses"], eager.raw["losses"])
    for part in ("params", "exp_avg", "exp_avg_sq"):
        _same(rep, part, got.raw[part], eager.raw[part])
    assert got.step == K == eager.step, (got.step, eager.step)
    rep.done()
    # without sync_lr() the captured step keeps the learning rate of step 0: theta_1 (made with it) and so the losses of steps 0 and 1
    # are the eager run's, everything after is not
    stale = _run_graph(precision, T.P_DROP, sync_lr=False)
    assert torch.equal(stale.raw["losses"][:2], eager.raw["losses"][:2])
    assert not torch.equal(stale.raw["losses"][2], eager.raw["losses"][2])
    differ = [k for k in eager.raw["params"] if not torch.equal(stale.raw["params"][k], eager.raw["params"][k])]
    print(f"[train] traj replay {precision}/no sync_lr: {len(differ)} of {len(eager.raw['params'])} parameter tensors differ")
    assert len(differ) == len(eager.raw["params"])


# ---- (d): checkpoint ----------------------------------------------------------------------------------------------------------------
def test_checkpoint_resume_equals_uninterrupted(tmp_path):
    """(d): model + fused optimizer + scheduler state through torch.save after K / 2 steps into fresh objects, the seed stream re-entered
    at word (K / 2) L: the second half equals the uninterrupted run bit for bit; torch.optim.AdamW loads the same file (the state-dict
    layout gaot_3d_amd/optim.py claims) and its next step is the fused one's"""
    import gaot_3d_amd
    from gaot_3d_amd import functional as GF
    full = _eager("bf16", T.P_DROP)
    half = K // 2
    model, opt, sch, first = _run_eager("bf16", T.P_DROP, 0, half)
    path = tmp_path / "ckpt.pt"
    torch.save(dict(model=model.state_dict(), opt=opt.state_dict(), sch=sch.state_dict()), path)
    del model, opt, sch
    rep = T.Report("traj checkpoint bf16")
    _same(rep, "losses before", torch.stack([v.reshape(()) for v in first]).cpu(), full.raw["losses"][:half])

    ck = torch.load(path)
    steps = [float(st["step"]) for st in ck["opt"]["state"].values()]
    assert steps == [float(half)] * len(T.case(N).names), steps
    ptrs = {st["step"].untyped_storage().data_ptr() for st in ck["opt"]["state"].values()}
    assert len(ptrs) == len(steps)              # one counter per parameter, as torch.optim.AdamW writes and updates them

    model, opt, sch = _make(T.P_DROP)
    model.load_state_dict(ck["model"], strict=True)
    opt.load_state_dict(ck["opt"])
    sch.load_state_dict(ck["sch"])
    assert opt.param_groups[0]["lr"] == T.lr_list(K, *T.LR_ARGS)[half]
    GF.set_dropout_seed(GF.dropout_seed_sequence(T.SEED, K * T.LAYERS)[half * T.LAYERS], DEV)
    model, opt, sch, second = _run_eager("bf16", T.P_DROP, half, K, objs=(model, opt, sch))
    got = _collect(model, opt, first + second)
    _same(rep, "losses after", got.raw["losses"][half:], full.raw["losses"][half:])
    for part in ("params", "exp_avg", "exp_avg_sq"):
        _same(rep, part, got.raw[part], full.raw[part])
    assert got.step == K
    rep.done()

    # the same file into the reference's optimizer: step K / 2 taken by torch.optim.AdamW from the fused optimizer's gradients
    ma, oa, sa = _make(T.P_DROP)
    ma.load_state_dict(ck["model"], strict=True)
    oa.load_state_dict(torch.load(path)["opt"])
    sa.load_state_dict(ck["sch"])
    mb, _ob, _sb = _make(T.P_DROP)
    mb.load_state_dict(ck["model"], strict=True)
    ob = torch.optim.AdamW(mb.parameters(), lr=T.LR_ARGS[0], weight_decay=T.WEIGHT_DECAY, foreach=False)
    ob.load_state_dict(torch.load(path)["opt"])
    GF.set_dropout_seed(GF.dropout_seed_sequence(T.SEED, K * T.LAYERS)[half * T.LAYERS], DEV)
    _run_eager("bf16", T.P_DROP, half, half + 1, objs=(ma, oa, sa))
    for qa, qb in zip(ma.parameters(), mb.parameters()):
        qb.grad = None if qa.grad is None else qa.grad.clone()
    ob.step()
    torch.cuda.synchronize()
    assert ob.param_groups[0]["lr"] == T.lr_list(K, *T.LR_ARGS)[half]
    for (k, qa), qb in zip(ma.named_parameters(), mb.parameters()):
        if not qa.requires_grad:
            continue
        assert float(ob.state[qb]["step"]) == half + 1, (k, float(ob.state[qb]["step"]))
        # parameters: the bar of test_fused_adamw_matches_torch; moments: a few fp32 ulps of the tensor's peak (FMA contraction, lerp)
        assert torch.allclose(qb.detach(), qa.detach(), rtol=1e-6, atol=1e-7), (k, (qb - qa).abs().max().item())
        for part, tol in (("exp_avg", 2e-6), ("exp_avg_sq", 1e-5)):
            a, b = oa.state[qa][part], ob.state[qb][part]
            assert float((a - b).abs().max()) <= tol * float(a.abs().max()), (k, part, float((a - b).abs().max()), float(a.abs().max()))
