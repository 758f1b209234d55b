"""FusedAdam (pepflowww_amd/optim.py, csrc/optimizer.hip) on the GPU against the float64 oracle (optim_oracle.py) on the shared cases
(optim_cases.py).

The tolerance of every value check is not a chosen number: per tensor and step the reference block -- torch.optim.Adam / AdamW with the
NaN loop and clip_grad_norm_, fp32, CPU -- runs ONE step from the kernel's own fp32 state before the step; its max |deviation| from the
oracle, times 4, plus one fp32 ulp of the tensor's largest magnitude is what the kernel may deviate (optim_cases.check_step).

Measured on the MI355X (max |deviation| from the oracle: kernel / torch reference / tolerance; the worst ratio to the tolerance per
configuration of test_values_follow_the_oracle):
    adam_ref   step 4  "zero"   p   7.4e-11 / 7.4e-11 / 4.1e-10   (0.18)
    adam_l2    step 2  "zero"   p   1.2e-10 / 1.3e-10 / 6.4e-10   (0.19)
    adamw      step 2  "small"  p   1.5e-10 / 1.7e-10 / 9.2e-10   (0.17)
    noclip     step 4  "small"  p   1.3e-10 / 1.3e-10 / 7.4e-10   (0.18)
    whole iteration as one graph, replay 0, ga_encoder.trunk.ipa_2.linear_out.weight  p  3.8e-9 / 3.8e-9 / 2.3e-8  (0.17)
    (the backward's gradients differ in their last bits from run to run, and with them the tensor this lands on: another run gave
    ga_encoder.trunk.ipa_3.linear_kv.weight, 1.5e-8 / 1.5e-8 / 9.0e-8, again 0.17)
The tests print these figures (-s)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import optim_cases as OC  # noqa: E402
import optim_oracle as OO  # noqa: E402
import gpu_util as G  # noqa: E402
import pepflowww_amd  # noqa: E402
from pepflowww_amd import synth  # noqa: E402
from pepflowww_amd.optim import FusedAdam  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_record(rec, config):
    c = OC.CONFIGS[config]
    g = [None if x is None else x.numpy() for x in OC.make_grads(rec["step"])]
    o = OO.step(rec["before"][0], g, rec["before"][1], rec["before"][2], rec["before"][3], rec["lr"], OC.BETAS, OC.EPS,
                c["weight_decay"], c["decoupled"], c["max_norm"])
    ref = OC.torch_one_step(rec["before"], g, rec["lr"], c["weight_decay"], c["decoupled"], c["max_norm"])
    rows = OC.check_step(rec["after"], o, ref, OC.NAMES, what=(config, rec["step"]))
    assert rec["after"][3] == o["steps"], (config, rec["step"], rec["after"][3], o["steps"])
    return o, rows


@pytest.mark.parametrize("config", list(OC.CONFIGS))
def test_values_follow_the_oracle(config):
    """Six steps (clip inactive / mild / strong, NaN entries, an all-zero gradient on warm moments, lr halved through param_groups
    before step 3, a parameter without gradient, a 4-byte-aligned view, numel 1 / 3 / chunk +- 1): p, exp_avg, exp_avg_sq after every
    step under the rule above; grad_norm to 4 ulp of fp32 (the kernel forms it in float64 and rounds once; clip_grad_norm_'s own fp32
    norm of norms is that far from it), nan_count exactly; no host read inside step()."""
    recs, opt, params = OC.run_fused(config, G.dev())
    worst = (0.0, None)
    for rec in recs:
        o, rows = _check_record(rec, config)
        for name, q, d_k, d_r, tol in rows:
            if tol > 0 and d_k / tol > worst[0]:
                worst = (d_k / tol, (rec["step"], name, q, d_k, d_r, tol))
        assert rec["nan_count"] == o["nan_count"] and rec["skipped"] == 0
        assert abs(rec["grad_norm"] - o["grad_norm"]) <= 4 * OC.ulp32(o["grad_norm"]), (rec["step"], rec["grad_norm"], o["grad_norm"])
    print(f"{config}: worst kernel deviation / tolerance = {worst[0]:.3f} at (step, tensor, quantity, kernel, reference, tolerance) = {worst[1]}")
    i = OC.NAMES.index("no_grad")
    assert recs[-1]["after"][3][i] == 0 and np.array_equal(_bits(recs[-1]["after"][0][i]), _bits(recs[0]["before"][0][i]))
    assert recs[-1]["after"][3][0] == len(OC.SCALES)
    assert any(r["nan_count"] > 0 for r in recs)
    # gradients are read-only: the NaN entries are still there and nothing was rescaled
    for p, g in zip(params, OC.make_grads(len(OC.SCALES) - 1)):
        assert g is None or np.array_equal(_bits(p.grad.cpu().numpy()), _bits(g.numpy()))


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_inf_gradient_skips_the_whole_step(sign):
    config = "adam_ref"
    recs, opt, params = OC.run_fused(config, G.dev(), n_steps=2)
    grads = [None if g is None else g.clone() for g in OC.make_grads(2)]
    grads[OC.NAMES.index("chunks")].view(-1)[OC.CHUNK + 17] = sign * float("inf")
    for p, g in zip(params, grads):
        p.grad = None if g is None else g.to(G.dev())
    keep = [p.detach().clone() for p in params] + [opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.steps.clone()]
    opt.step()
    now = [p.detach() for p in params] + [opt.exp_avg, opt.exp_avg_sq, opt.steps]
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(keep, now))
    assert int(opt.skipped_steps) == 1 and float(opt.last_grad_norm) == float("inf") and int(opt.last_nan_count) == 0
    # the next finite step is the oracle's step with the UN-advanced counters
    recs2, _, _ = OC.run_fused(config, G.dev(), n_steps=1, opt=opt, params=params, first_step=2)
    assert recs2[0]["before"][3][0] == 2 and recs2[0]["after"][3][0] == 3 and recs2[0]["skipped"] == 1
    _check_record(recs2[0], config)


def test_runs_are_bit_identical_and_tensors_independent():
    """The same six steps twice: every buffer bit-equal.  Two extra tensors in FRONT of the table (chunk indices, state offsets and
    the reduction's partial order all shift) leave the original tensors' bits unchanged; without a clip, since the clip coefficient --
    a function of the total norm -- is the one coupling between tensors."""
    a, _, _ = OC.run_fused("adam_l2", G.dev())
    b, _, _ = OC.run_fused("adam_l2", G.dev())
    for ra, rb in zip(a, b):
        assert ra["grad_norm"] == rb["grad_norm"]
        for q in range(3):
            assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(ra["after"][q], rb["after"][q])), (ra["step"], q)
    g = torch.Generator().manual_seed(77)
    extra = [(torch.randn(7, generator=g), torch.randn(7, generator=g)),
             (torch.randn(OC.CHUNK + 3, generator=g), torch.randn(OC.CHUNK + 3, generator=g))]
    c, _, _ = OC.run_fused("noclip", G.dev())
    d, opt, _ = OC.run_fused("noclip", G.dev(), extra=extra)
    assert len(opt._params) == len(OC.NAMES) + 2
    for rc, rd in zip(c, d):
        for q in range(3):
            assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(rc["after"][q], rd["after"][q])), (rc["step"], q)


def test_checkpoint_round_trip_with_torch_adam():
    config = "adam_ref"
    _, topt, tparams = OC.run_torch(config, n_steps=3)
    params = OC.make_params(G.dev())
    with torch.no_grad():
        for p, t in zip(params, tparams):
            p.copy_(t)
    c = OC.CONFIGS[config]
    opt = FusedAdam(params, lr=1.0, max_grad_norm=c["max_norm"])
    opt.load_state_dict(topt.state_dict())
    assert opt.param_groups[0]["lr"] == OC.LR and opt.steps.tolist() == [3] * (len(params) - 1) + [0]
    recs, _, _ = OC.run_fused(config, G.dev(), n_steps=2, opt=opt, params=params, first_step=3)
    for rec in recs:
        _check_record(rec, config)
    back = torch.optim.Adam([p.detach().cpu().clone().requires_grad_() for p in params], lr=1.0)
    back.load_state_dict(opt.state_dict())
    for bp, p in zip(back.param_groups[0]["params"], params):
        st, mine = back.state[bp], opt.state[p]
        assert float(st["step"]) == float(mine["step"]) and st["step"].dtype == torch.float32
        assert torch.equal(st["exp_avg"], mine["exp_avg"].cpu()) and torch.equal(st["exp_avg_sq"], mine["exp_avg_sq"].cpu())
    assert back.param_groups[0]["lr"] == opt.param_groups[0]["lr"] == OC.LR * 0.5


def test_scheduler_lowers_the_lr_of_the_next_step():
    config = "noclip"
    recs, opt, params = OC.run_fused(config, G.dev(), n_steps=1)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.8, patience=0)
    sched.step(1.0)
    sched.step(2.0)                                                      # a rising loss
    assert opt.param_groups[0]["lr"] == pytest.approx(OC.LR * 0.8)
    recs, _, _ = OC.run_fused(config, G.dev(), n_steps=1, opt=opt, params=params, first_step=1)
    assert recs[0]["lr"] == pytest.approx(OC.LR * 0.8)
    _check_record(recs[0], config)                                       # the oracle's step with the lowered lr ...
    with pytest.raises(AssertionError):                                  # ... and not with the old one
        _check_record(dict(recs[0], lr=OC.LR), config)


def test_whole_iteration_as_one_graph(seeded_sd):
    """GraphedTrainStep(..., optimizer=FusedAdam): one replay = forward, backward, NaN guard, clip, Adam.  Three replays: all 407
    parameters after a replay equal the oracle's update of (parameters before, the static gradients the replay left) under the rule
    above; the losses of replay k equal those of a step WITHOUT optimizer on a model copy holding the same parameter values, bit for
    bit; optimizer=None captures what the class always captured: one C-ABI call fewer than with the optimizer, losses bit-equal, and
    on the first replay its gradients equal those the graph with the optimizer left.  Those gradients cannot be asked to be bit-equal:
    two replays of ONE captured step on the same inputs differ in the last bits of 350 of the 407 gradients (measured on the MI355X:
    the weight gradients are accumulated atomically), so they are held to the bound test_graphed_training_step_equals_eager uses
    between the graph and the eager step, 1e-5 of the tensor's maximum + 1e-6."""
    from oracle import pepflow_oracle as O
    from pepflowww_amd.train_step import GraphedTrainStep
    dev = G.dev()
    B, L = 2, 32
    w = O.LOSS_WEIGHTS

    def model():
        m = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
        m.load_state_dict(seeded_sd, strict=True)
        return m.to(dev).train()

    def inputs(seed):
        batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in synth.make_pocket_batch(B, L, 6, seed=seed).items()}
        nz = synth.make_noise(B, L, 1, seed=seed + 1)
        noise = {"t": torch.rand(B, 1, generator=torch.Generator().manual_seed(seed)), **{k: nz[k] for k in ("trans0", "rot0", "ang0", "simplex0")}}
        return batch, noise

    m1, m2 = model(), model()
    names = [n for n, _ in m1.named_parameters()]
    assert len(names) == 407
    opt = FusedAdam(m1.parameters(), lr=5e-4, max_grad_norm=100.0)
    b0, n0 = inputs(31)
    plain = GraphedTrainStep(m2, b0, w, optimizer=None)
    step = GraphedTrainStep(m1, b0, w, optimizer=opt)
    assert step.n_launches == plain.n_launches + 1 and plain.optimizer is None
    assert all(torch.equal(a, b) for a, b in zip(m1.parameters(), m2.parameters()))      # capturing ran no update
    params = list(m1.parameters())
    worst = (0.0, None)
    for k, (batch, noise, seed) in enumerate(((b0, n0, 1234), (*inputs(57), 99), (*inputs(83), 7))):
        with torch.no_grad():
            for p2, p1 in zip(m2.parameters(), params):
                p2.copy_(p1)
        before = ([OC._np(p) for p in params], [OC._np(opt.state[p]["exp_avg"]) for p in params],
                  [OC._np(opt.state[p]["exp_avg_sq"]) for p in params], opt.steps.tolist())
        l1 = {q: v.clone() for q, v in step(batch, noise=noise, seed=seed).items()}
        l2 = plain(batch, noise=noise, seed=seed)
        for q in l1:
            assert torch.equal(l1[q], l2[q]), (k, q, l1[q].item(), l2[q].item())
        grads = [None if step.grads.get(n) is None else OC._np(step.grads[n]) for n in names]
        if k == 0:
            for n in names:
                ga, gb = step.grads.get(n), plain.grads.get(n)
                assert (ga is None) == (gb is None)
                # (gradients that are accumulated atomically may differ in the last bits between two runs: the bound of
                # test_graphed_training_step_equals_eager)
                assert ga is None or float((ga - gb).abs().max()) <= 1e-5 * float(gb.abs().max()) + 1e-6, n
        after = ([OC._np(p) for p in params], [OC._np(opt.state[p]["exp_avg"]) for p in params],
                 [OC._np(opt.state[p]["exp_avg_sq"]) for p in params])
        o = OO.step(before[0], grads, before[1], before[2], before[3], 5e-4, OC.BETAS, OC.EPS, 0.0, False, 100.0)
        ref = OC.torch_one_step(before, grads, 5e-4, max_norm=100.0)
        rows = OC.check_step(after, o, ref, names, what=("graph", k))
        for name, q, d_k, d_r, tol in rows:
            if tol > 0 and d_k / tol > worst[0]:
                worst = (d_k / tol, (k, name, q, d_k, d_r, tol))
        assert opt.steps.tolist() == o["steps"] and abs(float(opt.last_grad_norm) - o["grad_norm"]) <= 4 * OC.ulp32(o["grad_norm"])
        assert any(not np.array_equal(a, b) for a, b in zip(after[0], before[0]))           # the replay did update
    assert int(opt.skipped_steps) == 0 and opt.steps.tolist() == [3 if g is not None else 0 for g in grads]
    print(f"graphed iteration: worst kernel deviation / tolerance = {worst[0]:.3f} at {worst[1]}")
