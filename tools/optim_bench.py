"""Times the optimizer block of a training iteration on the full 407-parameter model with the gradients of one real step:

  (a) the reference's block (train.py:135-146): the per-parameter NaN loop, clip_grad_norm_, torch.optim.Adam.step() at its defaults;
  (b) pepflowww_amd.optim.FusedAdam.step() (csrc/optimizer.hip).

Both are timed with a host clock around `--calls` calls that end in a device synchronise, after `--warmup` calls; the two paths
alternate in one process for `--rounds` rounds and the min - max spread is reported.  For (b) also the device-event time and the
achieved bytes/s against the traffic of the update pass (read p, g, m, v, write p, m, v: 7 x 4 bytes per element, about 190 MB; the
norm pass reads g once more, 8 x 4 with it).  With --graph also the per-iteration time of GraphedTrainStep at B x L with and without
the captured optimizer.  Needs a ROCm device; prints one JSON line.

    python tools/optim_bench.py [--calls 50] [--warmup 5] [--rounds 3] [--graph 16x128] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pepflowww_amd  # noqa: E402
from pepflowww_amd import synth  # noqa: E402
from pepflowww_amd.optim import FusedAdam  # noqa: E402
from pepflowww_amd.train_step import GraphedTrainStep  # noqa: E402

WEIGHTS = {"trans_loss": 0.5, "rot_loss": 0.5, "bb_atom_loss": 0.25, "seqs_loss": 1.0, "angle_loss": 1.0, "torsion_loss": 0.5}
MAX_NORM = 100.0


def model_on(dev):
    m = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
    m.load_state_dict(synth.seeded_state_dict())
    return m.to(dev).train()


def reference_block(params, opt):
    for p in params:
        if p.grad is not None:
            if torch.isnan(p.grad).any():
                p.grad[torch.isnan(p.grad)] = 0
    torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
    opt.step()


def host_time(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def event_time(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--graph", default="16x128")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "optim_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    # gradients of one real step (B = 2, L = 32 is enough: the optimizer's work does not depend on the batch)
    m = model_on(dev)
    batch = {k: v.to(dev) for k, v in synth.make_pocket_batch(2, 32, 6, seed=31).items()}
    step = GraphedTrainStep(m, batch, WEIGHTS)
    step(batch, seed=1)
    grads = [None if p.grad is None else p.grad.detach().clone() for p in m.parameters()]
    del step
    pa = [p.detach().clone().requires_grad_() for p in m.parameters()]
    pb = [p.detach().clone().requires_grad_() for p in m.parameters()]
    for ps in (pa, pb):
        for p, g in zip(ps, grads):
            p.grad = None if g is None else g.clone()
    numel = sum(p.numel() for p, g in zip(pb, grads) if g is not None)
    ref = torch.optim.Adam(pa, lr=5e-4)
    fused = FusedAdam(pb, lr=5e-4, max_grad_norm=MAX_NORM)
    ta, tb = [], []
    for _ in range(args.rounds):
        ta.append(host_time(lambda: reference_block(pa, ref), args.calls, args.warmup))
        tb.append(host_time(fused.step, args.calls, args.warmup))
    tb_ev = event_time(fused.step, args.calls, args.warmup)
    tb_launch = event_time(fused.launch, args.calls, args.warmup)          # the three launches alone (what a graph replays)
    traffic = 7 * 4 * numel
    out = {"parameters": len(pb), "elements_with_gradient": numel, "calls": args.calls, "warmup": args.warmup,
           "reference_block_ms_host": {"min": min(ta), "max": max(ta), "rounds": ta},
           "fused_step_ms_host": {"min": min(tb), "max": max(tb), "rounds": tb},
           "fused_step_ms_device_events": tb_ev, "fused_launch_only_ms_device_events": tb_launch,
           "update_pass_traffic_bytes": traffic, "traffic_with_norm_pass_bytes": traffic // 7 * 8, "fused_launch_only_achieved_bytes_per_s": traffic / (tb_launch * 1e-3),
           "speedup_host_min_over_min": min(ta) / min(tb)}
    if args.graph:
        B, L = (int(x) for x in args.graph.split("x"))
        big = {k: v.to(dev) for k, v in synth.make_pocket_batch(B, L, 16, seed=5).items()}
        m1, m2 = model_on(dev), model_on(dev)
        plain = GraphedTrainStep(m1, big, WEIGHTS)
        whole = GraphedTrainStep(m2, big, WEIGHTS, optimizer=FusedAdam(m2.parameters(), lr=5e-4, max_grad_norm=MAX_NORM))
        tp, tw = [], []
        for _ in range(args.rounds):
            tp.append(host_time(lambda: plain(None, seed=3), 20, 3))
            tw.append(host_time(lambda: whole(None, seed=3), 20, 3))
        out["graphed_step"] = {"B": B, "L": L, "without_optimizer_ms": {"min": min(tp), "max": max(tp)},
                               "with_captured_optimizer_ms": {"min": min(tw), "max": max(tw)}, "calls": 20, "warmup": 3}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
