"""Time pf_sampler_step_cond (row flags + allowed classes) against pf_sampler_step on fabricated buffers (NOTES.md section 15).

    python tools/cond_step_bench.py [--batch 64] [--length 128] [--gen 16] [--steps 100] [--rounds 3]

Each round initialises the state and times `steps` consecutive launches of one form with device events; the two forms alternate.
The Philox draws are used (expo = NULL), as in a default sample() call."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pepflowww_amd import _capi, sampler  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--length", type=int, default=128)
    ap.add_argument("--gen", type=int, default=16)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    o = ap.parse_args()
    lib, dev = _capi.load(), torch.device("cuda:0")
    B, L, NS = o.batch, o.length, o.steps + 1
    rows = B * L
    g = torch.Generator().manual_seed(0)
    f = lambda *s: torch.randn(*s, generator=g).to(dev)
    eye = torch.eye(3).reshape(9).expand(rows, 9).contiguous().to(dev)
    gen = torch.zeros(B, L)
    gen[:, L - o.gen:] = 1
    t = {"rot1": eye, "trans1": f(rows, 3), "ang1": f(rows, 5).abs(), "seq1": torch.randint(0, 20, (rows,), generator=g).to(dev),
         "gen_mask": gen.reshape(rows).to(dev), "res_mask": torch.ones(rows, device=dev),
         "rot_t": eye.clone(), "trans_t": f(rows, 3), "ang_t": f(rows, 5), "seq_t": torch.zeros(rows, dtype=torch.int64, device=dev),
         "simplex_t": f(rows, 20), "trans0": f(rows, 3), "simplex0": f(rows, 20),
         "pred_rot": eye.clone(), "pred_trans": f(rows, 3), "pred_ang_raw": f(rows, 5), "pred_logits": f(rows, 20),
         "traj_rot": torch.zeros(NS, rows, 9, device=dev), "traj_trans": torch.zeros(NS, rows, 3, device=dev),
         "traj_ang": torch.zeros(NS, rows, 5, device=dev), "traj_seq": torch.zeros(NS, rows, dtype=torch.int64, device=dev),
         "traj_simplex": torch.zeros(NS, rows, 20, device=dev), "ts": torch.linspace(1e-2, 1.0, NS).to(dev),
         "step": torch.zeros(2, dtype=torch.int32, device=dev), "t_out": torch.zeros(B, device=dev)}
    a = _capi.SamplerArgs()
    for k, v in t.items():
        setattr(a, k, v.data_ptr())
    a.num_steps, a.B, a.L, a.seed = NS, B, L, 7
    a.sample_bb = a.sample_ang = a.sample_seq = 1
    noise = [eye, f(rows, 3), f(rows, 5).abs(), f(rows, 20)]
    plane = (torch.rand(rows, generator=g) < 0.6).to(torch.uint8) * 7
    allowed = sampler.pack_aa_allowed(torch.rand(B, L, 20, generator=g) < 0.9, B, L).reshape(rows)
    plane, allowed = plane.to(dev), allowed.to(dev)
    c = _capi.SamplerCondArgs()
    c.res_flags, c.aa_allowed = plane.data_ptr(), allowed.data_ptr()
    st = _capi.stream_ptr()

    def timed(cond):
        _capi.check(lib.pf_sampler_init(C.byref(a), *(n.data_ptr() for n in noise), st), "init")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(o.steps):
            rc = lib.pf_sampler_step_cond(C.byref(a), C.byref(c), st) if cond else lib.pf_sampler_step(C.byref(a), st)
            _capi.check(rc, "step")
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / o.steps * 1e3

    timed(False), timed(True)                       # warm-up: code objects
    res = {"B": B, "L": L, "gen": o.gen, "steps": o.steps, "pf_sampler_step_us": [], "pf_sampler_step_cond_us": []}
    for _ in range(o.rounds):
        res["pf_sampler_step_us"].append(round(timed(False), 3))
        res["pf_sampler_step_cond_us"].append(round(timed(True), 3))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
