"""Times geometry.cavity_scan (pf_cavity_fwd) on a synthetic receptor of --residues residues (synth.make_pocket, the grid of
geometry.cavity_grid with a margin of --margin A; 6 by default: with 8 the grid of 300 such residues at h = 0.5 passes the 128^3 points
of the kernel) at h = 1.0 and h = 0.5, and the fp32-emulating numpy oracle (tests/cavity_oracle.py) on
the CPU beside it.  Per spacing: the grid, what was found, the time of a call from device events around --reps eager calls (after
warm-up; allocation of the outputs and the status read included), the time of one call replayed from a captured graph (the launches
alone), and the oracle's wall time, after checking that the kernel's labels are the oracle's.  Needs a GPU; prints one JSON line.
Usage: python tools/cavity_bench.py [--residues 300] [--margin 6] [--reps 200]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from pepflowww_amd import _capi, geometry, synth  # noqa: E402
import cavity_oracle  # noqa: E402


def events(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--residues", type=int, default=300)
    ap.add_argument("--margin", type=float, default=6.0)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cavity_bench needs a GPU: a CPU run gives no time")
    dev = torch.device("cuda:0")
    d = synth.make_pocket(np.random.Generator(np.random.PCG64(2024)), args.residues, 1)
    n = args.residues
    pos, mask, aa = (torch.from_numpy(d[k][:n])[None] for k in ("pos_heavyatom", "mask_heavyatom", "aa"))
    radius = geometry.sasa_radius_table()
    dpos, dmask, daa, drad = pos.to(dev), mask.to(dev), aa.to(dev), radius.to(dev)
    out = {"device": torch.cuda.get_device_name(0), "residues": n, "atoms": int(mask.sum()), "margin": args.margin}
    for h in (1.0, 0.5):
        origin, dims = geometry.cavity_grid(pos, mask, h=h, margin=args.margin)
        dorigin = origin.to(dev)
        call = lambda check=True: geometry.cavity_scan(dpos, dmask, daa, dorigin, dims, h=h, radius=drad, check=check)  # noqa: E731
        got = call()
        t0 = time.perf_counter()
        ref = cavity_oracle.scan(pos[0].numpy(), mask[0].numpy(), aa[0].numpy(), radius.numpy(), origin[0].numpy(), dims, h, dtype=np.float32)
        oracle_s = time.perf_counter() - t0
        same = bool(np.array_equal(got["label"][0].cpu().numpy(), ref["label"]) and np.array_equal(got["buried"][0].cpu().numpy(), ref["buried"]))
        case = {"dims": list(dims), "points": int(np.prod(dims)), "n_found": int(got["n_found"][0]), "sizes": got["size"][0].tolist(),
                "equals_fp32_oracle": same, "call_us": round(events(call, args.reps), 1),
                "call_unchecked_us": round(events(lambda: call(False), args.reps), 1), "oracle_cpu_s": round(oracle_s, 2)}
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with _capi.capture_guard(), torch.cuda.graph(g, stream=s):
                call()
        torch.cuda.synchronize()
        case["graph_us"] = round(events(g.replay, args.reps), 1)
        out[f"h{h}"] = case
    print(json.dumps(out))


if __name__ == "__main__":
    main()
