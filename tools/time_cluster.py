"""Times geometry.cluster against the host path it replaces, on the same seeded matrices: copy the [B,B] matrix to the host, then
scipy's linkage + fcluster per group (for gromos, which scipy does not have, and where scipy is absent: the vectorised numpy oracle of
tests/cluster_oracle.py; the output says which).  Device times are medians between device events over `--reps` calls after a warm-up
and include the wrapper's host work (group index, allocations, the launch); host times are medians of a host clock around the copy and
the clustering.  Needs a ROCm device; prints one JSON line per shape and method.

    python tools/time_cluster.py [--reps 20] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cluster_cases as CC  # noqa: E402
import cluster_oracle as CO  # noqa: E402
from pepflowww_amd import geometry  # noqa: E402

try:
    from scipy.cluster import hierarchy
    from scipy.spatial.distance import squareform
except ImportError:
    hierarchy = None

SHAPES = ((1, 1024), (16, 256), (64, 64))       # (groups, samples per group)
CUTOFF = 2.0


def batch(G, n):
    B = G * n
    dist = np.full((B, B), np.nan, dtype=np.float32)
    for g in range(G):
        dist[g * n:(g + 1) * n, g * n:(g + 1) * n] = CC.distance_matrix(CC.seeded_points(n, 500 + g, centres=max(4, n // 40)))
    return dist, np.repeat(np.arange(G), n)


def host_path(dev, G, n, method):
    d = dev.cpu().numpy()
    for g in range(G):
        sub = d[g * n:(g + 1) * n, g * n:(g + 1) * n]
        if method != "gromos" and hierarchy is not None:
            hierarchy.fcluster(hierarchy.linkage(squareform(sub.astype(np.float64), checks=False), method), CUTOFF, "distance")
        else:
            CO.cluster_group(CO.group_matrix(sub, np.arange(n)), CUTOFF, method)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_cluster.py needs a ROCm device: a time taken elsewhere says nothing")
    lines = []
    for G, n in SHAPES:
        dist, groups = batch(G, n)
        dev = torch.as_tensor(dist).cuda()
        for method in geometry.CLUSTER_METHODS:
            for _ in range(5):                                      # warm-up: code objects, allocator, clocks
                out = geometry.cluster(dev, CUTOFF, groups=groups, method=method)
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = geometry.cluster(dev, CUTOFF, groups=groups, method=method)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            host_reps = args.reps if n < 1024 or method != "gromos" else max(5, args.reps // 4)
            hs = []
            for _ in range(host_reps):
                t0 = time.perf_counter()
                host_path(dev, G, n, method)
                hs.append((time.perf_counter() - t0) * 1e3)
            line = {"groups": G, "n": n, "method": method, "device_ms": round(statistics.median(ms), 4),
                    "device_ms_min": round(min(ms), 4), "host_ms": round(statistics.median(hs), 3), "host_reps": host_reps,
                    "host_path": "scipy" if method != "gromos" and hierarchy is not None else "numpy oracle",
                    "clusters": int(out["n_clusters"].sum())}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
