"""Measuring leg of the restrained relaxation (NOTES.md section 13): times one geometry.relax call (HIP events, after a warm-up
call): 64 complexes, a 12-residue peptide in a 116-residue pocket, 200 iterations; one geometry.relax_energy call; the launch count;
the share of column tiles culled (grad_kernel's criterion restated on the host, at the input structure).  The case is the seeded
complex of the test suite (tests/relax_cases.start_case), so this tool needs the tests/ directory beside it."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import relax_cases as RC  # noqa: E402
from pepflowww_amd import geometry  # noqa: E402

B, N, steps = 64, 128, 200
case = RC.start_case(5001, N, B)
args = [torch.as_tensor(case[k]).cuda() for k in ("pos", "atom_mask", "aa", "residue_index", "movable")]
geometry.relax(*args, steps=steps)
torch.cuda.synchronize()
times = []
for _ in range(5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = geometry.relax(*args, steps=steps)
    e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1))
# energy evaluation alone
ev = []
for _ in range(5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    geometry.relax_energy(args[0], args[0], *args[1:])
    e1.record()
    torch.cuda.synchronize()
    ev.append(e0.elapsed_time(e1))
# culling at the input: grad_kernel's list of column tiles restated (centre: CA, else the first existing atom; extent: distance +
# radius; the row tile's sphere round its movable residues; the kernel's slack), in float32 like the kernel
f = np.float32
rad = geometry.sasa_radius_table().numpy()
aa = case["aa"]
r = rad[np.where((aa < 0) | (aa > 20), 20, aa)]
ex = case["atom_mask"][:, :, :15] & (r > 0)
reach = f(geometry.RELAX_DEFAULTS["clash_margin"]) - f(geometry.RELAX_DEFAULTS["clash_overlap_tolerance"])
n_tiles = (N + 15) // 16
kept = total = 0
for b in range(B):
    x = case["pos"][b][:, :15].astype(f)
    first = np.where(ex[b, :, 1], 1, np.argmax(ex[b], 1))
    c = x[np.arange(N), first]
    ext = np.where(ex[b], np.linalg.norm(x - c[:, None], axis=-1).astype(f) + r[b], f(-1)).max(1)      # -1: no atom
    for rt in range(n_tiles):
        rows = [p for p in range(rt * 16, min(N, rt * 16 + 16)) if case["movable"][b, p] and ext[p] >= 0]
        if not rows:
            continue
        rc = min(rows, key=lambda p: abs(2 * (p - rt * 16) - 15))
        E = max(f(np.linalg.norm(c[p] - c[rc])) + ext[p] for p in rows)
        for ct in range(n_tiles):
            total += 1
            keep = False
            for q in range(ct * 16, min(N, ct * 16 + 16)):
                d = f(np.linalg.norm(c[q] - c[rc]))
                keep = keep or (ext[q] >= 0 and d <= (E + ext[q]) + reach + (f(1e-4) * ((d + E) + ext[q]) + f(1e-3)))
            kept += keep
res = dict(shape=[B, N, 12], steps=steps, relax_ms=sorted(times), relax_energy_ms=sorted(ev), launches=1 + 2 * (steps + 1),
           column_tiles=int(total), column_tiles_kept=int(kept), culled_share=float(1 - kept / total),
           accepted_mean=float(out["accepted"].float().sum(1).mean()), rmsd_mean=float(out["rmsd"].mean()),
           energy_first=float(out["energy_trace"][:, 0].mean()), energy_last=float(out["energy_trace"][:, -1].mean()))
print(json.dumps(res))
