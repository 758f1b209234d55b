"""Cases of the guided-sampling tests (tests/test_guide_cpu.py, tests/test_gpu_guide.py), built from seeds on the CPU.

ABI cases: cond_cases.abi_case's recipe (fabricated context, noise and per-step "network outputs") at cond_cases.ABI_SHAPES plus two
appended samples that can break the kernel's reductions -- 3x16 becomes 5x16, 2x272 becomes 4x272:
  * sample B0     has NO CONTEXT row (every unmasked residue is generated) and an EMPTY restraint list,
  * sample B0 + 1 has NO MOVABLE row (its backbone flag is off on every row: a peptide that is all energy and no shift), and no hot spot;
  * 3x16 keeps cond_cases' sample 1 without any generated residue (no peptide at all);
  * sample 0 carries a FULL restraint list of 64 pairs; the configuration "null_plane" has no hot-spot plane at all.
test_guide_cpu.py checks with the oracle alone that every term is positive somewhere, that the clip is active on one movable row and
inactive on another, and that no pair sits below 1e-3 Angstrom -- so the GPU tests cannot pass hollow."""
import functools
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_cases as CC  # noqa: E402
import cond_oracle as CO  # noqa: E402
import guide_oracle as GO  # noqa: E402
from cond_oracle import O  # noqa: E402
from pepflowww_amd import synth  # noqa: E402

NS = CC.NS_ABI
EXTRA = 2
CONFIGS = ("full", "null_plane", "other")


@functools.lru_cache(maxsize=None)
def abi_case(shape):
    B0, L, empty = CC.ABI_SHAPES[shape]
    B = B0 + EXTRA
    g = torch.Generator().manual_seed(2000 + B * L)
    gen = torch.rand(B, L, generator=g) < 0.4
    gen[:, 0] = True
    resm = torch.ones(B, L, dtype=torch.bool)
    resm[:, -1], gen[:, -1] = False, False
    if empty is not None:
        gen[empty] = False
    gen[B0] = resm[B0]                                   # no context row
    bb = torch.ones(B, L, dtype=torch.bool)
    bb[B0 + 1] = False                                   # no movable row
    seq1 = torch.randint(0, 20, (B, L), generator=g)
    seq1[:, -1] = 21
    gt = (CC._rots(g, B, L), 4 * torch.randn(B, L, 3, generator=g), 2 * math.pi * torch.rand(B, L, 5, generator=g), seq1)
    noise = synth.make_noise(B, L, NS, seed=23)
    preds = [(CC._rots(g, B, L), 4 * torch.randn(B, L, 3, generator=g), (4 * torch.rand(B, L, 5, generator=g) - 1) * 2 * math.pi,
              2 * torch.randn(B, L, 20, generator=g)) for _ in range(NS)]
    case = {"B": B, "L": L, "NS": NS, "B0": B0, "batch": {"generate_mask": gen, "res_mask": resm}, "gt": gt, "noise": noise, "preds": preds,
            "encoded": gt + (None, None), "flags": (bb, True, True)}
    run = lambda rec: CO.sample(None, case["batch"], noise, NS, case["flags"], encoded=case["encoded"], preds=preds, rec=rec)  # noqa: E731
    CO.widen_draws(run, noise, gen)                      # (the draws do not read the translations: widened once, for every guide)
    return case


def _pairs(g, rows, n):
    """n restraints (i, j, lo, hi, weight) between distinct rows of `rows`: bounds that some distances of a 4 A cloud violate on either side"""
    out = []
    for _ in range(n):
        i, j = (rows[k] for k in torch.randperm(len(rows), generator=g)[:2].tolist())
        lo = 2.0 + 6.0 * float(torch.rand((), generator=g))
        out.append((i, j, lo, lo + 2.0 * float(torch.rand((), generator=g)), 0.1 + float(torch.rand((), generator=g))))
    return out


@functools.lru_cache(maxsize=None)
def abi_guide(shape, name):
    """the guide dict of one configuration; hot spots and restraints per sample"""
    case = abi_case(shape)
    B, L, B0 = case["B"], case["L"], case["B0"]
    gen, resm = case["batch"]["generate_mask"], case["batch"]["res_mask"]
    g = torch.Generator().manual_seed(sum(map(ord, name)) + B * L)
    ctx = resm & ~gen
    hot = (torch.rand(B, L, generator=g) < (0.5 if L == 16 else 0.05)) & ctx
    hot[0, int(ctx[0].nonzero()[0])] = True
    hot[B0 + 1] = False
    restraints = []
    for b in range(B):
        rows = resm[b].nonzero().flatten().tolist()
        n = GO.MAX_PAIRS if b == 0 else 0 if b == B0 else 5 + b
        restraints.append(_pairs(g, rows, n))
    # radii for a cloud of 4 A standard deviation: its nearest neighbours sit at 1 - 3 A, so a hot spot is "far" beyond 2 A
    if name == "full":
        return {"weights": {"receptor_clash": 1.0, "self_clash": 0.5, "ca_bond": 0.25, "hotspot": 2.0}, "r_hotspot": 2.0, "hotspots": hot,
                "restraints": restraints, "scale": 0.15, "power": 1, "max_shift": 2.0}
    if name == "null_plane":
        return {"weights": [0.5, 1.0, 1.0, 3.0], "restraints": restraints[1], "scale": 0.02, "power": 2, "t_on": 0.25, "max_shift": 1.0}
    assert name == "other", name
    return {"weights": {"receptor_clash": 0.3, "hotspot": 1.0}, "r_receptor": 5.0, "r_hotspot": 1.5, "beta": 2.0, "hotspots": hot[0],
            "restraints": restraints[1:] + restraints[:1], "scale": 0.1, "power": 0, "max_shift": 0.5}


def abi_x(case, step=0):
    """the positions the potentials see at a step of an ABI case, and the row classes"""
    gen, resm = case["batch"]["generate_mask"], case["batch"]["res_mask"]
    cls = GO.row_classes(gen, resm, case["flags"][0])
    return torch.where(cls["M"][..., None], case["preds"][step][1], case["gt"][1]), cls


# ---- descent: a gentle step must lower the energy ------------------------------------------------------------------------------------
def descent_guide(shape):
    return {**abi_guide(shape, "full"), "scale": 2e-3, "power": 0, "max_shift": 0.05}


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def e2e_guide(shape, which, batch=None):
    """two guides for cond_cases.e2e_batch(shape): 'a' a head-to-tail cycle + hot spots + every weighted term, 'b' other weights, other
    hot spots, per-sample restraints"""
    batch = CC.e2e_batch(shape) if batch is None else batch
    gen, resm = batch["generate_mask"].bool(), batch["res_mask"].bool()
    B, L = gen.shape
    ctx = resm & ~gen
    g = torch.Generator().manual_seed(77 + L + ord(which))
    hot = torch.zeros(B, L, dtype=torch.bool)
    per_sample = []
    for b in range(B):
        c, p = ctx[b].nonzero().flatten().tolist(), gen[b].nonzero().flatten().tolist()
        for k in torch.randperm(len(c), generator=g)[:3].tolist():
            hot[b, c[k]] = True
        per_sample.append([(p[0], p[-1], 3.5, 6.0, 1.0), (p[len(p) // 2], c[b], 4.0, 8.0, 0.5)] + ([(c[0], c[1], 0.0, 1.0, 0.2)] if b else []))
    if which == "a":
        return {"weights": {"receptor_clash": 1.0, "self_clash": 1.0, "ca_bond": 1.0, "hotspot": 0.5}, "r_hotspot": 6.0, "hotspots": hot,
                "restraints": per_sample[0], "scale": 0.05, "max_shift": 1.0}
    return {"weights": [0.2, 0.0, 2.0, 1.5], "r_hotspot": 4.0, "beta": 0.5, "hotspots": hot, "restraints": per_sample, "scale": 0.1,
            "power": 2, "t_on": 0.2, "max_shift": 0.5}


def shard_guide_ref(guide, lo, hi, B):
    """what a shard [lo, hi) of the batch must be guided by (stated here on its own, for the helper tests)"""
    out = dict(guide)
    h = guide.get("hotspots")
    if h is not None and h.dim() == 2:
        out["hotspots"] = h[lo:hi]
    out["restraints"] = GO.restraint_lists(guide.get("restraints"), B)[lo:hi]
    return out
