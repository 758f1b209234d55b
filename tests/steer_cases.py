"""Cases of the steered sampling tests (tests/test_steer_cpu.py, tests/test_gpu_steer.py), built from seeds on the CPU.

STAND-ALONE cases: one launch holds eight groups of 1, 2, 3, 64, 65, 256, 257 and 1024 members (one wave, one pass of the workgroup,
beyond it, the cap) under interleaved, non-contiguous labels (B = 1672).  Weight kinds: uniform, one dominant, one -inf, all -inf
(code -1), a NaN energy, random.  Uniform kinds: "lo" = 0.5 * 2^-24 and "hi" = 1 - 0.5 * 2^-24 (the ends of what the kernel can draw) and
"mid".  The decision margin min |C_i - p_k S| / S is at most min(u, 1 - u) / n whatever the weights (C_{n-1} = S, p_{n-1} S = S (n - 1 + u)
/ n), so the two ends meet the 1e-9 condition only for n <= 29: groups of 1, 2, 3 take them, the larger groups take 0.25 / 0.75 instead
(margin <= 2.4e-4 / n).  test_steer_cpu asserts the margin of every decision of every case.

CHAIN cases: cond_cases.ABI_SHAPES, 3x16 with the groups {0, 2}, {1} and 2x272 as one group, NS_ABI steps, fabricated predictions.

END TO END: one complex of cond_cases.E2E_SHAPES["L24"] repeated to B = 4, 4 steps.  See e2e_case for the margin the free decisions need."""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_cases as CC  # noqa: E402
import cond_oracle as CO  # noqa: E402
import steer_oracle as SO  # noqa: E402
from cond_oracle import O  # noqa: E402
from pepflowww_amd import synth  # noqa: E402

SIZES = (1, 2, 3, 64, 65, 256, 257, 1024)
KINDS = ("uniform", "dominant", "one_neginf", "all_neginf", "nan_energy", "random")
UKINDS = ("lo", "hi", "mid")
U_LO, U_HI = 0.5 * 2.0 ** -24, 1.0 - 0.5 * 2.0 ** -24
MARGIN = 1e-9
LAM = 0.75


def u_for(n, ukind, g):
    if ukind == "mid":
        return 0.3 + 0.4 * float(torch.rand((), generator=g, dtype=torch.float64))
    if n <= 3:
        return U_LO if ukind == "lo" else U_HI
    return 0.25 if ukind == "lo" else 0.75


@functools.lru_cache(maxsize=None)
def standalone_case(kind, ukind, ess_frac=1.0):
    """-> dict(B, labels int64 [B], groups (member arrays), energy float32 [B, 5], logw float64 [B], u float64 [G], lam, ess_frac)"""
    g = torch.Generator().manual_seed(sum(map(ord, kind + ukind)) + 11)
    B = sum(SIZES)
    lab = torch.cat([torch.full((n,), 7 * j + 3, dtype=torch.int64) for j, n in enumerate(SIZES)])
    lab = lab[torch.randperm(B, generator=g)]                  # interleaved
    groups = SO.groups_of(lab.numpy(), B)
    energy = (2 * torch.rand(B, 5, generator=g)).to(torch.float32)
    logw = torch.zeros(B, dtype=torch.float64) if kind == "uniform" else 1.5 * torch.randn(B, generator=g, dtype=torch.float64)
    if kind == "uniform":
        energy[:] = energy[0]
    for m in groups:
        n = len(m)
        j = int(torch.randint(0, n, (), generator=g))
        if kind == "dominant":
            logw[m[j]] += 60.0
        elif kind == "one_neginf" and n > 1:
            logw[m[max(j, 1)]] = -SO.INF                       # (not the first member: C_0 = 0 would leave a margin of u / n)
        elif kind == "all_neginf":
            logw[m] = -SO.INF
        elif kind == "nan_energy" and n > 1:
            energy[m[max(j, 1)], int(torch.randint(0, 5, (), generator=g))] = float("nan")
    u = np.array([u_for(len(m), ukind, g) for m in groups])
    return {"B": B, "labels": lab, "groups": groups, "energy": energy, "logw": logw, "u": u, "lam": LAM, "ess_frac": ess_frac}


def standalone_ref(case):
    """the oracle's decision of every group of a stand-alone case (always active, always a moment)"""
    logw, eprev = case["logw"].numpy().copy(), np.zeros(case["B"])
    p = {"lam": case["lam"], "every": 1, "ess_frac": case["ess_frac"], "t_on": 0.0, "t_off": 1.0}
    out = SO.step_all(case["energy"].numpy(), logw, eprev, case["groups"], p, 0, 2, 0.5, case["u"])
    out["logw"] = logw
    return out


STANDALONE = [(k, u, 1.0) for k in KINDS for u in UKINDS] + [("random", "mid", 0.4), ("dominant", "mid", 0.4), ("uniform", "mid", 0.4)]


# ---- the kernel chain ------------------------------------------------------------------------------------------------------------------
CHAIN_GROUPS = {"3x16": [0, 1, 0], "2x272": [0, 0]}
CHAIN_GUIDE = {"weights": [1.0, 0.5, 0.25, 0.0], "restraints": [(0, 5, 3.0, 5.0, 1.0), (2, 9, 6.0, 7.0, 0.5)], "scale": 0.15}
CHAIN_TEMPER = {"sigma_trans": 2.0, "sigma_rot": 0.6}
CHAIN_STEER = {"lam": 0.5, "every": 1, "ess_frac": 1.0}


@functools.lru_cache(maxsize=None)
def chain_case(shape):
    case = dict(CC.abi_case(shape))
    B, L = case["B"], case["L"]
    case["flags"] = (torch.ones(B, L, dtype=torch.bool), True, True)
    case["labels"] = torch.tensor(CHAIN_GROUPS[shape], dtype=torch.int64)
    case["gauss"] = torch.randn(case["NS"] - 1, B, L, 6, generator=torch.Generator().manual_seed(6000 + B * L))
    case["u"] = torch.rand(case["NS"], len(set(CHAIN_GROUPS[shape])), generator=torch.Generator().manual_seed(6100 + B * L), dtype=torch.float64)
    return case


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
E2E_B = 4
E2E_LAM = 0.05
E2E_STEER = {"lam": E2E_LAM, "every": 1, "ess_frac": 1.0}
E2E_TEMPER = {"seq_temperature": 0.7, "sigma_trans": 1.0, "sigma_rot": 0.3}


@functools.lru_cache(maxsize=None)
def e2e_batch():
    """one complex of cond_cases.E2E_SHAPES["L24"] repeated to B = 4: the members of the one group are exchangeable"""
    one = CC.e2e_batch("L24")
    return {k: v[:1].repeat((E2E_B,) + (1,) * (v.dim() - 1)).contiguous() for k, v in one.items()}


def e2e_guide():
    batch = e2e_batch()
    gen, resm = batch["generate_mask"].bool(), batch["res_mask"].bool()
    c, p = (resm & ~gen)[0].nonzero().flatten().tolist(), gen[0].nonzero().flatten().tolist()
    hot = torch.zeros(gen.shape[1], dtype=torch.bool)
    hot[c[:3]] = True
    return {"weights": {"receptor_clash": 1.0, "self_clash": 1.0, "ca_bond": 1.0, "hotspot": 0.5}, "r_hotspot": 6.0, "hotspots": hot,
            "restraints": [(p[0], p[-1], 3.5, 6.0, 1.0)], "scale": 0.05, "max_shift": 1.0}


def e2e_noise(seed, equal_expo=False):
    B, L = e2e_batch()["aa"].shape
    noise = synth.make_noise(B, L, CC.NS_E2E, seed=seed)
    noise["gauss"] = torch.randn(CC.NS_E2E - 1, B, L, 6, generator=torch.Generator().manual_seed(7000 + seed))
    noise["resample_u"] = torch.rand(CC.NS_E2E, 1, generator=torch.Generator().manual_seed(7100 + seed), dtype=torch.float64)
    if equal_expo:
        noise["expo"] = noise["expo"][:, :1].repeat(1, B, 1, 1).contiguous()
    return noise


def weight_shift_bound(lam, tol_now, tol_prev):
    """How far the tolerance of the recorded energies can move a decision of a run that resamples at every step (ess_frac = 1, every = 1).

    The device's E_b of a step deviates from the oracle's by at most tol = max_b sum_k tol[s, b, k] (the rule of tests/test_gpu_guide.py,
    per term).  After the reset of the step before, logw_b = -lam * (E_b - eprev_b) with eprev_b a recorded energy of that step (the
    slot's own or its ancestor's), so |d logw_b| <= lam * (tol_now + tol_prev) =: d (step 0: eprev = 0, tol_prev = 0).
    C_i / S = A / (A + R) with A the sum of the weights up to i and R the rest: a logistic function sigma(x) of x = log A - log R.  Every
    weight moves by a factor within exp(+-d), so A and R do, and x by at most 2 d; sigma' <= 1/4, hence |d (C_i / S)| <= d / 2.  The
    decision a_k compares C_i / S with p_k, which does not move: a margin above d / 2 keeps every a_k."""
    return lam * (tol_now + tol_prev) / 2.0


U_GRID = (np.arange(200) + 0.5) / 200


def best_u(logw_rec, move):
    """the uniform of U_GRID with the largest decision margin for one group's log-weights; move: among those that move a particle"""
    n = len(logw_rec)
    best = (-1.0, 0.5)
    for u in U_GRID:
        d = SO.decide(np.zeros((n, 5), np.float32), logw_rec, np.zeros(n), 0.0, 1.0, True, True, u)
        if ((d["anc"] != np.arange(n)).any() or not move) and d["margin_c"] > best[0]:
            best = (d["margin_c"], float(u))
    return best[1]


def e2e_case(sd, seed=61):
    """-> dict(batch, guide, temper, steer, noise, encoded, ref, srec, energy, xs).  The uniforms are CHOSEN, step by step on the oracle's
    own run: of U_GRID the one with the largest margin, at step 0 among those that move a particle (the copies of one particle weigh almost
    the same a step later, so a later move is always one by a hair's breadth; a decision taken by a hair's breadth could not be compared
    with the device's, see weight_shift_bound; test_steer_cpu asserts that the case meets the bound).  Then the draws are widened on the
    oracle's free steered run."""
    batch = e2e_batch()
    guide, temper, steer = e2e_guide(), dict(E2E_TEMPER), dict(E2E_STEER)
    noise = e2e_noise(seed)
    with torch.no_grad():
        enc = O.encode(sd, batch)
        srec, grec = {}, []

        def run(rec):
            grec.clear()
            return SO.sample(sd, batch, noise, CC.NS_E2E, guide=guide, temper=temper, steer=steer, encoded=enc, rec=rec, srec=srec, grec=grec)
        for s in range(CC.NS_E2E - 1):
            run(None)
            noise["resample_u"][s, 0] = best_u(srec["logw"][s], move=s == 0)
        _, ref = CO.widen_draws(run, noise, batch["generate_mask"])
    return {"batch": batch, "guide": guide, "temper": temper, "steer": steer, "noise": noise, "encoded": enc, "ref": ref, "srec": srec,
            "energy": torch.stack([e for e, _, _ in grec]), "xs": [x for _, _, x in grec]}
