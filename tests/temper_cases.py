"""Cases of the tempered / stochastic sampling tests (tests/test_temper_cpu.py, tests/test_gpu_temper.py), built from seeds on the CPU.

ABI cases: guide_cases.abi_case's fabricated inputs (cond_cases.ABI_SHAPES extended: 3x16 becomes 5x16 and 2x272 becomes 4x272; one
appended sample has no context row, one has its backbone switch off on every row; 3x16 keeps its sample without any generated residue)
plus pre-drawn normals `gauss` [NS - 1, B, L, 6].  Configurations:
  * full           per-row temperatures mixed over [0.3, 3], both sigmas, power 1;
  * null_plane     no temperature plane, sigmas only, power 0, t_off = 0.6 on the grid linspace(0.3, 1, 3) = (0.3, 0.65, 1): step 0 is
                   noisy, step 1 lies beyond t_off and gets none;
  * tau_only       one temperature (0.1, the reference's evaluation setting of its inverse-folding baseline) for every row, sigmas 0;
  * nonuniform_ts  `full` on cond_cases.NONUNIFORM_TS.
Every configuration carries its own copy of the `expo` draws, widened (cond_oracle.widen_draws) on the TEMPER oracle's own run, so
"zero flipped draws" is a condition the oracle meets by itself; test_temper_cpu asserts the gap and that no check can pass hollow."""
import functools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_cases as CC  # noqa: E402
import cond_oracle as CO  # noqa: E402
import guide_cases as GC  # noqa: E402
import temper_oracle as TO  # noqa: E402
from cond_oracle import O  # noqa: E402
from pepflowww_amd import synth  # noqa: E402

NS = CC.NS_ABI
CONFIGS = ("full", "null_plane", "tau_only")
ALL_CONFIGS = CONFIGS + ("nonuniform_ts",)
SIGMA_TRANS, SIGMA_ROT = 2.0, 0.6          # Angstrom / radian per sqrt of flow time: a step of dt = 0.5 moves a row by ~1.4 A, ~0.4 rad


def mixed_tau(B, L, g):
    """per-row temperatures, log-uniform over [0.3, 3]"""
    return (0.3 * 10.0 ** torch.rand(B, L, generator=g)).to(torch.float32)


def abi_case(shape):
    """guide_cases.abi_case: the 5x16 / 4x272 inputs with the degenerate samples and the per-row backbone switch case["flags"]"""
    return GC.abi_case(shape)


def abi_temper(shape, name):
    """-> (temper dict, grid keywords of cond_oracle.sample)"""
    case = abi_case(shape)
    B, L = case["B"], case["L"]
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 3 * B * L)
    if name == "full":
        return {"seq_temperature": mixed_tau(B, L, g), "sigma_trans": SIGMA_TRANS, "sigma_rot": SIGMA_ROT, "power": 1}, {}
    if name == "null_plane":
        return {"sigma_trans": SIGMA_TRANS, "sigma_rot": SIGMA_ROT, "power": 0, "t_off": 0.6}, {"t_start": 0.3}
    if name == "tau_only":
        return {"seq_temperature": 0.1}, {}
    assert name == "nonuniform_ts", name
    return {"seq_temperature": mixed_tau(B, L, g), "sigma_trans": SIGMA_TRANS, "sigma_rot": SIGMA_ROT, "power": 1}, {"ts": CC.NONUNIFORM_TS}


def gauss_of(B, L, num_steps, seed):
    return torch.randn(num_steps - 1, B, L, 6, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def abi_config(shape, name):
    """-> dict(case, noise (own copy: gauss added, expo widened on the temper oracle's run), temper, kw = flags + grid keywords,
    ref = the oracle's trajectory, widened = how many draws the widening touched)"""
    case = abi_case(shape)
    temper, grid_kw = abi_temper(shape, name)
    kw = {"flags": case["flags"], **grid_kw}
    noise = {k: v.clone() for k, v in case["noise"].items()}
    noise["gauss"] = gauss_of(case["B"], case["L"], NS, 4000 + case["B"] * case["L"])
    run = lambda rec: TO.sample(None, case["batch"], noise, NS, temper=temper, encoded=case["encoded"], preds=case["preds"], rec=rec, **kw)  # noqa: E731
    n, ref = CO.widen_draws(run, noise, case["batch"]["generate_mask"])
    return {"case": case, "noise": noise, "temper": temper, "kw": kw, "ref": ref, "widened": n}


def movable(case):
    return case["batch"]["generate_mask"] & CO.row_flags(case["flags"], case["batch"]["generate_mask"])[0]


# ---- end to end: cond_cases.E2E_SHAPES, NS_E2E = 4 on linspace(0.01, 1, 4) = (0.01, 0.34, 0.67, 1) ------------------------------------
def e2e_temper(shape, which):
    """two parameter sets: 'a' one temperature plane per sample + both sigmas; 'b' a scalar temperature, other sigmas, power 0 and
    t_off = 0.6 (the step at t = 0.67 gets no noise)"""
    batch = CC.e2e_batch(shape)
    B, L = batch["aa"].shape
    g = torch.Generator().manual_seed(91 + L + ord(which))
    if which == "a":
        return {"seq_temperature": mixed_tau(B, L, g), "sigma_trans": 1.0, "sigma_rot": 0.3, "power": 1}
    assert which == "b", which
    return {"seq_temperature": 0.5, "sigma_trans": 0.5, "sigma_rot": 0.5, "power": 0, "t_off": 0.6}


def e2e_config(sd, shape, which, seed):
    """-> dict(batch, noise (gauss added, expo widened on the temper oracle's free run), temper, encoded, ref)"""
    batch = CC.e2e_batch(shape)
    B, L = batch["aa"].shape
    temper = e2e_temper(shape, which)
    noise = synth.make_noise(B, L, CC.NS_E2E, seed=seed)
    noise["gauss"] = gauss_of(B, L, CC.NS_E2E, 5000 + seed)
    with torch.no_grad():
        enc = O.encode(sd, batch)
        run = lambda rec: TO.sample(sd, batch, noise, CC.NS_E2E, temper=temper, encoded=enc, rec=rec)  # noqa: E731
        _, ref = CO.widen_draws(run, noise, batch["generate_mask"])
    return {"batch": batch, "noise": noise, "temper": temper, "encoded": enc, "ref": ref}


def shard_temper_ref(temper, lo, hi, B):
    """what a shard [lo, hi) of the batch must be tempered by (stated here on its own, for the helper tests)"""
    out = dict(temper)
    st = temper.get("seq_temperature")
    if torch.is_tensor(st) and st.dim() == 2:
        out["seq_temperature"] = st[lo:hi]
    return out
