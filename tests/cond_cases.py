"""Cases of the conditioned-sampler tests (tests/test_cond_cpu.py, tests/test_gpu_cond.py), built from seeds on the CPU.

Two families:
  * ABI cases: fabricated context, noise, start state and per-step "network outputs" for pf_sampler_init_cond / pf_sampler_step_cond
    alone -- no network, milliseconds each;
  * end-to-end cases: a seeded pocket batch + recorded noise for FlowModel.sample against cond_oracle.sample.
Every case carries caller-supplied `expo` draws, widened (cond_oracle.widen_draws) until every draw of the oracle's OWN run has a
top-2 gap of at least 5 %: "zero flipped draws" is then a condition the oracle meets by itself; test_cond_cpu asserts the gap."""
import functools
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import pepflow_oracle as O  # noqa: E402
from pepflowww_amd import synth  # noqa: E402
import cond_oracle as CO  # noqa: E402

CYS = 1                   # constants.py:53-58, 'ACDEFGHIKLMNPQRSTVWY'
NS_ABI = 3                # the record-only last step is hit
# (B, L, sample without a generated residue): 48 rows = one and a half 32-row workgroups of the step kernel; L = 272 = a second trip
# of the init kernel's 256-thread loop
ABI_SHAPES = {"3x16": (3, 16, 1), "2x272": (2, 272, None)}
NONUNIFORM_TS = (0.3, 0.35, 1.0)


def _rots(g, *shape):
    q = torch.randn(*shape, 4, generator=g)
    return O.quat_to_rot(q / q.norm(dim=-1, keepdim=True))


def _allowed(kind, B, L, g):
    if kind is None:
        return None
    if kind == "one":                       # a single class per residue
        return torch.nn.functional.one_hot(torch.randint(0, 20, (B, L), generator=g), 20).bool()
    if kind == "no_cys":                    # 19 classes, one [20] mask for every residue
        m = torch.ones(20, dtype=torch.bool)
        m[CYS] = False
        return m
    assert kind == "random", kind
    m = torch.rand(B, L, 20, generator=g) < 0.5
    m[..., 0] |= ~m.any(-1)
    return m


def _mixed_flags(B, L, g):
    return tuple(torch.rand(B, L, generator=g) < 0.6 for _ in range(3))


@functools.lru_cache(maxsize=None)
def abi_case(shape):
    """Fabricated inputs of the two entry points at one of ABI_SHAPES.  Raw predicted angles lie in [-2 pi, 6 pi): below 0 and above
    2 pi.  The start rotations have a relative angle in [0.05, pi - 0.1] to the noise rotations (the geodesic is ill-conditioned at pi)."""
    B, L, empty = ABI_SHAPES[shape]
    g = torch.Generator().manual_seed(1000 + B * L)
    gen = torch.rand(B, L, generator=g) < 0.4
    gen[:, 0] = True
    resm = torch.ones(B, L, dtype=torch.bool)
    resm[:, -1], gen[:, -1] = False, False          # a padded residue
    if empty is not None:
        gen[empty] = False                          # one sample with no generated residue
    seq1 = torch.randint(0, 20, (B, L), generator=g)
    seq1[:, -1] = 21
    gt = (_rots(g, B, L), 4 * torch.randn(B, L, 3, generator=g), 2 * math.pi * torch.rand(B, L, 5, generator=g), seq1)
    noise = synth.make_noise(B, L, NS_ABI, seed=17)
    preds = [(_rots(g, B, L), 4 * torch.randn(B, L, 3, generator=g), (4 * torch.rand(B, L, 5, generator=g) - 1) * 2 * math.pi,
              2 * torch.randn(B, L, 20, generator=g)) for _ in range(NS_ABI)]
    axis = torch.randn(B, L, 3, generator=g)
    theta = CO.ROT_ANGLE_MIN + torch.rand(B, L, 1, generator=g) * (CO.ROT_ANGLE_MAX - CO.ROT_ANGLE_MIN)
    start = {"rotmats": noise["rot0"] @ O.so3_exp(axis / axis.norm(dim=-1, keepdim=True) * theta),
             "trans": 4 * torch.randn(B, L, 3, generator=g), "angles": 2 * math.pi * torch.rand(B, L, 5, generator=g),
             "seqs": torch.randint(0, 20, (B, L), generator=g)}
    return {"B": B, "L": L, "NS": NS_ABI, "batch": {"generate_mask": gen, "res_mask": resm}, "gt": gt, "noise": noise, "preds": preds,
            "start": start, "encoded": gt + (None, None)}


# name -> (flags kind, allowed kind, partial start, grid): what an ABI run is conditioned on
ABI_CONFIGS = {
    "partial_t001": ("all", None, True, ("t_start", 0.01)),
    "partial_t05": ("all", None, True, ("t_start", 0.5)),
    "partial_t099": ("all", None, True, ("t_start", 0.99)),
    "mixed_one": ("mixed", "one", False, None),
    "mixed_no_cys": ("mixed", "no_cys", False, None),
    "mixed_random": ("mixed", "random", True, ("t_start", 0.5)),
    "nonuniform_ts": ("all", None, False, ("ts", NONUNIFORM_TS)),
}


@functools.lru_cache(maxsize=None)
def abi_config(shape, name):
    """-> dict(case, noise (own widened copy), kw = the conditioning keywords of cond_oracle.sample, ref = the oracle's trajectory)"""
    case = abi_case(shape)
    B, L = case["B"], case["L"]
    fk, ak, partial, grid = ABI_CONFIGS[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)) + B * L)
    kw = {"flags": _mixed_flags(B, L, g) if fk == "mixed" else (True, True, True), "aa_allowed": _allowed(ak, B, L, g),
          "start": case["start"] if partial else None, "t_start": None, "ts": None}
    if grid is not None:
        kw[grid[0]] = grid[1]
    noise = {k: v.clone() for k, v in case["noise"].items()}
    run = lambda rec: CO.sample(None, case["batch"], noise, case["NS"], encoded=case["encoded"], preds=case["preds"], rec=rec, **kw)
    _, ref = CO.widen_draws(run, noise, case["batch"]["generate_mask"])
    return {"case": case, "noise": noise, "kw": kw, "ref": ref}


# ---- end to end: seeded model, NS = 4, B = 2 -----------------------------------------------------------------------------------------
NS_E2E, B_E2E = 4, 2
# L0 = 24 is padded to 32 internally (the one-kernel attention form); L = 64 with 12 generated residues: the fused forms the benchmark runs
E2E_SHAPES = {"L24": (24, 6), "L64": (64, 12)}
E2E_CONFIGS = ("native_t06", "traj_start", "mixed_allowed")


@functools.lru_cache(maxsize=None)
def e2e_batch(shape):
    L, n_gen = E2E_SHAPES[shape]
    return synth.make_pocket_batch(B_E2E, L, n_gen, seed=2718)


def e2e_config(sd, shape, name, start=None):
    """-> dict(batch, noise (widened), kw, encoded, ref = the oracle's trajectory).  traj_start: `start` = the last entry of a first run's trajectory (default: of the oracle's
    own plain run on the same noise)."""
    batch = e2e_batch(shape)
    L = batch["aa"].shape[1]
    noise = synth.make_noise(B_E2E, L, NS_E2E, seed=31 + E2E_CONFIGS.index(name))
    g = torch.Generator().manual_seed(7 + L)
    with torch.no_grad():
        enc = O.encode(sd, batch)
        if name == "native_t06":
            kw = {"t_start": 0.6, "start": "native"}
        elif name == "traj_start":
            if start is None:
                start = O.sample(sd, batch, noise, NS_E2E, encoded=enc)[-1]
            kw = {"t_start": 0.5, "start": {k: start[k].clone() for k in ("rotmats", "trans", "angles", "seqs")}}
        else:
            kw = {"flags": _mixed_flags(B_E2E, L, g), "aa_allowed": _allowed("random", B_E2E, L, g), "t_start": 0.4, "start": "native"}
        run = lambda rec: CO.sample(sd, batch, noise, NS_E2E, encoded=enc, rec=rec, **kw)
        _, ref = CO.widen_draws(run, noise, batch["generate_mask"])
    return {"batch": batch, "noise": noise, "kw": kw, "encoded": enc, "ref": ref}


def sample_kwargs(kw):
    """cond_oracle.sample's conditioning keywords -> FlowModel.sample's"""
    out = {k: v for k, v in kw.items() if k in ("t_start", "ts", "start", "aa_allowed") and v is not None}
    if "flags" in kw:
        out["sample_bb"], out["sample_ang"], out["sample_seq"] = kw["flags"]
    return out
