"""CPU oracle of guided sampling (FlowModel.sample(guide=...), geometry.ca_potential, pf_guidance_fwd).

TEST INFRASTRUCTURE ONLY.  The reference has no such call; the five C-alpha potentials are stated here in torch from their formulas
(include/pepflow_hip.h), and their gradient comes from AUTOGRAD in float64 -- the kernel's hand-derived gradient is checked against
differentiation, not against a second hand derivation.  Parameters are rounded to fp32 first (they reach the kernel through an fp32
device buffer), so oracle and kernel start from the same numbers.

  energies(x, cls, guide)            the five terms [B, 5] in x's dtype
  potential(x, cls, guide)           float64 energies and gradient on the movable rows
  guided(x_p, x1, cls, guide, t)     one step's guided prediction, its energies and largest shift
  guided_preds(case, guide, ...)     the fabricated per-step predictions of an ABI case, guided: cond_oracle.sample(preds=...) serves
  sample(...)                        cond_oracle.sample's loop restated with the guided prediction in place of x_p (free-running)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_oracle as CO  # noqa: E402
from cond_oracle import O  # noqa: E402

TERMS = ("receptor_clash", "self_clash", "ca_bond", "hotspot", "restraint")
DEFAULTS = {"weights": None, "r_receptor": 4.5, "r_self": 4.5, "min_sep": 3, "bond_tol": 0.1, "r_hotspot": 8.0, "beta": 1.0,
            "hotspots": None, "restraints": None, "scale": 1.0, "t_on": 0.0, "power": 1, "max_shift": 2.0}
CA_CA = 3.8
MAX_PAIRS = 64


def _f32(v):
    return float(np.float32(v))


def params(guide):
    """the guide dict with defaults filled in and every number rounded to fp32 (as a Python float); weights -> a list of four"""
    g = {**DEFAULTS, **(guide or {})}
    w = g["weights"]
    if w is None:
        w = [0.0] * 4
    elif isinstance(w, dict):
        w = [w.get(k, 0.0) for k in TERMS[:4]]
    out = {k: _f32(g[k]) for k in ("r_receptor", "r_self", "bond_tol", "r_hotspot", "beta", "scale", "t_on", "max_shift")}
    out.update(weights=[_f32(v) for v in w], min_sep=int(g["min_sep"]), power=int(g["power"]), hotspots=g["hotspots"], restraints=g["restraints"])
    return out


def restraint_lists(restraints, B):
    if not restraints:
        return [[] for _ in range(B)]
    if all(len(r) == 5 and not isinstance(r[0], (list, tuple)) for r in restraints):
        return [list(restraints)] * B
    assert len(restraints) == B
    return [list(r) for r in restraints]


def row_classes(gen, resm, bb_flag, hotspots=None):
    """-> dict of bool [B, L]: P peptide, M movable, C context, H hot spots"""
    gen, resm = gen.bool(), resm.bool()
    fb = bb_flag.bool() if torch.is_tensor(bb_flag) else torch.full(gen.shape, bool(bb_flag))
    P, C = gen & resm, resm & ~gen
    H = torch.zeros_like(P) if hotspots is None else torch.as_tensor(hotspots).bool().expand(P.shape) & C
    return {"P": P, "M": P & fb, "C": C, "H": H}


def energies(x, cls, guide):
    """[B, 5] in x's dtype; differentiable in x.  A pair at distance 0 gives its energy and no gradient."""
    p = params(guide)
    B, L = cls["P"].shape
    P, C, H = cls["P"], cls["C"], cls["H"]
    dt = x.dtype
    diff = x[:, :, None] - x[:, None]
    d = torch.sqrt((diff * diff).sum(-1).clamp_min(torch.finfo(dt).tiny))                       # [B, i, j]
    relu2 = lambda v: torch.relu(v) ** 2  # noqa: E731
    zero = torch.zeros((), dtype=dt)
    idx = torch.arange(L)
    sep = idx[None, :] - idx[:, None]                                               # j - i
    e0 = torch.where(P[:, :, None] & C[:, None, :], relu2(p["r_receptor"] - d), zero).sum((1, 2))
    e1 = torch.where(P[:, :, None] & P[:, None, :] & (sep >= max(p["min_sep"], 1))[None], relu2(p["r_self"] - d), zero).sum((1, 2))
    db = torch.diagonal(d, offset=1, dim1=1, dim2=2)                                # [B, L - 1]
    e2 = torch.where(P[:, :-1] & P[:, 1:], relu2((db - CA_CA).abs() - p["bond_tol"]), zero).sum(1)
    has_p = P.any(1)
    Ps = torch.where(has_p[:, None], P, torch.ones_like(P))                         # (a sample without peptide rows: masked out below)
    lse = torch.logsumexp((-p["beta"] * d).masked_fill(~Ps[:, :, None], float("-inf")), dim=1)      # over i, per j
    s = -lse / p["beta"]
    e3 = torch.where(H & has_p[:, None], relu2(s - p["r_hotspot"]), zero).sum(1)
    e4 = []
    res = P | C
    for b, rs in enumerate(restraint_lists(p["restraints"], B)):
        tot = torch.zeros((), dtype=dt)
        for (i, j, lo, hi, w) in rs:
            if w > 0 and bool(res[b, i]) and bool(res[b, j]):
                tot = tot + _f32(w) * (relu2(_f32(lo) - d[b, i, j]) + relu2(d[b, i, j] - _f32(hi)))
        e4.append(tot)
    w = p["weights"]
    return torch.stack([w[0] * e0, w[1] * e1, w[2] * e2, w[3] * e3, torch.stack(e4)], -1)


def potential(x, cls, guide):
    """float64: (energies [B, 5], gradient of their sum on the movable rows [B, L, 3], zero elsewhere) -- by autograd"""
    with torch.enable_grad():
        x64 = x.detach().double().requires_grad_(True)
        e = energies(x64, cls, guide)
        (g,) = torch.autograd.grad(e.sum(), x64)
    return e.detach(), torch.where(cls["M"][..., None], g, torch.zeros_like(g))


def schedule(t, p, dtype=torch.float64):
    """lambda(t): 0 below t_on, else scale * u^power with u = (t - t_on) / (1 - t_on)"""
    t = torch.as_tensor(t, dtype=torch.float32).to(dtype)
    u = (t - p["t_on"]) / (1.0 - p["t_on"])
    lam = p["scale"] * (torch.ones_like(u) if p["power"] == 0 else u if p["power"] == 1 else u * u)
    return torch.where(t < p["t_on"], torch.zeros_like(lam), lam)


def guided(x_p, x1, cls, guide, t, dtype=torch.float64):
    """One step: x = x_p on movable rows, x1 elsewhere; -> (guided prediction in `dtype`: x - clipped shift on movable rows, x_p on every
    other row; energies [B, 5] and gradient [B, L, 3] in float64; |shift| per row in `dtype`).  t: a number or [B]."""
    p = params(guide)
    B = x_p.shape[0]
    M = cls["M"][..., None]
    x = torch.where(M, x_p, x1)
    e, g = potential(x, cls, guide)
    lam = schedule(t, p, dtype).reshape(-1, 1, 1).expand(B, 1, 1)
    sh = lam * g.to(dtype)
    n = torch.linalg.norm(sh, dim=-1, keepdim=True)
    sh = sh * torch.clamp(p["max_shift"] / n.clamp_min(1e-12), max=1.0)
    out = torch.where(M, x.to(dtype) - sh, x_p.to(dtype))
    return out, e, g, torch.linalg.norm(sh, dim=-1) * cls["M"]


def guided_preds(case, guide, flags=(True, True, True), grid=None, dtype=torch.float32, rec=None):
    """The fabricated per-step predictions of an ABI case (cond_cases.abi_case's layout) with the translations guided; rec: a list that
    receives (energies, shift_max [B], the positions the energies were taken at) per step."""
    gen, resm = case["batch"]["generate_mask"], case["batch"]["res_mask"]
    cls = row_classes(gen, resm, CO.row_flags(flags, gen)[0], params(guide)["hotspots"])
    grid = CO.make_grid(case["NS"]) if grid is None else grid
    out = []
    for i, (R_p, x_p, a_p, lg) in enumerate(case["preds"]):
        x_g, e, _, n = guided(x_p, case["gt"][1], cls, guide, grid[i], dtype)
        if rec is not None:
            rec.append((e, n.max(1).values, torch.where(cls["M"][..., None], x_p, case["gt"][1])))
        out.append((R_p, x_g.to(dtype), a_p, lg))
    return out


def sample(sd, batch, noise, num_steps, flags=(True, True, True), t_start=None, ts=None, start=None, aa_allowed=None, *, guide=None,
           grec=None, encoded=None, preds=None, rec=None, dtype=torch.float32):
    """cond_oracle.sample's loop with the GUIDED translation prediction in place of x_p (guide = None: x_p itself).  grec: a list that
    receives (energies [B, 5] float64, shift_max [B], the positions the energies were taken at) per step.  The other arguments: as cond_oracle.sample."""
    gen, resm = batch["generate_mask"].bool(), batch["res_mask"].bool()
    B, L = gen.shape
    tmask = O.torsions_mask()
    c = lambda v: v.to(dtype)  # noqa: E731
    R1, x1, ang1, seq1, node, edge = O.encode(sd, batch) if encoded is None else encoded
    R1, x1, ang1 = c(R1), c(x1), c(ang1)
    fb, fa, fs = CO.row_flags(flags, gen)
    bb, an, sq = gen & fb, gen & fa, gen & fs
    allowed = CO.allowed_rows(aa_allowed, B, L)
    grid = CO.make_grid(num_steps, t_start, ts)
    cls = None if guide is None else row_classes(gen, resm, fb, params(guide)["hotspots"])
    expo = iter(c(noise["expo"]))
    R_t, x_t, a_t, seq_t, sx_t, x0, sx0 = CO.sample(sd, batch, {**noise, "expo": noise["expo"][:1]}, num_steps, flags, t_start, ts, start,
                                                    aa_allowed, encoded=(R1, x1, ang1, seq1, node, edge), rec=rec, dtype=dtype, init_only=True)
    next(expo)
    state = (R_t, x_t, a_t, seq_t, sx_t)
    traj = []
    for i in range(num_steps):
        if preds is None:
            t = torch.ones(B, 1) * grid[i]
            R_p, x_p, ang_p, logits = O.ga_encoder(sd, t, state[0], state[1], state[2], state[3], node, edge, resm.long())
        else:
            R_p, x_p, ang_raw, logits = (c(v) for v in preds[i])
            ang_p = ang_raw % O.TWO_PI
        if guide is not None:
            x_u = torch.where(cls["M"][..., None], x_p, x1)
            x_p, e, _, n = guided(x_p, x1, cls, guide, grid[i], dtype)
            if grec is not None:
                grec.append((e, n.max(1).values, x_u))
        drawn = CO.draw(logits, next(expo), allowed, rec)
        R_c = torch.where(bb[..., None, None], R_p, R1)
        x_c = torch.where(bb[..., None], x_p, x1)
        seq_m = torch.where(gen, drawn, seq1)
        seq_c = torch.where(sq, drawn, seq1)
        a_c = torch.where(gen[..., None], ang_p, ang1)
        a_c = torch.where(tmask[seq_m].bool(), a_c, torch.zeros_like(a_c))
        a_c = torch.where(fa[..., None], a_c, ang1)
        sx_c = c(O.seq_to_simplex(seq_c))
        traj.append({"rotmats": R_c, "trans": x_c, "angles": a_c, "seqs": seq_c, "seqs_simplex": sx_c,
                     "rotmats_1": R1, "trans_1": x1, "angles_1": ang1, "seqs_1": seq1})
        if i == num_steps - 1:
            break
        dt = c((grid[i + 1] - grid[i]) * torch.ones(B, 1))[..., None]
        R_t, x_t, a_t, seq_t, sx_t = state
        x_n = torch.where(bb[..., None], x_t + (x_c - x0) * dt, x1)
        R_n = torch.where(bb[..., None, None], O.so3_geodesic(dt * 10, R_c, R_t), R1)
        sx_n = sx_t + (sx_c - sx0) * dt
        drawn = CO.draw(sx_n, next(expo), allowed, rec)
        seq_m = torch.where(gen, drawn, seq1)
        seq_n = torch.where(sq, drawn, seq1)
        a_n = torch.where(gen[..., None], O.tor_geodesic(dt, a_c, a_t), ang1)
        a_n = torch.where(tmask[seq_m].bool(), a_n, torch.zeros_like(a_n))
        a_n = torch.where(fa[..., None], a_n, ang1)
        state = (R_n, x_n, a_n, seq_n, sx_n)
    return traj
