"""CPU oracle of tempered and stochastic sampling (FlowModel.sample(temper=...), pf_sampler_temper).

TEST INFRASTRUCTURE ONLY.  The reference has no such call.  This file restates the loop of cond_oracle.sample on top of its helpers
and of `O` (oracle/pepflow_oracle.py, imported, not edited) with two additions:

  * the PREDICTION draw (draw index 1 + 2 i) takes logits / tau, tau the row's temperature; the initial draw and the state draw from
    the simplex stay as they are;
  * before the Euler step of every step but the last, the rows that move (generated, backbone switch on) are perturbed:
        a = sqrt(dt) * (1 - t)^power for t < t_off, else 0
        x_t += (sigma_trans * a) * z[0:3]          R_t = R_t @ Exp((sigma_rot * a) * z[3:6])
    and the step is taken from the perturbed state ("perturb, then drift").

It also restates, in numpy integer arithmetic, the Philox4x32-10 round function and the counter layout and Box-Muller transform the
kernel draws its six normals per row with, in a float32 variant (the kernel's arithmetic) and a float64 variant (its yardstick).
With temper=None the result is torch.equal to cond_oracle.sample (tests/test_temper_cpu.py)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_oracle as CO  # noqa: E402
from cond_oracle import O  # noqa: E402

DEFAULTS = {"seq_temperature": 1.0, "sigma_trans": 0.0, "sigma_rot": 0.0, "power": 1, "t_off": 1.0}
M32 = np.uint64(0xFFFFFFFF)


# ---- Philox4x32-10, counter layout, Box-Muller -----------------------------------------------------------------------------------------
def philox4x32_10(ctr, k0, k1):
    """ctr: uint32 [..., 4]; k0, k1: the key's words -> uint32 [..., 4].  Ten rounds in uint64 arithmetic (a 32 x 32 product fits)."""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, -1).astype(np.uint32)


def counters(L, step, sample_ids):
    """the two counter blocks of every (sample, residue) at one step: uint32 [B, L, 2, 4] = {l*2 + q, 0x80000000 | s, lo32(gs), hi32(gs)}"""
    gs = np.asarray(sample_ids, dtype=np.int64).astype(np.uint64)
    B = gs.shape[0]
    c = np.zeros((B, L, 2, 4), dtype=np.uint64)
    c[..., 0] = (np.arange(L, dtype=np.uint64)[None, :, None] * np.uint64(2) + np.arange(2, dtype=np.uint64)[None, None, :]) & M32
    c[..., 1] = np.uint64(0x80000000 | int(step))
    c[..., 2] = (gs & M32)[:, None, None]
    c[..., 3] = (gs >> np.uint64(32))[:, None, None]
    return c.astype(np.uint32)


def normals(seed, sample_ids, L, step, dtype=np.float32):
    """six normals per (sample, residue) of one step, [B, L, 6] in `dtype`: u = ((c >> 8) + 0.5) * 2^-24 (exact in both formats);
    Box-Muller on (u0, u1), (u2, u3) of block 0 and (u0, u1) of block 1.  float32: the kernel's operations, 2 pi as float32(2 pi)."""
    seed = int(seed) & (2 ** 64 - 1)
    out = philox4x32_10(counters(L, step, sample_ids), seed & 0xFFFFFFFF, seed >> 32)           # [B, L, 2, 4]
    u = ((out >> np.uint32(8)).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -24)
    two_pi = dtype(np.float32(2 * np.pi)) if dtype is np.float32 else dtype(2 * np.pi)
    z = []
    for q, k in ((0, 0), (0, 2), (1, 0)):
        r = np.sqrt(dtype(-2.0) * np.log(u[:, :, q, k]))
        ang = two_pi * u[:, :, q, k + 1]
        z += [r * np.cos(ang), r * np.sin(ang)]
    z = np.stack(z, -1)
    assert z.dtype == dtype
    return z


def all_normals(seed, sample_ids, L, num_steps, dtype=np.float32):
    """[num_steps - 1, B, L, 6] torch tensor: what the kernel draws over a whole run"""
    B = len(sample_ids)
    if num_steps < 2:
        return torch.zeros(0, B, L, 6, dtype=torch.float32 if dtype is np.float32 else torch.float64)
    return torch.from_numpy(np.stack([normals(seed, sample_ids, L, s, dtype) for s in range(num_steps - 1)]))


# ---- the two additions -----------------------------------------------------------------------------------------------------------------
def params(temper):
    for k in temper:
        assert k in DEFAULTS, k
    return {**DEFAULTS, **temper}


def tau_plane(temper, B, L):
    """None (no tempering: absent or the scalar 1.0) or the float32 [B, L] temperatures"""
    st = params(temper)["seq_temperature"]
    if torch.is_tensor(st):
        return st.to(torch.float32).expand(B, L)
    return None if float(st) == 1.0 else torch.full((B, L), float(st), dtype=torch.float32)


def noise_scale(grid, i, temper, dtype):
    """a = sqrt(dt) * (1 - t)^power, 0 from t_off on: from the float32 grid (dt is the float32 difference, as the kernel and
    cond_oracle form it), carried in `dtype`; t_off is compared as the float32 the device holds"""
    p = params(temper)
    t, dt = grid[i].to(dtype), (grid[i + 1] - grid[i]).to(dtype)
    if float(grid[i]) >= float(np.float32(p["t_off"])):
        return torch.zeros((), dtype=dtype)
    u = 1 - t
    w = {0: torch.ones((), dtype=dtype), 1: u, 2: u * u}[p["power"]]
    return torch.sqrt(dt) * w


def perturb(R_t, x_t, movable, z, grid, i, temper, dtype):
    """the state the Euler step of step i starts from: (R_t, x_t) with the noise of that step on the movable rows"""
    p = params(temper)
    a = noise_scale(grid, i, temper, dtype)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).to(dtype)       # (the device holds the sigmas in float32)  # noqa: E731
    st, sr = f32(p["sigma_trans"]) * a, f32(p["sigma_rot"]) * a
    z = z.to(dtype)
    if float(st) != 0:
        x_t = torch.where(movable[..., None], x_t + st * z[..., 0:3], x_t)
    if float(sr) != 0:
        R_t = torch.where(movable[..., None, None], R_t @ O.so3_exp(sr * z[..., 3:6]), R_t)
    return R_t, x_t


def sample(sd, batch, noise, num_steps, flags=(True, True, True), t_start=None, ts=None, start=None, aa_allowed=None, *, temper=None,
           encoded=None, preds=None, rec=None, states=None, dtype=torch.float32, pre=None):
    """cond_oracle.sample with `temper` (a dict with any of DEFAULTS' entries; None: the same loop without the additions).
    noise["gauss"]: the normals [num_steps - 1, B, L, 6].  pre: a list that receives the perturbed (R_t, x_t) of every step."""
    if temper is None:
        return CO.sample(sd, batch, noise, num_steps, flags, t_start, ts, start, aa_allowed, encoded=encoded, preds=preds, rec=rec,
                         states=states, dtype=dtype)
    gen, resm = batch["generate_mask"].bool(), batch["res_mask"].bool()
    B, L = gen.shape
    tmask = O.torsions_mask()
    c = lambda v: v.to(dtype)  # noqa: E731
    R1, x1, ang1, seq1, node, edge = O.encode(sd, batch) if encoded is None else encoded
    R1, x1, ang1 = c(R1), c(x1), c(ang1)
    fb, fa, fs = CO.row_flags(flags, gen)
    bb, sq = gen & fb, gen & fs
    allowed = CO.allowed_rows(aa_allowed, B, L)
    grid = CO.make_grid(num_steps, t_start, ts)
    tau = tau_plane(temper, B, L)
    p = params(temper)
    noisy = p["sigma_trans"] != 0 or p["sigma_rot"] != 0
    # ---- initial state: cond_oracle's own (it consumes draw 0) ----
    R_t, x_t, a_t, seq_t, sx_t, x0, sx0 = CO.sample(sd, batch, noise, num_steps, flags, t_start, ts, start, aa_allowed,
                                                     encoded=(R1, x1, ang1, seq1, node, edge), rec=rec, dtype=dtype, init_only=True)
    expo = iter(c(noise["expo"])[1:])
    state = (R_t, x_t, a_t, seq_t, sx_t)
    traj = []
    for i in range(num_steps):
        if preds is None:
            t = torch.ones(B, 1) * grid[i]
            R_p, x_p, ang_p, logits = O.ga_encoder(sd, t, state[0], state[1], state[2], state[3], node, edge, resm.long())
        else:
            R_p, x_p, ang_raw, logits = (c(v) for v in preds[i])
            ang_p = ang_raw % O.TWO_PI
        # ---- addition 1: the prediction draw takes logits / tau ----
        if tau is not None:
            logits = logits / c(tau)[..., None]
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
        R_t, x_t, a_t, seq_t, sx_t = state
        # ---- addition 2: perturb, then drift ----
        if noisy:
            R_t, x_t = perturb(R_t, x_t, bb, noise["gauss"][i], grid, i, temper, dtype)
        if pre is not None:
            pre.append((R_t, x_t))
        dt = c((grid[i + 1] - grid[i]) * torch.ones(B, 1))[..., None]
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
        if states is not None:
            th = torch.linalg.norm(O.so3_calc_vf(R_t, R_c), dim=-1)
            states.append(state + (~bb | ((th > CO.ROT_ANGLE_MIN) & (th < CO.ROT_ANGLE_MAX)),))
    return traj
