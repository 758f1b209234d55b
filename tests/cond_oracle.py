"""CPU oracle of the conditioned sampler (FlowModel.sample(t_start= / ts= / start= / aa_allowed= / per-residue switches)).

TEST INFRASTRUCTURE ONLY.  The reference has no such call: its sample() (flow_model.py:229-374) starts from pure noise on
linspace(1e-2, 1, num_steps), applies its three switches to the whole peptide and may draw any of the 20 residue types.  This file
restates that loop from the functions of oracle/pepflow_oracle.py (imported, not edited: encode, ga_encoder, the manifold maps of
corrupt / euler_step, seq_to_simplex, zero_center_part, categorical, torsions_mask) and adds

  * the grid (t_start / ts),
  * the partial start: the interpolants of the training corruption (flow_model.py:125-158, O.corrupt) between the drawn noise and a
    given state at the grid's first time,
  * the three switches per residue: a row's flag stands exactly where the reference tests `sample_*` (252-277, 304-312, 335-341),
  * the allowed classes: the draw is argmax(where(allowed, (p + 1e-8) / E, -1)) with p the softmax over the allowed classes.

With every argument at its default the result is torch.equal to O.sample (tests/test_cond_cpu.py)."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import pepflow_oracle as O  # noqa: E402

DRAW_GAP = 0.05          # as tests/train_oracle.py: a draw whose top-2 gap is below 5 % is "tight"
# The SO(3) geodesic is ill-conditioned where the relative rotation angle nears pi (the log map's axis) -- rotations are compared
# where that angle lies in this band, stated as a condition of the check:
ROT_ANGLE_MIN, ROT_ANGLE_MAX = 0.05, 3.141592653589793 - 0.1


def row_flags(flags, gen):
    """(sample_bb, sample_ang, sample_seq), each a bool or a bool [B, L] tensor -> three bool [B, L] tensors"""
    return tuple(f.bool() if torch.is_tensor(f) else torch.full(gen.shape, bool(f)) for f in flags)


def allowed_rows(aa_allowed, B, L):
    return None if aa_allowed is None else torch.as_tensor(aa_allowed).bool().expand(B, L, O.N_CLASSES)


def scores(logits, expo, allowed):
    """what the draw takes the arg-max of (layers.py:17-22 as O.categorical states it), classes outside the set at -1"""
    if allowed is None:
        return (torch.softmax(logits, -1) + 1e-8) / expo
    p = torch.softmax(logits.masked_fill(~allowed, float("-inf")), -1)
    return torch.where(allowed, (p + 1e-8) / expo, torch.full_like(p, -1.0))


def draw(logits, expo, allowed, rec):
    if rec is not None:
        rec.append(scores(logits, expo, allowed))
    if allowed is None:
        return O.categorical(torch.softmax(logits, -1), expo)
    return torch.argmax(scores(logits, expo, allowed), -1)


def make_grid(num_steps, t_start=None, ts=None):
    if ts is not None:
        return torch.as_tensor(ts, dtype=torch.float32)
    return torch.linspace(1e-2 if t_start is None else t_start, 1.0, num_steps)       # flow_model.py:280, built in fp32


def sample(sd, batch, noise, num_steps, flags=(True, True, True), t_start=None, ts=None, start=None, aa_allowed=None, *,
           encoded=None, preds=None, rec=None, states=None, dtype=torch.float32, init_only=False):
    """The conditioned sample loop.  batch / noise / the returned list of dicts: as O.sample.
    start: None, "native" or a dict with any of rotmats / trans / angles / seqs (missing: the native's).
    encoded: (R1, x1, ang1, seq1, node, edge) to skip encode(); preds: per step (rotmats, trans, RAW angles, logits) to stand in for the
    network (the C-ABI tests); rec: a list that receives every draw's score tensor, in draw order; states: a list that receives the
    state after every Euler step (R, x, angles, seq, simplex, rows whose rotation step had a relative angle in the band below); dtype: float64 runs the same
    arithmetic in double (the yardstick of the fp32 oracle's own error); init_only: return the initial state
    (R_t, x_t, ang_t, seq_t, simplex_t, trans0, simplex0) instead of the trajectory."""
    gen, resm = batch["generate_mask"].bool(), batch["res_mask"].bool()
    B, L = gen.shape
    tmask = O.torsions_mask()
    c = lambda v: v.to(dtype)
    R1, x1, ang1, seq1, node, edge = O.encode(sd, batch) if encoded is None else encoded
    R1, x1, ang1 = c(R1), c(x1), c(ang1)
    fb, fa, fs = row_flags(flags, gen)
    bb, an, sq = gen & fb, gen & fa, gen & fs
    allowed = allowed_rows(aa_allowed, B, L)
    grid = make_grid(num_steps, t_start, ts)
    sx1 = c(O.seq_to_simplex(seq1))
    expo = iter(c(noise["expo"]))
    # ---- initial state, flow_model.py:252-277 with the row's flag for `sample_*` ----
    R0 = torch.where(bb[..., None, None], c(noise["rot0"]), R1)
    x0 = torch.where(bb[..., None], O.zero_center_part(c(noise["trans0"]), gen, resm), x1)
    a0 = torch.where(an[..., None], c(noise["ang0"]), ang1)
    sx0 = torch.where(sq[..., None], O.SIMPLEX_K * c(noise["simplex0"]), sx1)
    R_t, x_t, a_t, sx_t = R0, x0, a0, sx0
    if start is not None:                           # partial start: O.corrupt's interpolants at t0, base = noise, target = start
        st = {} if isinstance(start, str) else start
        assert isinstance(start, dict) or start == "native", start
        sR, sx, sa = c(st.get("rotmats", R1)), c(st.get("trans", x1)), c(st.get("angles", ang1))
        ss = st.get("seqs", seq1)
        t0 = c(grid[0])
        x_t = torch.where(bb[..., None], (1 - t0) * x0 + t0 * sx, x0)
        R_t = torch.where(bb[..., None, None], O.so3_geodesic(t0, sR, R0), R0)
        a_t = torch.where(an[..., None], O.tor_geodesic(t0, sa, a0), a0)
        sx_t = torch.where(sq[..., None], (1 - t0) * sx0 + t0 * c(O.seq_to_simplex(ss)), sx0)
    seq_t = torch.where(sq, draw(sx_t, next(expo), allowed, rec), seq1)
    if init_only:
        return R_t, x_t, a_t, seq_t, sx_t, x0, sx0
    state = (R_t, x_t, a_t, seq_t, sx_t)
    traj = []
    for i in range(num_steps):
        if preds is None:
            t = torch.ones(B, 1) * grid[i]
            R_p, x_p, ang_p, logits = O.ga_encoder(sd, t, state[0], state[1], state[2], state[3], node, edge, resm.long())
        else:
            R_p, x_p, ang_raw, logits = (c(v) for v in preds[i])
            ang_p = ang_raw % O.TWO_PI              # (ga_encoder's last line)
        # ---- post-process, 291-312: the reference draws the sequence and masks the torsions by it whatever sample_seq says ----
        drawn = draw(logits, next(expo), allowed, rec)
        R_c = torch.where(bb[..., None, None], R_p, R1)
        x_c = torch.where(bb[..., None], x_p, x1)
        seq_m = torch.where(gen, drawn, seq1)
        seq_c = torch.where(sq, drawn, seq1)
        a_c = torch.where(gen[..., None], ang_p, ang1)
        a_c = torch.where(tmask[seq_m].bool(), a_c, torch.zeros_like(a_c))
        a_c = torch.where(fa[..., None], a_c, ang1)                     # `if not sample_ang` (308): every row, generated or not
        sx_c = c(O.seq_to_simplex(seq_c))
        traj.append({"rotmats": R_c, "trans": x_c, "angles": a_c, "seqs": seq_c, "seqs_simplex": sx_c,
                     "rotmats_1": R1, "trans_1": x1, "angles_1": ang1, "seqs_1": seq1})
        if i == num_steps - 1:
            break
        # ---- Euler step, 316-341 ----
        dt = c((grid[i + 1] - grid[i]) * torch.ones(B, 1))[..., None]
        R_t, x_t, a_t, seq_t, sx_t = state
        x_n = torch.where(bb[..., None], x_t + (x_c - x0) * dt, x1)
        R_n = torch.where(bb[..., None, None], O.so3_geodesic(dt * 10, R_c, R_t), R1)
        sx_n = sx_t + (sx_c - sx0) * dt
        drawn = draw(sx_n, next(expo), allowed, rec)
        seq_m = torch.where(gen, drawn, seq1)
        seq_n = torch.where(sq, drawn, seq1)
        a_n = torch.where(gen[..., None], O.tor_geodesic(dt, a_c, a_t), ang1)
        a_n = torch.where(tmask[seq_m].bool(), a_n, torch.zeros_like(a_n))
        a_n = torch.where(fa[..., None], a_n, ang1)
        state = (R_n, x_n, a_n, seq_n, sx_n)
        if states is not None:                      # the state after this step + the rows whose rotation step is well conditioned
            th = torch.linalg.norm(O.so3_calc_vf(R_t, R_c), dim=-1)
            states.append(state + (~bb | ((th > ROT_ANGLE_MIN) & (th < ROT_ANGLE_MAX)),))
    return traj


def min_gap(rec, rows):
    """smallest top-2 gap (1 - second / first) over every recorded draw on the rows where a draw is used"""
    worst = 1.0
    for sc in rec:
        top = torch.topk(sc, 2, dim=-1).values[rows]
        if top.numel():
            worst = min(worst, float((1 - top[..., 1] / top[..., 0]).min()))
    return worst


def widen_draws(run, noise, rows, rounds=4):
    """As train_oracle.widen_draws, for a whole free-running loop: run(rec) is the oracle's own run on `noise`; a draw whose top-2 gap is
    below 5 % gets the exponential of its winner halved, in place (the winner stays the winner, so the trajectory does not move).
    -> (number of draws widened, what the last run returned: the oracle's result on the final draws).  Afterwards "zero flipped draws" is a condition the oracle meets by itself."""
    total = 0
    for _ in range(rounds):
        rec = []
        out = run(rec)
        assert len(rec) == noise["expo"].shape[0], (len(rec), noise["expo"].shape)
        changed = 0
        for d, sc in enumerate(rec):
            top = torch.topk(sc, 2, dim=-1)
            tight = ((1 - top.values[..., 1] / top.values[..., 0]) < DRAW_GAP) & rows
            if tight.any():
                e = noise["expo"][d][tight]
                e[torch.arange(e.shape[0]), top.indices[..., 0][tight]] *= 0.5
                noise["expo"][d][tight] = e
                changed += int(tight.sum())
        total += changed
        if not changed:
            return total, out
    raise AssertionError("draws still tight after widening")
