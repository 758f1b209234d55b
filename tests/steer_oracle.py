"""CPU oracle of steered sampling (FlowModel.sample(steer=...), pf_sampler_steer).

TEST INFRASTRUCTURE ONLY.  The reference has no such call, and the method is written from the publications (Feynman-Kac steering,
Singhal et al. 2025; systematic resampling, Kitagawa 1996, Douc & Cappe 2005), not checked against any other program.  This file restates

  * the DECIDE step of one particle group in numpy float64, every sum sequential in ascending member order (np.cumsum), so that only
    exp() can differ from the kernel in its last bits;
  * the Philox uniform of a (step, group) in integer arithmetic (temper_oracle.philox4x32_10);
  * the loop of guide_oracle.sample / temper_oracle.sample with the resampling added after every Euler step, with a `preds=` path and
    an option to FORCE a given ancestor record.  With steer=None it returns what the existing oracles return (torch.equal).

Every decision reports its MARGINS: min |C_i - p_k S| / S over all (i, k), and |ESS - ess_frac n| / n."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_oracle as CO  # noqa: E402
import guide_oracle as GO  # noqa: E402
import temper_oracle as TO  # noqa: E402
from cond_oracle import O  # noqa: E402

DEFAULTS = {"groups": None, "lam": 1.0, "every": 1, "ess_frac": 0.5, "t_on": 0.0, "t_off": 1.0}
INF = float("inf")


def params(steer):
    for k in steer:
        assert k in DEFAULTS, k
    return {**DEFAULTS, **steer}


def groups_of(labels, B):
    """labels (None: one group) -> list of member arrays, groups in the order of their first member, members ascending"""
    lab = np.zeros(B, dtype=np.int64) if labels is None else np.asarray(labels).reshape(-1)
    order, out = [], {}
    for b in range(B):
        if int(lab[b]) not in out:
            order.append(int(lab[b]))
            out[int(lab[b])] = []
        out[int(lab[b])].append(b)
    return [np.asarray(out[k], dtype=np.int64) for k in order]


def philox_u(seed, step, gs0):
    """the uniform of (step, group): counter {0, 0xC0000000 | s, lo32(gs0), hi32(gs0)}, u = ((c0 >> 8) + 0.5) * 2^-24 (float64, exact)"""
    seed, gs0 = int(seed) & (2 ** 64 - 1), int(gs0) & (2 ** 64 - 1)
    ctr = np.array([0, 0xC0000000 | int(step), gs0 & 0xFFFFFFFF, gs0 >> 32], dtype=np.uint64).astype(np.uint32)
    out = TO.philox4x32_10(ctr, seed & 0xFFFFFFFF, seed >> 32)
    return (float(int(out[0]) >> 8) + 0.5) * 2.0 ** -24


def energy_sum(e5):
    """E_b = (double) e0 + e1 + e2 + e3 + e4 in that order, from float32 terms [n, 5]"""
    e5 = np.asarray(e5, dtype=np.float32)
    E = e5[:, 0].astype(np.float64)
    for j in range(1, 5):
        E = E + e5[:, j].astype(np.float64)
    return E


def decide(e5, logw, eprev, lam, ess_frac, active, moment, u):
    """One group's decision.  e5 float32 [n, 5], logw / eprev float64 [n] (not modified), u a float.
    -> dict: logw_rec (after the update, before a reset), logw, eprev (what the buffers hold afterwards), ess, code, anc (LOCAL ancestor
    of every slot), counts, margin_c, margin_ess."""
    n = len(logw)
    lw, pv = np.array(logw, dtype=np.float64), np.array(eprev, dtype=np.float64)
    with np.errstate(all="ignore"):
        if active:
            E = energy_sum(e5)
            fin = np.isfinite(E)
            lw = np.where(fin, lw + (-np.float64(lam)) * (E - pv), -INF)
            pv = np.where(fin, E, pv)
        lw = np.where(np.isnan(lw), -INF, lw)
        out = {"logw_rec": lw.copy(), "anc": np.arange(n), "counts": np.ones(n, dtype=np.int64), "margin_c": INF, "margin_ess": INF}
        if not active:
            out["logw_rec"] = np.where(np.isnan(np.asarray(logw, dtype=np.float64)), -INF, np.asarray(logw, dtype=np.float64))
        M = lw.max()
        ok = bool(np.isfinite(M))
        ess = 0.0
        if ok:
            w = np.exp(lw - M)
            C = np.cumsum(w)                                   # sequential, ascending
            S, Q = C[-1], np.cumsum(w * w)[-1]
            ess = S * S / Q
    resample = moment and ok and (ess_frac >= 1.0 or ess <= ess_frac * n)
    if moment and ok and 0.0 < ess_frac < 1.0:
        out["margin_ess"] = abs(ess - ess_frac * n) / n
    out.update(ess=float(ess), code=(0 if not moment else -1 if not ok else 2 if resample else 1))
    if resample:
        thr = ((np.float64(u) + np.arange(n, dtype=np.float64)) / np.float64(n)) * S
        a = np.searchsorted(C, thr, side="right")              # the first i with C_i > thr
        a = np.where(a < n, a, np.nonzero(w > 0)[0][-1])
        c = np.bincount(a, minlength=n)
        anc = np.arange(n)
        anc[c == 0] = np.repeat(np.arange(n), np.maximum(c - 1, 0))
        out.update(anc=anc, counts=c, margin_c=float(np.abs(C[:, None] - thr[None, :]).min() / S))
        pv = pv[anc]
        lw = np.zeros(n)
    out.update(logw=lw, eprev=pv)
    return out


def step_all(e5, logw, eprev, groups, p, s, num_steps, t, u_row):
    """the decide step of every group at step s: e5 float32 [B, 5]; logw / eprev float64 [B] are UPDATED in place; u_row[g] the uniforms.
    -> dict: ancestors [B] (sample indices), logw_rec [B], ess [G], code [G], margin_c [G], margin_ess [G]"""
    B = len(logw)
    active = float(np.float64(p["t_on"])) <= float(np.float32(t)) <= float(np.float64(p["t_off"]))
    moment = active and s < num_steps - 1 and (s + 1) % int(p["every"]) == 0
    out = {"ancestors": np.arange(B), "logw_rec": np.zeros(B), "ess": [], "code": [], "margin_c": [], "margin_ess": []}
    for g, m in enumerate(groups):
        d = decide(np.asarray(e5)[m], logw[m], eprev[m], p["lam"], p["ess_frac"], active, moment, u_row[g])
        out["ancestors"][m] = m[d["anc"]]
        out["logw_rec"][m] = d["logw_rec"]
        if active:
            logw[m], eprev[m] = d["logw"], d["eprev"]
        for k in ("ess", "code", "margin_c", "margin_ess"):
            out[k].append(d[k])
    return out


def lineage_brute(ancestors):
    """for every final slot, walk back through the record one particle at a time"""
    a = np.asarray(ancestors)
    N, B = a.shape
    lin = np.zeros((N, B), dtype=np.int64)
    for b in range(B):
        slot = b
        lin[N - 1, b] = slot
        for s in range(N - 2, -1, -1):
            slot = int(a[s, slot])
            lin[s, b] = slot
    return lin


def uniforms(steer, noise, num_steps, B, seed=0, sample_ids=None):
    """[num_steps, G] float64: the supplied noise["resample_u"], else the Philox restatement keyed by the group's first global sample"""
    groups = groups_of(params(steer)["groups"], B)
    if noise is not None and noise.get("resample_u") is not None:
        return np.asarray(noise["resample_u"], dtype=np.float64)
    ids = np.arange(B) if sample_ids is None else np.asarray(sample_ids)
    return np.array([[philox_u(seed, s, ids[m[0]]) for m in groups] for s in range(num_steps)])


def sample(sd, batch, noise, num_steps, flags=(True, True, True), t_start=None, ts=None, start=None, aa_allowed=None, *, guide=None,
           temper=None, steer=None, force=None, energies=None, srec=None, grec=None, encoded=None, preds=None, rec=None,
           dtype=torch.float32, seed=0, pred_rec=None):
    """The loop of guide_oracle.sample and temper_oracle.sample in one, with the resampling after every Euler step.
    steer=None: delegates to the existing oracles whenever one of guide / temper is None (what they return, torch.equal).
    force: an ancestor record [num_steps, B] to apply INSTEAD of the oracle's own decisions (the decisions are still taken and recorded).
    energies: float32 [num_steps, B, 5] to weigh by instead of the oracle's own (the device's record).
    srec: a dict that receives ancestors, logw [N, B], ess, code, margin_c, margin_ess [N, G].  pred_rec: a list that receives every
    step's (R_p, x_p, ang_p, logits) as the network (or preds) gave them."""
    if steer is None and temper is None:
        return GO.sample(sd, batch, noise, num_steps, flags, t_start, ts, start, aa_allowed, guide=guide, grec=grec, encoded=encoded,
                         preds=preds, rec=rec, dtype=dtype)
    if steer is None and guide is None:
        return TO.sample(sd, batch, noise, num_steps, flags, t_start, ts, start, aa_allowed, temper=temper, encoded=encoded, preds=preds,
                         rec=rec, dtype=dtype)
    assert steer is None or guide is not None, "steer needs guide"
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
    cls = None if guide is None else GO.row_classes(gen, resm, fb, GO.params(guide)["hotspots"])
    tau = None if temper is None else TO.tau_plane(temper, B, L)
    tp = None if temper is None else TO.params(temper)
    noisy = tp is not None and (tp["sigma_trans"] != 0 or tp["sigma_rot"] != 0)
    R_t, x_t, a_t, seq_t, sx_t, x0, sx0 = CO.sample(sd, batch, {**noise, "expo": noise["expo"][:1]}, num_steps, flags, t_start, ts, start,
                                                    aa_allowed, encoded=(R1, x1, ang1, seq1, node, edge), rec=rec, dtype=dtype, init_only=True)
    expo = iter(c(noise["expo"])[1:])
    if steer is not None:
        sp = params(steer)
        groups = groups_of(sp["groups"], B)
        U = uniforms(steer, noise, num_steps, B, seed)
        logw, eprev = np.zeros(B), np.zeros(B)
        keep = {k: [] for k in ("ancestors", "logw", "ess", "code", "margin_c", "margin_ess")}
    state = (R_t, x_t, a_t, seq_t, sx_t)
    traj = []
    for i in range(num_steps):
        if preds is None:
            t = torch.ones(B, 1) * grid[i]
            R_p, x_p, ang_p, logits = O.ga_encoder(sd, t, state[0], state[1], state[2], state[3], node, edge, resm.long())
        else:
            R_p, x_p, ang_raw, logits = (c(v) for v in preds[i])
            ang_p = ang_raw % O.TWO_PI
        if pred_rec is not None:
            pred_rec.append((R_p, x_p, ang_p, logits))
        e = None
        if guide is not None:
            x_u = torch.where(cls["M"][..., None], x_p, x1)
            x_p, e, _, n = GO.guided(x_p, x1, cls, guide, grid[i], dtype)
            if grec is not None:
                grec.append((e, n.max(1).values, x_u))
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
        anc = np.arange(B)
        if steer is not None:                          # the decision of step i: taken on this step's energies, also on the last step
            e5 = (e.to(torch.float32) if energies is None else torch.as_tensor(energies)[i]).numpy()
            d = step_all(e5, logw, eprev, groups, sp, i, num_steps, grid[i], U[i])
            anc = d["ancestors"]
            keep["ancestors"].append(anc.copy())
            keep["logw"].append(d["logw_rec"])
            for k in ("ess", "code", "margin_c", "margin_ess"):
                keep[k].append(d[k])
            if force is not None:
                anc = np.asarray(force[i])
        if i == num_steps - 1:
            break
        R_t, x_t, a_t, seq_t, sx_t = state
        if noisy:
            R_t, x_t = TO.perturb(R_t, x_t, bb, noise["gauss"][i], grid, i, temper, dtype)
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
        if steer is not None and (anc != np.arange(B)).any():      # the gather: the seven per-particle tensors
            ix = torch.as_tensor(anc, dtype=torch.int64)
            state = tuple(v[ix] for v in state)
            x0, sx0 = x0[ix], sx0[ix]
    if steer is not None and srec is not None:
        srec.update({k: np.asarray(v) for k, v in keep.items()})
    return traj
