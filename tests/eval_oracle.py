"""numpy float64 restatements of the evaluation metrics (test infrastructure for test_eval_cpu.py / test_gpu_eval.py)."""
import numpy as np


def kabsch(x, y):
    """x, y [n,3] -> dict(r_refl, t_refl: the reference's align rule r = V U^T; r, t: the proper rotation; rmsd_plain, rmsd (proper),
    rmsd_refl).  y ~ r x + t."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = len(x)
    if n == 0:
        nan = float("nan")
        return dict(rmsd_plain=nan, rmsd=nan, rmsd_refl=nan)
    xm, ym = x.mean(0), y.mean(0)
    xc, yc = x - xm, y - ym
    u, s, vt = np.linalg.svd(xc.T @ yc)
    r_refl = vt.T @ u.T
    d = np.sign(np.linalg.det(r_refl)) or 1.0
    r = vt.T @ np.diag([1.0, 1.0, d]) @ u.T
    res = lambda rr: float(np.sqrt(((xc @ rr.T - yc) ** 2).sum() / n))
    return dict(r_refl=r_refl, t_refl=ym - r_refl @ xm, r=r, t=ym - r @ xm, rmsd_plain=float(np.sqrt(((x - y) ** 2).sum() / n)),
                rmsd=res(r), rmsd_refl=res(r_refl))


def batch_align(pos_1, pos_2, mask):
    """[B,L,A,3], [B,L,A,3], [B,L,A] -> pos_1 aligned onto pos_2 by the reference's rule, each sample on its own atoms."""
    pos_1, pos_2, mask = np.asarray(pos_1, np.float64), np.asarray(pos_2, np.float64), np.asarray(mask, bool)
    out = np.empty_like(pos_1)
    for b in range(pos_1.shape[0]):
        k = kabsch(pos_1[b][mask[b]], pos_2[b][mask[b]])
        out[b] = pos_1[b] @ k["r_refl"].T + k["t_refl"]
    return out


def binding_sites(ctx_ca, ca_mask, res_mask, gen_mask, pep, cutoff=10.0):
    """[L,3], [L], [L], [L], [L,3] -> (site [L] bool, margin = min over context-peptide pairs of | |d| - cutoff |)."""
    ctx_ca, pep = np.asarray(ctx_ca, np.float64), np.asarray(pep, np.float64)
    ctx = np.asarray(res_mask, bool) & ~np.asarray(gen_mask, bool) & np.asarray(ca_mask, bool)
    pp = np.asarray(gen_mask, bool) & np.asarray(res_mask, bool)
    d = np.sqrt(((ctx_ca[:, None, :] - pep[None, pp, :]) ** 2).sum(-1))           # [L, n_pep]
    site = ctx & (d <= cutoff).any(1) if d.shape[1] else np.zeros(len(ctx), bool)
    margin = np.abs(d[ctx] - cutoff).min() if d[ctx].size else np.inf
    return site, margin
