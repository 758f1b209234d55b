"""numpy float64 oracle of the torsion angles and of the side-chain packing comparison (csrc/torsions.hip lists the conventions):
`torsions` for one structure, `compare` for one pair.  Written from the definitions, vectorised over residues, independent of the
kernels' arithmetic: the angle comes from the projected outer bonds through arctan2, the comparison wraps in float64, the exchange
of equivalent atoms evaluates both full sums.  `torsions` also returns, for every angle, the lengths that the fp32 error bound of the
GPU tests is made of."""
import numpy as np

TWO_PI = 2.0 * np.pi
BACKBONE = (((-1, 1), (-1, 2), (0, 0), (0, 1)),         # omega: CA(n-1), C(n-1), N, CA   as (residue offset, slot)
            ((-1, 2), (0, 0), (0, 1), (0, 2)),          # phi
            ((0, 0), (0, 1), (0, 2), (1, 0)),           # psi
            ((0, 0), (0, 1), (0, 2), (0, 3)))           # psi_o


def dihedral(p0, p1, p2, p3):
    """[...,3] x 4 -> angle in [0, 2 pi), ok, and the bound's ingredients: |b0|, |b1|, |b2|, |v|, |w|, the largest |coordinate|"""
    with np.errstate(all="ignore"):
        b0, b1, b2 = p0 - p1, p2 - p1, p3 - p2
        l1 = np.linalg.norm(b1, axis=-1)
        u = b1 / l1[..., None]
        v = b0 - (b0 * u).sum(-1, keepdims=True) * u
        w = b2 - (b2 * u).sum(-1, keepdims=True) * u
        y = (u * np.cross(v, w)).sum(-1)
        x = (v * w).sum(-1)
        ang = np.mod(np.arctan2(y, x), TWO_PI)
        ang = np.where(ang >= TWO_PI, 0.0, ang)
        lv, lw = np.linalg.norm(v, axis=-1), np.linalg.norm(w, axis=-1)
        ok = (l1 > 0) & (lv > 0) & (lw > 0) & np.isfinite(ang)
        scale = np.max(np.abs(np.stack([p0, p1, p2, p3])), axis=(0, -1))
    return ang, ok, dict(b0=np.linalg.norm(b0, axis=-1), b1=l1, b2=np.linalg.norm(b2, axis=-1), v=lv, w=lw, scale=scale)


def torsions(pos, mask, aa, chi_atoms, residue_index=None):
    """pos [N,A,3], mask [N,A], aa [N], chi_atoms [21,4,4] -> dict(angles [N,8] float64, defined [N,8] bool, geom: dict of [N,8])"""
    pos = np.asarray(pos, np.float64)
    mask = np.asarray(mask) != 0
    aa = np.asarray(aa, np.int64)
    N = len(aa)
    t = np.where((aa < 0) | (aa > 20), 20, aa)
    idx = np.arange(N, dtype=np.int64) if residue_index is None else np.asarray(residue_index, np.int64)
    bonded_prev = np.zeros(N, bool)
    bonded_prev[1:] = idx[1:] - idx[:-1] == 1
    bonded_next = np.zeros(N, bool)
    bonded_next[:-1] = bonded_prev[1:]
    angles, defined = np.zeros((N, 8)), np.zeros((N, 8), bool)
    geom = {k: np.zeros((N, 8)) for k in ("b0", "b1", "b2", "v", "w", "scale")}
    rows = np.arange(N)
    for k in range(8):
        if k < 4:
            need = np.ones(N, bool)
            if k < 2:
                need = bonded_prev
            elif k == 2:
                need = bonded_next
            res = [np.clip(rows + off, 0, N - 1) for off, _ in BACKBONE[k]]
            slot = [np.full(N, s) for _, s in BACKBONE[k]]
        else:
            c = np.asarray(chi_atoms)[t, k - 4]                      # [N,4]
            need = (t < 20) & (c >= 0).all(-1)
            res = [rows] * 4
            slot = [np.clip(c[:, j], 0, 13) for j in range(4)]
        for r, s in zip(res, slot):
            need = need & mask[r, s]
        p = [pos[r, s] for r, s in zip(res, slot)]
        ang, ok, g = dihedral(*p)
        ok = ok & need
        angles[:, k] = np.where(ok, ang, 0.0)
        defined[:, k] = ok
        for name in geom:
            geom[name][:, k] = g[name]
    return dict(angles=angles, defined=defined, geom=geom)


def wrap(d, periodic=False):
    """absolute angle difference -> [0, pi], or [0, pi/2] for a pi-periodic angle"""
    d = np.abs(np.mod(np.asarray(d, np.float64) + np.pi, TWO_PI) - np.pi)
    return np.where(periodic, np.minimum(d, np.pi - d), d)


def frame_local(pos, mask):
    """-> local [N,14,3] coordinates in the backbone frame, ok [N]"""
    with np.errstate(all="ignore"):
        n, ca, c = pos[:, 0], pos[:, 1], pos[:, 2]
        u = c - ca
        lu = np.linalg.norm(u, axis=-1)
        e1 = u / lu[:, None]
        v = n - ca
        v = v - (v * e1).sum(-1, keepdims=True) * e1
        lv = np.linalg.norm(v, axis=-1)
        e2 = v / lv[:, None]
        e3 = np.cross(e1, e2)
        d = pos[:, :14] - ca[:, None]
        local = np.stack([(d * e[:, None]).sum(-1) for e in (e1, e2, e3)], -1)
    return local, mask[:, 0] & mask[:, 1] & mask[:, 2] & (lu > 0) & (lv > 0)


def compare(x, y, periodic, swap, correct_tol):
    """x, y: dicts of one structure each (pos [N,A,3], atom_mask [N,A], aa [N], angles [N,8], defined [N,8]); periodic [21,4] bool,
    swap [21,4] -> the kernel's outputs for the pair in float64 / int, per residue included, plus swap_margin [N]: |plain - exchanged|
    where an exchange was possible (inf elsewhere), to tell a marginal decision from a wrong one"""
    px, py = np.asarray(x["pos"], np.float64), np.asarray(y["pos"], np.float64)
    mx, my = np.asarray(x["atom_mask"]) != 0, np.asarray(y["atom_mask"]) != 0
    ax, ay = np.asarray(x["angles"], np.float64), np.asarray(y["angles"], np.float64)
    dx, dy = np.asarray(x["defined"]) != 0, np.asarray(y["defined"]) != 0
    tx, ty = (np.where((t < 0) | (t > 20), 20, t) for t in (np.asarray(x["aa"], np.int64), np.asarray(y["aa"], np.int64)))
    N = len(tx)
    same = (tx == ty) & (tx < 20)
    cmp = dx & dy
    cmp[:, 3:] &= same[:, None]
    per = np.zeros((N, 8), bool)
    per[:, 4:] = np.asarray(periodic)[tx] != 0
    e = wrap(ax - ay, per)
    err = np.where(cmp, e, np.nan)
    inside = cmp & (e <= correct_tol)
    chi = cmp[:, 4:]
    with_chi = chi.any(1)
    correct = with_chi & (inside[:, 4:] | ~chi).all(1)

    lx, okx = frame_local(px, mx)
    ly, oky = frame_local(py, my)
    sc_sq, sc_n, swapped = np.zeros(N), np.zeros(N, np.int64), np.zeros(N, bool)
    margin = np.full(N, np.inf)
    for n in np.nonzero(same & okx & oky)[0]:
        both = mx[n, :14] & my[n, :14]
        both[:4] = False
        slots = np.nonzero(both)[0]
        plain = float(((lx[n, slots] - ly[n, slots]) ** 2).sum())
        best = plain
        s = [int(v) for v in np.asarray(swap)[tx[n]]]
        listed = [q for q in ((s[0], s[1]), (s[2], s[3])) if q[0] != q[1]]
        if listed and all(both[q[0]] and both[q[1]] for q in listed):
            perm = np.arange(14)
            for u, v in listed:
                perm[u], perm[v] = v, u
            alt = float(((lx[n, perm[slots]] - ly[n, slots]) ** 2).sum())
            margin[n] = abs(alt - plain)
            if alt < plain:
                best, swapped[n] = alt, True
        sc_sq[n], sc_n[n] = best, len(slots)
    atoms = int(sc_n.sum())
    return dict(err=err, err_sum=np.nansum(err, 0), err_count=cmp.sum(0), within=inside.sum(0), res_with_chi=int(with_chi.sum()),
                res_correct=int(correct.sum()), sc_sq=sc_sq, sc_n=sc_n, swapped=swapped, swap_margin=margin, sc_sq_sum=float(sc_sq.sum()),
                sc_atoms=atoms, sc_rmsd=float(np.sqrt(sc_sq.sum() / atoms)) if atoms else float("nan"), compared=cmp)
