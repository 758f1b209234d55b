"""numpy float64 restatement of pf_lddt_fwd, pf_contacts_fwd and geometry.dockq (conventions: csrc/lddt.hip, csrc/contacts.hip): test
infrastructure.  One structure pair at a time, in row blocks of 32 residues, so nothing larger than [448, N * 14] (lddt) or
[480, N * 15] (contacts) is held: a few arrays of 30 MB at 512 residues.

Besides the values, every function returns per row residue the number of decisions that lie within `bound` of their threshold --
those an fp32 evaluation of the same coordinates may take the other way:
  lddt      near_scored: the row's atom pairs with |d_y - cutoff| < bound; near_kept: its scored pairs with
            min_t | |d_y - d_x| - t | < bound over t = 0.5, 1, 2, 4 (the *_cross forms: over partners of another group);
  contacts  near_contact_x / _y, near_interface_x / _y: the row's counted residue pairs with |sqrt(m) - cutoff| < bound."""
import numpy as np

SLOTS = 14
CONTACT_SLOTS = 15
THRESHOLDS = np.array([0.5, 1.0, 2.0, 4.0])
SLOT_MASKS = {"ca": 0x2, "backbone": 0xF, "all": 0x3FFF}
BLOCK = 32
CONTACT_BLOCK = 32


def _bits(slot_mask, n):
    return np.array([(slot_mask >> s) & 1 for s in range(n)], bool)


def compared_atoms(mask_x, aa_x, mask_y, aa_y, slot_mask):
    """[N,14] bool: the atoms that take part"""
    same = (np.asarray(aa_x) == np.asarray(aa_y))[:, None] | (np.arange(SLOTS) < 4)[None, :]
    return np.asarray(mask_x)[:, :SLOTS].astype(bool) & np.asarray(mask_y)[:, :SLOTS].astype(bool) & _bits(slot_mask, SLOTS)[None, :] & same


def lddt(pos_x, mask_x, aa_x, pos_y, mask_y, aa_y, slot_mask=0x3FFF, cutoff=15.0, exclude_same_residue=False, group=None, query=None,
         bound=0.0):
    """one pair: pos_* [N,A,3], mask_* [N,A], aa_* [N]; group / query [N] (of y) -> dict of [N] / [N,14] integer arrays"""
    N = pos_x.shape[0]
    cmp_ = compared_atoms(mask_x, aa_x, mask_y, aa_y, slot_mask)
    X, Y = np.asarray(pos_x, np.float64)[:, :SLOTS].reshape(N * SLOTS, 3), np.asarray(pos_y, np.float64)[:, :SLOTS].reshape(N * SLOTS, 3)
    col = np.flatnonzero(cmp_.reshape(-1))                  # the partners: every compared atom
    rows_on = cmp_ & (np.ones(N, bool) if query is None else np.asarray(query).astype(bool))[:, None]
    grp = None if group is None else np.asarray(group).astype(np.uint8)
    keys = ["scored", "kept", "near_scored", "near_kept"]
    if grp is not None:
        keys += [k + "_cross" for k in keys]
    atom = {k: np.zeros(N * SLOTS, np.int64) for k in keys}
    Yc, Xc, y2 = Y[col], X[col], (Y[col] ** 2).sum(1)
    for r0 in range(0, N, BLOCK):
        row = np.flatnonzero(rows_on[r0:r0 + BLOCK].reshape(-1)) + r0 * SLOTS
        if row.size == 0 or col.size == 0:
            continue
        # a coarse cull through the Gram form (its error is ~1e-11 A^2 against a slack of 0.1 A), the exact expression on what is left
        g = (Y[row] ** 2).sum(1)[:, None] + y2[None, :] - 2.0 * (Y[row] @ Yc.T)
        a, b = np.nonzero(g < (cutoff + bound + 0.1) ** 2)
        ra, cb = row[a], col[b]
        ok = ra != cb
        if exclude_same_residue:
            ok &= ra // SLOTS != cb // SLOTS
        a, b, ra, cb = a[ok], b[ok], ra[ok], cb[ok]
        d_y = np.sqrt(1e-10 + ((Y[ra] - Yc[b]) ** 2).sum(1))
        d_x = np.sqrt(1e-10 + ((X[ra] - Xc[b]) ** 2).sum(1))
        scored = d_y < cutoff
        l1 = np.abs(d_y - d_x)
        kept = (l1[:, None] < THRESHOLDS[None, :]).sum(1)
        near_s = np.abs(d_y - cutoff) < bound
        near_k = scored & (np.abs(l1[:, None] - THRESHOLDS[None, :]).min(1) < bound)
        parts = [("", np.ones(ra.size, bool))]
        if grp is not None:
            parts.append(("_cross", grp[ra // SLOTS] != grp[cb // SLOTS]))
        for tag, m in parts:
            np.add.at(atom["scored" + tag], ra, scored & m)
            np.add.at(atom["kept" + tag], ra, np.where(scored & m, kept, 0))
            np.add.at(atom["near_scored" + tag], ra, near_s & m)
            np.add.at(atom["near_kept" + tag], ra, near_k & m)
    out = {}
    for k, v in atom.items():
        v = v.reshape(N, SLOTS)
        out[k] = v.sum(1)
        if not k.startswith("near"):
            out[k.replace("scored", "scored_atom").replace("kept", "kept_atom")] = v
    return out


def score(kept, scored):
    """kept / (4 scored) from summed counts, NaN where nothing is scored"""
    kept, scored = np.asarray(kept, np.float64), np.asarray(scored, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return kept / (4.0 * scored)


def contacts(pos_x, mask_x, pos_y, mask_y, group, slot_mask=0x3FFF, contact_cutoff=5.0, interface_cutoff=10.0, bound=0.0):
    """one pair: pos_* [N,A,3], mask_* [N,A], group [N] (of y) -> dict of [N] arrays"""
    N = pos_x.shape[0]
    grp = np.asarray(group).astype(np.uint8)
    side = []
    for pos, mask in ((pos_x, mask_x), (pos_y, mask_y)):
        A = min(pos.shape[1], CONTACT_SLOTS)
        m = np.zeros((N, CONTACT_SLOTS), bool)
        m[:, :A] = np.asarray(mask)[:, :A].astype(bool) & _bits(slot_mask, A)[None, :]
        p = np.zeros((N, CONTACT_SLOTS, 3))
        p[:, :A] = np.asarray(pos, np.float64)[:, :A]
        side.append((p, m))
    has = side[0][1].any(1) & side[1][1].any(1)
    out = {k: np.zeros(N, np.int64) for k in ("contacts_x", "contacts_y", "contacts_shared", "near_contact_x", "near_contact_y",
                                              "near_interface_x", "near_interface_y")}
    out.update(interface_x=np.zeros(N, bool), interface_y=np.zeros(N, bool), min_dist_x=np.full(N, np.inf), min_dist_y=np.full(N, np.inf))
    for g in np.unique(grp[has]):                           # rows of one group byte against the residues of every other
        rows_g, cols = np.flatnonzero(has & (grp == g)), np.flatnonzero(has & (grp != g))
        for r0 in range(0, rows_g.size if cols.size else 0, CONTACT_BLOCK):
            rows = rows_g[r0:r0 + CONTACT_BLOCK]
            dist = [np.sqrt(_min_d2(p[rows], m[rows], p[cols], m[cols])) for p, m in side]              # [r, c]
            cx, cy = dist[0] < contact_cutoff, dist[1] < contact_cutoff
            out["contacts_x"][rows], out["contacts_y"][rows], out["contacts_shared"][rows] = cx.sum(1), cy.sum(1), (cx & cy).sum(1)
            for tag, d in (("x", dist[0]), ("y", dist[1])):
                out["interface_" + tag][rows] = (d < interface_cutoff).any(1)
                out["min_dist_" + tag][rows] = d.min(1)
                out["near_contact_" + tag][rows] = (np.abs(d - contact_cutoff) < bound).sum(1)
                out["near_interface_" + tag][rows] = (np.abs(d - interface_cutoff) < bound).sum(1)
    return out


def _min_d2(pa, ma, pb, mb):
    """pa [r,15,3], ma [r,15], pb [c,15,3], mb [c,15] -> [r,c]: the smallest squared distance between existing atoms (every residue
    has one).  Candidates come from the Gram form about a common centre (its error, ~1e-12 A^2, is far below any bound used with
    it); the winning atom pair's distance is then taken from the coordinate differences."""
    r, c = pa.shape[0], pb.shape[0]
    centre = pb[mb].mean(0)
    A, B = (pa - centre).reshape(-1, 3), (pb - centre).reshape(-1, 3)
    g = ((A ** 2).sum(1) + np.where(ma.reshape(-1), 0.0, 1e30))[:, None] + ((B ** 2).sum(1) + np.where(mb.reshape(-1), 0.0, 1e30))[None, :]
    g -= 2.0 * (A @ B.T)
    g = g.reshape(r, CONTACT_SLOTS, c, CONTACT_SLOTS).transpose(0, 2, 1, 3).reshape(r, c, -1)
    k = g.argmin(-1)
    sa, sb = k // CONTACT_SLOTS, k % CONTACT_SLOTS
    d = pa[np.arange(r)[:, None], sa] - pb[np.arange(c)[None, :], sb]
    return (d ** 2).sum(-1)


def kabsch(X, Y):
    """X, Y [n,3] -> (R, t): the proper rotation and translation that minimise |R x + t - y|"""
    cx, cy = X.mean(0), Y.mean(0)
    U, _, Vt = np.linalg.svd((X - cx).T @ (Y - cy))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, cy - R @ cx


def rmsd_after(X, Y, fit, measure):
    """RMSD over `measure` after the superposition of X onto Y fitted over `fit` (NaN when either is empty)"""
    if not fit.any() or not measure.any():
        return np.nan
    R, t = kabsch(X[fit], Y[fit])
    return float(np.sqrt((((X[measure] @ R.T + t) - Y[measure]) ** 2).sum(1).mean()))


def dockq_score(fnat, irmsd, lrmsd):
    return (fnat + 1.0 / (1.0 + (irmsd / 1.5) ** 2) + 1.0 / (1.0 + (lrmsd / 8.5) ** 2)) / 3.0


def dockq(pos_x, mask_x, pos_y, mask_y, group, contact_cutoff=5.0, interface_cutoff=10.0):
    """one pair -> dict of floats: fnat, fnonnat, irmsd, lrmsd, dockq (group != 0: the ligand)"""
    c = contacts(pos_x, mask_x, pos_y, mask_y, group, 0x3FFF, contact_cutoff, interface_cutoff)
    N = pos_x.shape[0]
    lig = np.asarray(group) != 0
    n_y, n_x, n_s = c["contacts_y"][lig].sum(), c["contacts_x"][lig].sum(), c["contacts_shared"][lig].sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        fnat, fnonnat = np.float64(n_s) / n_y, np.float64(n_x - n_s) / n_x
    both = np.asarray(mask_x)[:, :4].astype(bool) & np.asarray(mask_y)[:, :4].astype(bool)
    X, Y = np.asarray(pos_x, np.float64)[:, :4].reshape(4 * N, 3), np.asarray(pos_y, np.float64)[:, :4].reshape(4 * N, 3)
    on = lambda m: (both & m[:, None]).reshape(-1)  # noqa: E731
    face = on(c["interface_y"])
    irmsd = rmsd_after(X, Y, face, face)
    lrmsd = rmsd_after(X, Y, on(~lig), on(lig))
    return dict(fnat=float(fnat), fnonnat=float(fnonnat), irmsd=irmsd, lrmsd=lrmsd, dockq=float(dockq_score(fnat, irmsd, lrmsd)),
                n_native_contacts=int(n_y), n_sample_contacts=int(n_x))
