"""numpy restatement of pf_mutation_scan_fwd (csrc/mutscan.hip lists the conventions): test infrastructure.  float64 by default, built
from pack_oracle's pieces -- the frame chain (build_rotamers), the pair function with the bound's ingredients (pair_sums), the
own-residue pair rule (own_pair_table), the rigid-group table (rigid) -- looping over the scanned residues and the candidate types.

What is restated here and not taken from pack_oracle.Structure: every residue but the scanned one is environment exactly as given (no
residue is packed), and the scanned residue's own fixed atoms, radii, type bits, exclusions and own-pair table are the CANDIDATE type's.
It is not FoldX and not Rosetta: the packer's self energy on an unmoved environment."""
import numpy as np

import energy_oracle as EO
import pack_oracle as PO

SLOTS, S0, RA, TYPES = PO.SLOTS, PO.S0, PO.RA, 20


class Scan:
    """One structure: pos [N,A,3], atom_mask [N,A], aa [N], residue_index [N], positions [N]; candidates None or [N,20]; group None
    or [N].  Attributes: scanned [N] bool; res: {(q, t): per-rotamer dict} for every evaluated pair -- pack_oracle's KEYS and
    `pairs`, `table`, E (sets (a) + (b) + the table energy) and Ei (the part of (a) against residues of another group)."""

    def __init__(self, pos, atom_mask, aa, residue_index, positions, candidates=None, group=None, rotamers=None, cutoff=8.0,
                 weights=EO.WEIGHTS, near=0.0, dtype=np.float64):
        self.cutoff, self.w, self.near, self.dtype = float(cutoff), np.asarray(weights, np.float64), float(near), dtype
        chi, count, energy = PO.rotamer_table() if rotamers is None else rotamers
        self.rot_chi, self.rot_count, self.rot_energy = np.asarray(chi), np.asarray(count), np.asarray(energy, np.float64)
        self.rad_tab, self.typ_tab = EO.tables()
        pos, mask, aa = np.asarray(pos), np.asarray(atom_mask) != 0, np.asarray(aa, np.int64)
        N, A = mask.shape
        S = min(A, SLOTS)
        self.N, self.aa, self.idx = N, aa, np.asarray(residue_index, np.int64)
        self.t = np.where((aa < 0) | (aa > 20), 20, aa)
        self.grp = np.zeros(N, np.int64) if group is None else np.asarray(group).astype(np.int64)
        self.scanned = (np.asarray(positions) != 0) & (aa >= 0) & (aa <= 19) & mask[:, 0] & mask[:, 1] & mask[:, 2]
        self.rad, self.typ = self.rad_tab[self.t], self.typ_tab[self.t]
        X, ok = np.zeros((N, SLOTS, 3)), np.zeros((N, SLOTS), bool)
        X[:, :S] = pos[:, :S].astype(np.float64)
        ok[:, :S] = mask[:, :S] & (self.rad[:, :S] > 0)
        self.in_pos, self.in_mask, self.env_X, self.env_ok = pos, mask, X, ok
        self.centre = np.where(ok[:, 1:2], X[:, 1], np.where(ok.any(1)[:, None], X[np.arange(N), ok.argmax(1)], np.inf))
        cand = np.ones((N, TYPES), bool) if candidates is None else np.asarray(candidates) != 0
        self.res = {}
        for q in np.flatnonzero(self.scanned):
            for t in range(TYPES):
                if cand[q, t] or t == aa[q]:
                    self.res[int(q), t] = self._evaluate(int(q), t)

    def _evaluate(self, q, t):
        T, f = PO.rigid(), self.dtype
        R = int(self.rot_count[t])
        atoms, exists, cb = PO.build_rotamers(self.in_pos[q, :3], t, self.rot_chi[t, :R], f)
        atoms = atoms.astype(np.float64)
        rad_t, typ_t = self.rad_tab[t], self.typ_tab[t]
        Xr, okr = atoms.reshape(R * RA, 3), np.tile(exists, R)
        Rr, Tr, slot_r = np.tile(rad_t[S0:14], R), np.tile(typ_t[S0:14], R), np.tile(np.arange(S0, 14), R)
        ca = self.in_pos[q, 1].astype(np.float64)
        ext = float(np.sqrt(((atoms[:, exists] - ca) ** 2).sum(-1)).max()) if exists.any() else 0.0
        # (a): every existing atom of a residue of another residue_index, as given (culled by distance: a superset)
        reach = self.cutoff + self.near + ext + 12.0
        close = np.flatnonzero((np.sqrt(((self.centre - ca) ** 2).sum(-1)) < reach) & (self.idx != self.idx[q]))
        Xc, okc = self.env_X[close].reshape(-1, 3), self.env_ok[close].reshape(-1)
        Rc, Tc = self.rad[close].reshape(-1), self.typ[close].reshape(-1)
        res_c, slot_c = np.repeat(close, SLOTS), np.tile(np.arange(SLOTS), len(close))
        allow = np.ones((len(Xr), len(Xc)), bool)
        cys, pro = PO.res_index()["CYS"], PO.res_index()["PRO"]
        if t == cys:
            allow &= ~((slot_r == S0)[:, None] & ((self.t[res_c] == cys) & (slot_c == S0))[None])
        if t == pro:
            prev = self.idx[res_c] + 1 == self.idx[q]
            allow &= ~((slot_r == 6)[:, None] & (prev & np.isin(slot_c, (1, 2, 3)))[None])
            allow &= ~((slot_r == 5)[:, None] & (prev & (slot_c == 2))[None])
        za = PO.pair_sums(Xr, Rr, Tr, okr, Xc, Rc, Tc, okc, allow, self.cutoff, self.w, self.near)
        across = allow & (self.grp[res_c] != self.grp[q])[None]
        zi = PO.pair_sums(Xr, Rr, Tr, okr, Xc, Rc, Tc, okc, across, self.cutoff, self.w, self.near)
        # (b): the own residue as type t has it: the given N, CA, C, O and slot 14, CB rebuilt, then the rotamer's own atoms
        A = self.in_mask.shape[1]
        X_own, ok_own = np.zeros((SLOTS, 3)), np.zeros(SLOTS, bool)
        for s in (0, 1, 2, 3, 14):
            if s < A:
                X_own[s], ok_own[s] = self.in_pos[q, s], self.in_mask[q, s] and rad_t[s] > 0
        if T["mask"][t, 4] and rad_t[4] > 0:
            X_own[4], ok_own[4] = cb, True
        own = PO.own_pair_table()[t]
        zb = {k: np.zeros(len(Xr), za[k].dtype) for k in PO.KEYS}
        if own[S0:14].any():
            for r in range(R):
                Xo = np.concatenate([X_own[:S0], atoms[r], X_own[14:15]])
                oko = np.concatenate([ok_own[:S0], exists, ok_own[14:15]])
                sl = slice(r * RA, (r + 1) * RA)
                z = PO.pair_sums(Xr[sl], Rr[sl], Tr[sl], okr[sl], Xo, rad_t, typ_t, oko, own[S0:14], self.cutoff, self.w, self.near)
                for k in PO.KEYS:
                    zb[k][sl] = z[k]
        out = PO._fold({k: za[k] + zb[k] for k in PO.KEYS}, R)
        out["E"] = out["E"] + self.rot_energy[t, :R]
        out["table"] = np.abs(self.rot_energy[t, :R])
        out["Ei"] = zi["E"].reshape(R, RA).sum(1)
        out["interface"] = PO._fold(zi, R)                  # the bound's ingredients of Ei
        return out

    def energy(self):
        """-> (energy [N,20] = min_r E (+inf where not evaluated), rotamer [N,20] (-1), n_rotamers [N,20] (0))"""
        e, rot = np.full((self.N, TYPES), np.inf), np.full((self.N, TYPES), -1, np.int64)
        cnt = np.zeros((self.N, TYPES), np.int64)
        for (q, t), z in self.res.items():
            rot[q, t] = int(np.argmin(z["E"]))
            e[q, t], cnt[q, t] = z["E"][rot[q, t]], len(z["E"])
        return e, rot, cnt
