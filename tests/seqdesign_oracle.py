"""numpy restatement of pf_sequence_design_fwd (csrc/seqdesign.hip lists the conventions): test infrastructure.  float64 by default.

It is not ProteinMPNN and not Rosetta fixbb: iterated conditional modes over (type, rotamer) with the packer's energy.  Built from
pack_oracle's pieces (build_rotamers, pair_sums with the bound's ingredients, _fold, rigid) and from scan_oracle.Scan._evaluate for
E_self, which is the scan's E[q,t,r] on an environment from which the designed residues are taken out.  What is restated here: which
residues are designed and their candidate sets, the state (a residue's current atoms follow its current type), the three pair sets P, F
and the total with their exclusions, the start, the search, the profile, brute force and the output structure.  `with_F=False` drops F
from the conditional energy: test_seqdesign_cpu.py shows that the search is then no longer a descent of the total."""
import itertools

import numpy as np

import energy_oracle as EO
import pack_oracle as PO
import scan_oracle as SO

SLOTS, S0, RA, TYPES, MAX_RES = PO.SLOTS, PO.S0, PO.RA, 20, 64
FRAME = np.array([s < S0 or s == 14 for s in range(SLOTS)])
SUMMED = PO.SUMMED
# the fp32 additions of a conditional energy beyond those pack_cases.bound counts for E_self: the nine rows of P and of a partner's
# part of F, the six levels of F's butterfly and the two sums E_self + P + F (csrc/seqdesign.hip: summation order), rounded up
N_EXTRA = 16


class Design:
    """One structure: pos [N,A,3], atom_mask [N,A], aa [N], residue_index [N], designed [N]; candidates None or [N,20]; ref_energy
    None or [20].  Attributes: designed [N] bool (all False and status 1 with more than MAX_RES), dlist (ascending), types[p] (the
    candidate types, ascending), self_[p][t]: per-rotamer dict (pack_oracle's KEYS, pairs, table, E), atoms[p][t] [R,9,3],
    exists[p][t] [9], frame[p][t] = (X [15,3], ok [15]) of the fixed atoms under type t.  A state is a list of (t, r), one per p."""

    def __init__(self, pos, atom_mask, aa, residue_index, designed, candidates=None, ref_energy=None, rotamers=None, cutoff=8.0,
                 weights=EO.WEIGHTS, near=0.0, dtype=np.float64, with_F=True):
        self.cutoff, self.w, self.near, self.dtype, self.with_F = float(cutoff), np.asarray(weights, np.float64), float(near), dtype, with_F
        pos, mask, aa = np.asarray(pos), np.asarray(atom_mask) != 0, np.asarray(aa, np.int64)
        N, A = mask.shape
        self.N, self.aa, self.idx, self.in_pos, self.in_mask = N, aa, np.asarray(residue_index, np.int64), pos, mask
        des = (np.asarray(designed) != 0) & (aa >= 0) & (aa <= 19) & mask[:, 0] & mask[:, 1] & mask[:, 2]
        self.status = int(des.sum() > MAX_RES)
        self.designed = des & (self.status == 0)
        self.dlist = np.flatnonzero(self.designed)
        self.ref = None if ref_energy is None else np.asarray(ref_energy, np.float32).astype(np.float64)
        scan = SO.Scan(pos, mask, aa, residue_index, np.zeros(N, bool), rotamers=rotamers, cutoff=cutoff, weights=weights, near=near,
                       dtype=dtype)
        scan.env_ok[self.designed] = False                  # a designed residue is not environment
        ok = scan.env_ok
        scan.centre = np.where(ok[:, 1:2], scan.env_X[:, 1], np.where(ok.any(1)[:, None], scan.env_X[np.arange(N), ok.argmax(1)], np.inf))
        self.scan, self.rot_chi, self.rot_count = scan, scan.rot_chi, scan.rot_count
        self.rad_tab, self.typ_tab = scan.rad_tab, scan.typ_tab
        cand = np.ones((N, TYPES), bool) if candidates is None else np.asarray(candidates) != 0
        T = PO.rigid()
        self.types, self.self_, self.atoms, self.exists, self.frame = [], [], [], [], []
        for q in self.dlist:
            ts = [int(t) for t in np.flatnonzero(cand[q])] or [int(aa[q])]
            self.types.append(ts)
            se, at, ex, fr = {}, {}, {}, {}
            for t in ts:
                z = scan._evaluate(int(q), t)
                z = {k: v for k, v in z.items() if k not in ("Ei", "interface")}
                if self.ref is not None:
                    z["E"] = z["E"] + self.ref[t]
                    z["table"] = z["table"] + abs(self.ref[t])
                R = int(self.rot_count[t])
                a3, e9, cb = PO.build_rotamers(pos[q, :3], t, self.rot_chi[t, :R], dtype)
                X, okf = np.zeros((SLOTS, 3)), np.zeros(SLOTS, bool)
                for s in (0, 1, 2, 3, 14):
                    if s < A:
                        X[s], okf[s] = pos[q, s], mask[q, s] and self.rad_tab[t, s] > 0
                if T["mask"][t, 4] and self.rad_tab[t, 4] > 0:
                    X[4], okf[4] = cb, True
                se[t], at[t], ex[t], fr[t] = z, a3.astype(np.float64), e9, (X, okf)
            self.self_.append(se)
            self.atoms.append(at)
            self.exists.append(ex)
            self.frame.append(fr)
        self.ca = pos[:, 1].astype(np.float64)

    # ---- the state --------------------------------------------------------------------------------------------------------------------
    def current(self, p, state):
        """the 15 current atoms of designed residue p in `state` = (t, r) -> (X [15,3], ok [15])"""
        t, r = state
        X, ok = self.frame[p][t][0].copy(), self.frame[p][t][1].copy()
        X[S0:14], ok[S0:14] = self.atoms[p][t][r], self.exists[p][t]
        return X, ok

    def partners(self, p):
        """the other designed residues of another residue_index that can be within reach (culled by CA distance: a superset)"""
        q = self.dlist[p]
        d = np.sqrt(((self.ca[self.dlist] - self.ca[q]) ** 2).sum(-1))
        return [int(p2) for p2 in np.flatnonzero((d <= self.cutoff + self.near + 30.0) & (self.idx[self.dlist] != self.idx[q])) if p2 != p]

    def rows_against(self, p, t, p2, state2, cols, row=None):
        """the rotamer atoms of every rotamer of type t on residue p (or of rotamer `row` alone) against the current atoms of p2 in
        state2, of which `cols` [15] bool take part -> per-rotamer dict.  Never evaluated: CYS SG against CYS SG; a PRO row's CD
        against CA, C, O and CG against C of the residue before it."""
        q, q2, (t2, _) = self.dlist[p], self.dlist[p2], state2
        at = self.atoms[p][t] if row is None else self.atoms[p][t][row:row + 1]
        R = len(at)
        X2, ok2 = self.current(p2, state2)
        allow = np.ones((R * RA, SLOTS), bool)
        j = np.tile(np.arange(RA), R)
        cys, pro = PO.res_index()["CYS"], PO.res_index()["PRO"]
        if t == cys and t2 == cys:
            allow[j == 0, S0] = False
        if t == pro and self.idx[q2] + 1 == self.idx[q]:
            allow[np.ix_(j == 1, [1, 2, 3])] = False
            allow[j == 0, 2] = False
        z = PO.pair_sums(at.reshape(R * RA, 3), np.tile(self.rad_tab[t, S0:14], R), np.tile(self.typ_tab[t, S0:14], R),
                         np.tile(self.exists[p][t], R), X2, self.rad_tab[t2], self.typ_tab[t2], ok2 & cols, allow, self.cutoff, self.w,
                         self.near)
        return PO._fold(z, R)

    # ---- the energies -----------------------------------------------------------------------------------------------------------------
    def conditional(self, p, t, state):
        """E_self[p,t,.] + P + F against `state` of the others -> per-rotamer dict"""
        out = {k: np.array(v, copy=True) for k, v in self.self_[p][t].items()}
        everything = np.ones(SLOTS, bool)
        n_f, any_partner = 0, False
        for p2 in self.partners(p):
            any_partner = True
            z = self.rows_against(p, t, p2, state[p2], everything)                              # P
            for k in SUMMED:
                out[k] = out[k] + z[k]
            out["n"] = out["n"] + z["n"]
            if self.with_F:                                                                     # F: the partner's rotamer, p's frame
                t2, r2 = state[p2]
                f = self.rows_against(p2, t2, p, (t, 0), FRAME, row=r2)
                for k in SUMMED:
                    out[k] = out[k] + f[k][0]
                n_f = max(n_f, int(f["n"][0]))
        if any_partner:
            out["n"] = out["n"] + n_f + N_EXTRA
        return out

    def flat(self, p, state):
        """the conditional energies of every candidate (t, r) of p, types ascending, rotamers ascending
        -> (keys: the list of (t, r), dict of arrays over them)"""
        parts = [(t, self.conditional(p, t, state)) for t in self.types[p]]
        keys = [(t, r) for t, z in parts for r in range(len(z["E"]))]
        return keys, {k: np.concatenate([np.broadcast_to(z[k], z["E"].shape) for _, z in parts]) for k in parts[0][1]}

    def flat_self(self, p):
        parts = [(t, self.self_[p][t]) for t in self.types[p]]
        keys = [(t, r) for t, z in parts for r in range(len(z["E"]))]
        return keys, {k: np.concatenate([np.broadcast_to(z[k], z["E"].shape) for _, z in parts]) for k in parts[0][1]}

    def total(self, state):
        """-> dict of scalars: E = sum E_self + sum_p sum_(p2 != p) rot(p) against frame(p2) + sum_(p < p2) rot(p) against rot(p2)"""
        out = {k: 0.0 for k in SUMMED + ("table",)}
        n_max = 0
        everything = np.ones(SLOTS, bool)
        for p in range(len(self.dlist)):
            t, r = state[p]
            s = self.self_[p][t]
            for k in out:
                out[k] += float(s[k][r])
            n_row = int(s["n"][r])
            for p2 in self.partners(p):
                z = self.rows_against(p, t, p2, state[p2], everything if p2 > p else FRAME, row=r)
                for k in SUMMED:
                    out[k] += float(z[k][0])
                n_row += int(z["n"][0])
            n_max = max(n_max, n_row)
        out["n"] = n_max
        return out

    # ---- the search -------------------------------------------------------------------------------------------------------------------
    def start(self):
        out = []
        for p in range(len(self.dlist)):
            keys, z = self.flat_self(p)
            out.append(keys[int(np.argmin(z["E"]))])
        return out

    def icm(self, sweeps=8, audit=False, start=None):
        """start: the state to begin from (None: `start()`) -> dict(start, state, choices [sweeps_run][P] of (t, r), changed, changed_types, energy_trace, sweeps_run, margins: at every
        decision the runner-up's energy minus the minimum; with audit, moves: for every accepted move (the conditional energy it
        saves, the total it saves))"""
        cur = self.start() if start is None else list(start)
        out = dict(start=list(cur), choices=[], changed=[], changed_types=[], energy_trace=[self.total(cur)["E"]], margins=[],
                   sweeps_run=0, moves=[])
        for p in range(len(self.dlist)):
            e = np.sort(self.flat_self(p)[1]["E"])
            out["margins"].append(float(e[1] - e[0]) if len(e) > 1 else np.inf)
        for _ in range(sweeps):
            changed, changed_t, row = 0, 0, []
            for p in range(len(self.dlist)):
                keys, z = self.flat(p, cur)
                best = keys[int(np.argmin(z["E"]))]
                srt = np.sort(z["E"])
                out["margins"].append(float(srt[1] - srt[0]) if len(srt) > 1 else np.inf)
                if best != cur[p]:
                    if audit:
                        before = self.total(cur)["E"]
                        saved = float(z["E"][keys.index(cur[p])] - z["E"].min())
                    changed += 1
                    changed_t += best[0] != cur[p][0]
                    cur[p] = best
                    if audit:
                        out["moves"].append((saved, before - self.total(cur)["E"]))
                row.append(best)
            out["choices"].append(row)
            out["changed"].append(changed)
            out["changed_types"].append(changed_t)
            out["energy_trace"].append(self.total(cur)["E"])
            out["sweeps_run"] += 1
            if changed == 0:
                break
        out["state"] = cur
        return out

    def profile(self, state):
        """-> (profile [N,20] = min_r conditional (+inf), profile_rotamer [N,20] (-1))"""
        e, rot = np.full((self.N, TYPES), np.inf), np.full((self.N, TYPES), -1, np.int64)
        for p, q in enumerate(self.dlist):
            for t in self.types[p]:
                z = self.conditional(p, t, state)["E"]
                rot[q, t] = int(np.argmin(z))
                e[q, t] = z[rot[q, t]]
        return e, rot

    def brute_force(self):
        """-> (the smallest total over every combination of candidate (t, r), its state): only for a handful of residues and states"""
        P = len(self.dlist)
        keys = [self.flat_self(p)[0] for p in range(P)]
        size = [len(k) for k in keys]
        shape = lambda *ps: [size[p] if p in ps else 1 for p in range(P)]  # noqa: E731
        total = np.zeros(size)
        everything = np.ones(SLOTS, bool)
        for p in range(P):
            total = total + self.flat_self(p)[1]["E"].reshape(shape(p))
            for p2 in self.partners(p):
                m = np.zeros((size[p], size[p2]))
                for k2, st2 in enumerate(keys[p2]):
                    col = [self.rows_against(p, t, p2, st2, everything if p2 > p else FRAME)["E"] for t in self.types[p]]
                    m[:, k2] = np.concatenate(col)
                total = total + (m if p < p2 else m.T).reshape(shape(p, p2))
        arg = np.unravel_index(int(np.argmin(total)), total.shape)
        return float(total[arg]), [keys[p][int(k)] for p, k in enumerate(arg)]

    def output(self, state):
        """-> (aa [N], pos [N,15,3], mask [N,15] bool, chi [N,4], rotamer [N]) of the designed structure, float64"""
        T = PO.rigid()
        A = self.in_mask.shape[1]
        S = min(A, SLOTS)
        pos, mask, chi = np.zeros((self.N, SLOTS, 3)), np.zeros((self.N, SLOTS), bool), np.zeros((self.N, 4))
        pos[:, :S], mask[:, :S] = self.in_pos[:, :S], self.in_mask[:, :S]
        aa, rot = self.aa.copy(), np.full(self.N, -1, np.int64)
        for p, q in enumerate(self.dlist):
            t, r = state[p]
            aa[q], rot[q] = t, r
            mask[q, 4:14] = T["mask"][t, 4:14]
            pos[q, 4:14] = 0.0
            if mask[q, 4]:
                pos[q, 4] = self.frame[p][t][0][4]
            pos[q, S0:14][self.exists[p][t]] = self.atoms[p][t][r][self.exists[p][t]]
            chi[q] = self.rot_chi[t, r]
        return aa, pos, mask, chi, rot


def state_product(o):
    """every state of a small Design, for tests"""
    return itertools.product(*[o.flat_self(p)[0] for p in range(len(o.dlist))])
