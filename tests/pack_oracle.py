"""numpy restatement of pf_pack_sidechains_fwd (csrc/packing.hip lists the conventions): test infrastructure.  float64 by default; every
function that builds or scores takes `dtype`, so that the same statements run in float32 measure what fp32 costs (pack_cases.py).

It is not SCWRL4 and not Rosetta's packer: a staggered rotamer grid, the package's own Vina-form pair energy (energy_oracle.pair_terms),
iterated conditional modes.  What is restated here independently of pepflowww_amd.geometry: the rotamer grid, the own-residue pair rule
(a breadth-first search over geometry.bond_table), the frame chain (in a loop form and in a vectorised form), the three pair sets and
their exclusions, the search."""
import itertools
import os

import numpy as np

import energy_oracle as EO
from pepflowww_amd import geometry
from pepflowww_amd.preprocess import _HERE, _tables

SLOTS, S0, RA = 15, 5, 9            # slots per residue, the first rotamer slot, rotamer atoms per residue
FIXED_SLOTS = (0, 1, 2, 3, 4, 14)
STAGGERED = (60.0, 180.0, 300.0)
PLANAR = {"ASN": 2, "ASP": 2, "GLN": 3, "GLU": 3, "HIS": 2, "PHE": 2, "TYR": 2, "TRP": 2}
PI_PERIODIC = {"ASP": 2, "GLU": 3, "PHE": 2, "TYR": 2}
PRO_ROWS = ((30.0, -35.0), (-30.0, 35.0))
N_CHI = {"ALA": 0, "GLY": 0, "CYS": 1, "SER": 1, "THR": 1, "VAL": 1, "ASP": 2, "ASN": 2, "HIS": 2, "ILE": 2, "LEU": 2, "PHE": 2, "PRO": 2,
         "TRP": 2, "TYR": 2, "GLN": 3, "GLU": 3, "MET": 3, "ARG": 4, "LYS": 4}
COUNTS_30 = {"ARG": 81, "LYS": 81, "GLN": 108, "GLU": 54, "MET": 27, "ASN": 36, "HIS": 36, "TRP": 36, "ASP": 18, "PHE": 18, "TYR": 18,
             "ILE": 9, "LEU": 9, "CYS": 3, "SER": 3, "THR": 3, "VAL": 3, "PRO": 2, "ALA": 1, "GLY": 1}
_CACHE = {}


def res_index():
    return _tables()["res_index"]


def rotamer_rows(step_deg=30.0):
    """-> [21] lists of chi rows in degrees"""
    rows = [[()] for _ in range(21)]
    for name, t in res_index().items():
        if t >= 20 or N_CHI[name] == 0:
            continue
        if name == "PRO":
            rows[t] = list(PRO_ROWS)
            continue
        axes = []
        for k in range(1, N_CHI[name] + 1):
            if PLANAR.get(name) == k:
                period = 180.0 if PI_PERIODIC.get(name) == k else 360.0
                axes.append(tuple(np.arange(0.0, period - 1e-9, step_deg)))
            else:
                axes.append(STAGGERED)
        rows[t] = list(itertools.product(*axes))
    return rows


def rotamer_table(step_deg=30.0):
    """-> chi [21,R,4] float32 radians (the values the device reads), count [21], energy [21,R]"""
    rows = rotamer_rows(step_deg)
    count = np.array([len(r) for r in rows], np.int32)
    chi = np.zeros((21, int(count.max()), 4))
    for t, rs in enumerate(rows):
        for r, row in enumerate(rs):
            chi[t, r, :len(row)] = np.radians(row)
    return chi.astype(np.float32), count, np.zeros(chi.shape[:2], np.float32)


def rigid():
    if "rigid" not in _CACHE:
        d = np.load(os.path.join(_HERE, "data", "rigid_groups.npz"))
        _CACHE["rigid"] = dict(rot=d["rotation"][:21].astype(np.float64), trans=d["translation"][:21].astype(np.float64),
                               group=d["atom14_group"][:21].astype(np.int64), pos=d["atom14_position"][:21].astype(np.float64),
                               mask=d["heavyatom_mask"].astype(bool))
    return _CACHE["rigid"]


def own_pair_table():
    """-> [21,15,15] bool: (t, a, b): a a rotamer atom, b more than three bonds away (breadth-first search over bond_table), b fixed
    (N, CA, C, O, CB, OXT) or a rotamer atom of a smaller slot"""
    if "own" not in _CACHE:
        bonds = geometry.bond_table().numpy()
        g, has = rigid()["group"], EO.tables()[0] > 0            # (the slots a type has, OXT among them)
        tab = np.zeros((21, SLOTS, SLOTS), bool)
        for t in range(20):
            for a in range(S0, 14):
                if not (has[t, a] and g[t, a] >= 4):
                    continue
                dist = {a: 0}
                front = [a]
                while front:
                    nxt = []
                    for u in front:
                        for v in np.flatnonzero(bonds[t, u]):
                            if int(v) not in dist:
                                dist[int(v)] = dist[u] + 1
                                nxt.append(int(v))
                    front = nxt
                for b in range(SLOTS):
                    if not has[t, b] or b == a or dist.get(b, 99) <= 3:
                        continue
                    if b in FIXED_SLOTS or (b < a and g[t, b] >= 4):
                        tab[t, a, b] = True
        _CACHE["own"] = tab
    return _CACHE["own"]


def basis(ca, c, n, dtype=np.float64):
    """construct_3d_basis(CA, C, N) -> R [3,3] (columns e1, e2, e3), in `dtype` with the kernel's operation order"""
    f = dtype
    ca, c, n = (np.asarray(v, f) for v in (ca, c, n))
    u, v = c - ca, n - ca
    e1 = u / (np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) + f(1e-6))
    pr = (e1[0] * v[0] + e1[1] * v[1]) + e1[2] * v[2]
    v = v - pr * e1
    e2 = v / (np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + f(1e-6))
    e3 = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], f)
    return np.stack([e1, e2, e3], 1)


def chi1_offset(bb, t, dtype=np.float64):
    """eps: the signed angle about CA-CB from the real N to the ideal N (both in the backbone frame).  chi1 is measured from the real
    N and the ideal groups turn from the ideal one, so frame 1 is turned by chi1 - eps.  0 for a type without CB."""
    f, T = dtype, rigid()
    if not T["mask"][t, 4]:
        return f(0.0)
    R = basis(bb[1], bb[2], bb[0], f)
    nr = (R.T @ (np.asarray(bb[0], f) - np.asarray(bb[1], f))).astype(f)
    nr[2] = 0
    ni, q = T["pos"][t, 0].astype(f), T["pos"][t, 4].astype(f)
    ax = q / np.sqrt((q * q).sum())
    pa, pb = nr - (nr @ ax) * ax, ni - (ni @ ax) * ax
    return f(np.arctan2(ax @ np.cross(pa, pb), pa @ pb))


def _rx(chi, f):
    s, c = np.sin(f(chi)), np.cos(f(chi))
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], f)


def build_rotamer_loop(bb, t, chi, dtype=np.float64):
    """one rotamer, written as loops over frames and atoms: bb [3,3] = N, CA, C; -> (atoms [9,3], exists [9], CB [3])"""
    f, T = dtype, rigid()
    R, o = basis(bb[1], bb[2], bb[0], f), np.asarray(bb[1], f)
    chi = np.array(chi, f)
    chi[0] = chi[0] - chi1_offset(bb, t, f)
    frames = [(R, o)]
    for k in range(4):
        Rg, tg = T["rot"][t, 4 + k].astype(f), T["trans"][t, 4 + k].astype(f)
        Rm = (Rg @ _rx(chi[k], f)).astype(f)
        Rp, tp = frames[-1]
        frames.append(((Rp @ Rm).astype(f), (Rp @ tg + tp).astype(f)))
    atoms, exists = np.zeros((RA, 3), f), np.zeros(RA, bool)
    for j in range(RA):
        s = S0 + j
        if s < 14 and T["mask"][t, s] and T["group"][t, s] >= 4:
            Rk, tk = frames[T["group"][t, s] - 3]
            atoms[j] = Rk @ T["pos"][t, s].astype(f) + tk
            exists[j] = True
    return atoms, exists, (R @ T["pos"][t, 4].astype(f) + o).astype(f)


def build_rotamers(bb, t, chis, dtype=np.float64):
    """all rotamers of one residue, vectorised over them: chis [R,4] -> (atoms [R,9,3], exists [9], CB [3])"""
    f, T = dtype, rigid()
    chis = np.array(chis, f)
    chis[:, 0] = chis[:, 0] - chi1_offset(bb, t, f)
    n = len(chis)
    R0, o = basis(bb[1], bb[2], bb[0], f), np.asarray(bb[1], f)
    Rs, ts = [np.broadcast_to(R0, (n, 3, 3))], [np.broadcast_to(o, (n, 3))]
    for k in range(4):
        s, c = np.sin(chis[:, k]), np.cos(chis[:, k])
        rx = np.zeros((n, 3, 3), f)
        rx[:, 0, 0] = 1
        rx[:, 1, 1], rx[:, 1, 2], rx[:, 2, 1], rx[:, 2, 2] = c, -s, s, c
        Rm = np.einsum("ij,njk->nik", T["rot"][t, 4 + k].astype(f), rx).astype(f)
        ts.append((np.einsum("nij,j->ni", Rs[-1], T["trans"][t, 4 + k].astype(f)) + ts[-1]).astype(f))
        Rs.append(np.einsum("nij,njk->nik", Rs[-1], Rm).astype(f))
    atoms, exists = np.zeros((n, RA, 3), f), np.zeros(RA, bool)
    for j in range(RA):
        s = S0 + j
        if s < 14 and T["mask"][t, s] and T["group"][t, s] >= 4:
            g = T["group"][t, s] - 3
            atoms[:, j] = np.einsum("nij,j->ni", Rs[g], T["pos"][t, s].astype(f)) + ts[g]
            exists[j] = True
    return atoms, exists, (R0 @ T["pos"][t, 4].astype(f) + o).astype(f)


def pair_sums(Xr, Rr, Tr, okr, Xc, Rc, Tc, okc, allow, cutoff, w, near=0.0):
    """rows against columns with the pair function of energy_oracle; allow [n,m]: the pairs that are evaluated at all.
    -> per row: E (sum of w . t over the pairs with r < cutoff), rep (the unweighted repulsion term), absw = sum |w_k t_k|, dabsw = sum |w_k dt_k/dr|, n, jump = sum |w_k t_k|
    of the pairs with |r - cutoff| < near (inside or outside: what such a pair can move E by), n_near"""
    n = len(Xr)
    z = dict(E=np.zeros(n), absw=np.zeros(n), dabsw=np.zeros(n), n=np.zeros(n, np.int64), jump=np.zeros(n), n_near=np.zeros(n, np.int64),
             rep=np.zeros(n))
    if n == 0 or len(Xc) == 0:
        return z
    Xr, Xc = np.asarray(Xr, np.float64), np.asarray(Xc, np.float64)
    r = np.sqrt(((Xr[:, None] - Xc[None]) ** 2).sum(-1))
    cand = allow & okr[:, None] & okc[None] & (r < cutoff + near)
    cols = np.flatnonzero(cand.any(0))
    if len(cols) == 0:
        return z
    r, cand = r[:, cols], cand[:, cols]
    d = r - Rr[:, None] - Rc[cols][None]
    ti, tj = Tr[:, None], Tc[cols][None]
    hp = ((ti & 1) != 0) & ((tj & 1) != 0)
    hb = (((ti & 2) != 0) & ((tj & 4) != 0)) | (((ti & 4) != 0) & ((tj & 2) != 0))
    t, g = EO.pair_terms(d, hp, hb)
    w = np.asarray(w, np.float64)
    inside, nr = cand & (r < cutoff), cand & (np.abs(r - cutoff) < near)
    aw = np.abs(t * w).sum(-1)
    z["E"] = ((t * w).sum(-1) * inside).sum(1)
    z["absw"] = (aw * inside).sum(1)
    z["dabsw"] = (np.abs(g * w).sum(-1) * inside).sum(1)
    z["n"] = inside.sum(1)
    z["jump"] = (aw * nr).sum(1)
    z["rep"] = (t[..., 2] * inside).sum(1)
    z["n_near"] = nr.sum(1)
    return z


KEYS = ("E", "absw", "dabsw", "n", "jump", "n_near", "rep")
SUMMED = ("E", "absw", "dabsw", "jump", "n_near", "rep", "pairs")


def _fold(z, R):
    """per row [R*9] -> per rotamer [R]: sums, and for n the largest row count"""
    out = {k: z[k].reshape(R, RA).sum(1) for k in ("E", "absw", "dabsw", "jump", "n_near", "rep")}
    out["n"] = z["n"].reshape(R, RA).max(1)
    out["pairs"] = z["n"].reshape(R, RA).sum(1)
    return out


class Structure:
    """One structure prepared for packing: pos [N,A,3], atom_mask [N,A], aa [N], residue_index [N], movable [N].  Attributes: packed
    [N] bool, plist (the packed residues, ascending), for packed position p: atoms[p] [R,9,3], exists[p] [9], count[p]; env: the fixed
    atoms (X [N,15,3], ok [N,15]); self_[p]: dict of per-rotamer arrays (KEYS, pairs) of sets (a) + (b) plus the table energy in E."""

    def __init__(self, pos, atom_mask, aa, residue_index, movable, rotamers=None, cutoff=8.0, weights=EO.WEIGHTS, near=0.0,
                 dtype=np.float64):
        self.cutoff, self.w, self.near, self.dtype = float(cutoff), np.asarray(weights, np.float64), float(near), dtype
        chi, count, energy = rotamer_table() if rotamers is None else rotamers
        self.rot_chi, self.rot_count, self.rot_energy = np.asarray(chi), np.asarray(count), np.asarray(energy, np.float64)
        rad_tab, typ_tab = EO.tables()
        T = rigid()
        pos, mask, aa = np.asarray(pos), np.asarray(atom_mask) != 0, np.asarray(aa, np.int64)
        N, A = mask.shape
        S = min(A, SLOTS)
        self.N, self.aa, self.idx = N, aa, np.asarray(residue_index, np.int64)
        self.t = np.where((aa < 0) | (aa > 20), 20, aa)
        self.packed = (np.asarray(movable) != 0) & (aa >= 0) & (aa <= 19) & mask[:, 0] & mask[:, 1] & mask[:, 2]
        self.plist = np.flatnonzero(self.packed)
        self.rad, self.typ = rad_tab[self.t], typ_tab[self.t]
        X, ok = np.zeros((N, SLOTS, 3)), np.zeros((N, SLOTS), bool)
        X[:, :S] = pos[:, :S].astype(np.float64)
        ok[:, :S] = mask[:, :S] & (self.rad[:, :S] > 0)
        self.in_pos, self.in_mask = pos, mask
        self.atoms, self.exists, self.count = [], [], []
        for q in self.plist:
            t = self.t[q]
            cnt = int(self.rot_count[t])
            at, ex, cb = build_rotamers(pos[q, :3], t, self.rot_chi[t, :cnt], dtype)
            self.atoms.append(at.astype(np.float64))
            self.exists.append(ex)
            self.count.append(cnt)
            ok[q, 4:14] = False
            if T["mask"][t, 4]:
                X[q, 4], ok[q, 4] = cb, True
        self.env_X, self.env_ok = X, ok
        self.ca = X[:, 1]
        self.ext = [float(np.sqrt(((self.atoms[p][:, self.exists[p]] - self.ca[q]) ** 2).sum(-1)).max()) if self.exists[p].any() else 0.0
                    for p, q in enumerate(self.plist)]
        self.self_ = [self._self(p) for p in range(len(self.plist))]

    def _rows(self, p):
        q, R = self.plist[p], self.count[p]
        ex = np.tile(self.exists[p], R)
        return (self.atoms[p].reshape(R * RA, 3), np.tile(self.rad[q, S0:14], R), np.tile(self.typ[q, S0:14], R), ex)

    def _self(self, p):
        q, R, t = self.plist[p], self.count[p], self.t[self.plist[p]]
        Xr, Rr, Tr, okr = self._rows(p)
        slot_r = np.tile(np.arange(S0, 14), R)
        # (a): every fixed atom of a residue of another residue_index (culled by CA distance: a superset)
        reach = self.cutoff + self.near + self.ext[p] + 12.0
        centre = np.where(self.env_ok[:, 1:2], self.ca, np.where(self.env_ok.any(1)[:, None],
                                                                  self.env_X[np.arange(self.N), self.env_ok.argmax(1)], np.inf))
        close = np.flatnonzero((np.sqrt(((centre - self.ca[q]) ** 2).sum(-1)) < reach) & (self.idx != self.idx[q]))
        Xc, okc = self.env_X[close].reshape(-1, 3), self.env_ok[close].reshape(-1)
        Rc, Tc = self.rad[close].reshape(-1), self.typ[close].reshape(-1)
        res_c, slot_c = np.repeat(close, SLOTS), np.tile(np.arange(SLOTS), len(close))
        allow = np.ones((len(Xr), len(Xc)), bool)
        cys, pro = res_index()["CYS"], res_index()["PRO"]
        if t == cys:
            allow &= ~((slot_r == S0)[:, None] & ((self.t[res_c] == cys) & (slot_c == S0))[None])
        if t == pro:
            prev = self.idx[res_c] + 1 == self.idx[q]
            allow &= ~((slot_r == 6)[:, None] & (prev & np.isin(slot_c, (1, 2, 3)))[None])
            allow &= ~((slot_r == 5)[:, None] & (prev & (slot_c == 2))[None])
        za = pair_sums(Xr, Rr, Tr, okr, Xc, Rc, Tc, okc, allow, self.cutoff, self.w, self.near)
        # (b): the own residue, per rotamer
        own = own_pair_table()[t]
        zb = {k: np.zeros(len(Xr), za[k].dtype) for k in KEYS}
        for r in range(R):
            Xo = np.concatenate([self.env_X[q, :S0], self.atoms[p][r], self.env_X[q, 14:15]])
            oko = np.concatenate([self.env_ok[q, :S0], self.exists[p], self.env_ok[q, 14:15]])
            sl = slice(r * RA, (r + 1) * RA)
            z = pair_sums(Xr[sl], Rr[sl], Tr[sl], okr[sl], Xo, self.rad[q], self.typ[q], oko, own[S0:14], self.cutoff, self.w, self.near)
            for k in KEYS:
                zb[k][sl] = z[k]
        out = _fold({k: za[k] + zb[k] for k in KEYS}, R)
        out["E"] = out["E"] + self.rot_energy[t, :R]
        out["table"] = np.abs(self.rot_energy[t, :R])
        return out

    def near_residues(self, p):
        q = self.plist[p]
        d = np.sqrt(((self.ca[self.plist] - self.ca[q]) ** 2).sum(-1))
        lim = self.cutoff + self.near + self.ext[p] + np.asarray(self.ext) + 1e-6
        return [p2 for p2 in np.flatnonzero((d <= lim) & (self.idx[self.plist] != self.idx[q])) if p2 != p]

    def pair(self, p, p2, cur2, rows=None):
        """set (c): every rotamer of p (or only the rotamer `rows`) against rotamer cur2 of p2 -> per-rotamer dict"""
        q, q2 = self.plist[p], self.plist[p2]
        if rows is None:
            Xr, Rr, Tr, okr = self._rows(p)
            R = self.count[p]
        else:
            Xr, Rr, Tr, okr = self.atoms[p][rows], self.rad[q, S0:14], self.typ[q, S0:14], self.exists[p]
            R = 1
        allow = np.ones((len(Xr), RA), bool)
        cys = res_index()["CYS"]
        if self.t[q] == cys and self.t[q2] == cys:
            allow[np.arange(len(Xr)) % RA == 0, 0] = False
        z = pair_sums(Xr, Rr, Tr, okr, self.atoms[p2][cur2], self.rad[q2, S0:14], self.typ[q2, S0:14], self.exists[p2], allow,
                      self.cutoff, self.w, self.near)
        return _fold(z, R)

    def conditional(self, p, cur):
        """E_self[p, r] + sum over the other packed residues of E_pair(r, cur) -> per-rotamer dict (self and pair parts summed)"""
        out = {k: np.array(v, copy=True) for k, v in self.self_[p].items()}
        for p2 in self.near_residues(p):
            z = self.pair(p, p2, cur[p2])
            for k in SUMMED:
                out[k] = out[k] + z[k]
            out["n"] = out["n"] + z["n"]
        return out

    def total(self, cur):
        """-> dict of scalars: E = sum E_self + sum over pairs p < p2, and the bound's ingredients summed"""
        out = {k: 0.0 for k in SUMMED + ("table",)}
        n_max = 0
        for p in range(len(self.plist)):
            s = self.self_[p]
            for k in out:
                out[k] += float(s[k][cur[p]])
            n_row = int(s["n"][cur[p]])
            for p2 in self.near_residues(p):
                if p2 > p:
                    z = self.pair(p, p2, cur[p2], rows=cur[p])
                    for k in SUMMED:
                        out[k] += float(z[k][0])
                    n_row += int(z["n"][0])
            n_max = max(n_max, n_row)
        out["n"] = n_max
        return out

    def start(self):
        return [int(np.argmin(s["E"])) for s in self.self_]

    def icm(self, sweeps=8):
        """-> dict(start, rotamer, choices [sweeps_run][P], changed, energy_trace [sweeps_run + 1], sweeps_run, margins: at every
        decision the runner-up's energy minus the minimum (inf with one rotamer))"""
        cur = self.start()
        out = dict(start=list(cur), choices=[], changed=[], energy_trace=[self.total(cur)["E"]], margins=[], sweeps_run=0)
        for s in self.self_:
            e = np.sort(s["E"])
            out["margins"].append(float(e[1] - e[0]) if len(e) > 1 else np.inf)
        for _ in range(sweeps):
            changed, row = 0, []
            for p in range(len(self.plist)):
                e = self.conditional(p, cur)["E"]
                best = int(np.argmin(e))
                srt = np.sort(e)
                out["margins"].append(float(srt[1] - srt[0]) if len(e) > 1 else np.inf)
                changed += best != cur[p]
                cur[p] = best
                row.append(best)
            out["choices"].append(row)
            out["changed"].append(changed)
            out["energy_trace"].append(self.total(cur)["E"])
            out["sweeps_run"] += 1
            if changed == 0:
                break
        out["rotamer"] = cur
        return out

    def brute_force(self):
        """-> (the smallest total over every combination, its rotamers): only for a handful of residues"""
        P = len(self.plist)
        pair = {}
        for p in range(P):
            for p2 in range(p + 1, P):
                if p2 in self.near_residues(p):
                    pair[p, p2] = np.stack([self.pair(p, p2, r2)["E"] for r2 in range(self.count[p2])], 1)
        shape = lambda *ps: [self.count[p] if p in ps else 1 for p in range(P)]  # noqa: E731
        total = np.zeros(self.count)
        for p in range(P):
            total = total + self.self_[p]["E"].reshape(shape(p))
        for (p, p2), m in pair.items():
            total = total + m.reshape(shape(p, p2))
        arg = np.unravel_index(int(np.argmin(total)), total.shape)
        return float(total[arg]), [int(v) for v in arg]

    def output(self, cur):
        """-> (pos [N,15,3], mask [N,15] bool, chi [N,4]) of the packed structure, float64"""
        T = rigid()
        A = self.in_mask.shape[1]
        S = min(A, SLOTS)
        pos, mask, chi = np.zeros((self.N, SLOTS, 3)), np.zeros((self.N, SLOTS), bool), np.zeros((self.N, 4))
        pos[:, :S], mask[:, :S] = self.in_pos[:, :S], self.in_mask[:, :S]
        for p, q in enumerate(self.plist):
            t = self.t[q]
            mask[q, 4:14] = T["mask"][t, 4:14]
            pos[q, 4:14] = 0.0
            if mask[q, 4]:
                pos[q, 4] = self.env_X[q, 4]
            pos[q, S0:14][self.exists[p]] = self.atoms[p][cur[p]][self.exists[p]]
            chi[q] = self.rot_chi[t, cur[p]]
        return pos, mask, chi
