"""Seeded inputs, the rotamer table of the tile-edge test and the comparison rule of test_scan_cpu.py and test_gpu_scan.py: test
infrastructure.

The rule is pack_cases.bound, unchanged, and no new tolerance: pf_mutation_scan_fwd evaluates the same rows (rotamer atoms built by the
same frame chain from the same backbone), the same pair function and the same sums in the same order as pf_pack_sidechains_fwd's
self energy, so every term of that derivation (K_sum, K_POS, BUILD, the cutoff's `jump`) applies to E[q,t,r] as it does to E_self, with
n the largest partner count of a row.  energy_interface is a sub-sum of the same rows, without the table energy: the same bound over
its own ingredients.  A decision (the argmin over a type's rotamers) is judged by test_gpu_pack.within.

Inputs are pack_cases.make_case(seed, B, N) with positions = movable.  The cap on pairs near the cutoff (lddt_cases.NEAR_CAP of the
counted pairs within POS(M) of it) is a condition on a case and is asserted on the oracle's numbers before any device runs; SEEDS
records, per N, a seed for which the oracle alone meets it (checked on the CPU by test_scan_cpu.test_recorded_seeds_meet_the_cap)."""
import numpy as np

import lddt_cases as LC
import pack_cases as PC
import pack_oracle as PO
import scan_oracle as SO

bound = PC.bound
B = 4
SEEDS = {1: 201, 2: 202, 15: 215, 16: 216, 17: 217, 33: 233}
KEYS = ("pos", "atom_mask", "aa", "residue_index", "positions")
# the rows of one pass of scan_kernel (a row: one rotamer atom the type has) and the lanes of a wave in its argmin
ROW_TILE, WAVE = 256, 64


def make_case(N, A=None):
    """the recorded case of N residues: pack_cases.make_case with positions = movable; group: the last min(N, 12) residues against
    the rest; N = 16 has 14 atom slots"""
    case = PC.make_case(SEEDS[N], B, N, A=(14 if N == 16 else 15) if A is None else A)
    case["positions"] = case.pop("movable")
    case["group"] = np.broadcast_to(np.arange(N) >= N - min(N, 12), (B, N)).copy()
    return case


def max_coord(case):
    return PC.max_coord(case)


_ORACLES = {}


def oracle(case, key=None, rotamers=None, candidates=None, dtype=np.float64):
    """the scan_oracle.Scan of every structure of the case (kept under `key`); asserts the cap on pairs near the cutoff"""
    if key is not None and key in _ORACLES:
        return _ORACLES[key]
    near = PC.pos_err(max_coord(case))
    group = case.get("group")
    res = [SO.Scan(case["pos"][b], case["atom_mask"][b], case["aa"][b], case["residue_index"][b], case["positions"][b],
                   candidates=None if candidates is None else candidates[b], group=None if group is None else group[b],
                   rotamers=rotamers, near=near, dtype=dtype) for b in range(case["pos"].shape[0])]
    counted = sum(float(z["pairs"].sum()) for o in res for z in o.res.values())
    n_near = sum(float(z["n_near"].sum()) for o in res for z in o.res.values())
    assert n_near <= LC.NEAR_CAP * max(counted, 1.0), ("a bad case: too many pairs near the cutoff", n_near, counted)
    if key is not None:
        _ORACLES[key] = res
    return res


def rows_of_type():
    """-> [20]: the rotamer atoms each type has (slots 5..13 in a chi1..chi4 rigid group)"""
    T = PO.rigid()
    return (T["mask"][:20, 5:14] & (T["group"][:20, 5:14] >= 4)).sum(1)


def edge_table(seed=7):
    """A caller's rotamer table whose counts put rows = count x atoms one below, at and one above the multiples of ROW_TILE where a
    type's atom count allows it, the counts 63, 64, 65 around a wave of the argmin, and the counts 1 and 128 (R = 128).  Random chi,
    random table energies of a few tenths.  -> (chi [21,128,4] float32, count [21] int32, energy [21,128] float32)"""
    idx = PO.res_index()
    want = {"SER": 1, "CYS": 128, "THR": 127, "VAL": 128, "PRO": 2, "ASP": 85, "ASN": 86, "ILE": 64, "LEU": 65, "MET": 63, "GLN": 63,
            "GLU": 64, "LYS": 65, "HIS": 51, "ARG": 42, "PHE": 43, "TYR": 73, "TRP": 57, "ALA": 1, "GLY": 3}
    rng = np.random.default_rng(seed)
    count = np.ones(21, np.int32)
    for name, c in want.items():
        count[idx[name]] = c
    chi = rng.uniform(0.0, 2.0 * np.pi, (21, 128, 4)).astype(np.float32)
    energy = rng.uniform(-0.3, 0.3, (21, 128)).astype(np.float32)
    return chi, count, energy


def edge_case():
    """N = 17, two structures, three scanned residues each (the last three that can be scanned)"""
    case = {k: v[:2].copy() for k, v in make_case(17).items()}
    ok = (case["aa"] >= 0) & (case["aa"] <= 19) & case["atom_mask"][:, :, :3].all(-1)
    pos = np.zeros_like(ok)
    for b in range(2):
        pos[b, np.flatnonzero(ok[b])[-3:]] = True
    case["positions"] = pos
    return case


# ---- hand-made cases -------------------------------------------------------------------------------------------------------------------

def _with_positions(case):
    case = dict(case)
    case["positions"] = case.pop("movable")
    return case


def hand_lone(name="MET"):
    """pack_cases.hand_lone: a lone residue, nothing but its own backbone"""
    return _with_positions(PC.hand_lone(name))


def _lone_plus(name, n_extra):
    case = _with_positions(PC._one_residue(name, extra=n_extra))
    case["positions"][0, 1:] = False
    return case


def hand_pocket(n_per_tip=4):
    """An ALA (the wild type) facing a pocket of lone carbons (each the CB of a residue that has nothing else) laid out around where
    LEU's CD1 and CD2 sit in the rotamer that is best for a lone LEU (3: chi1 180, chi2 60): n_per_tip carbons 4.0 A from each tip (d
    = 4.0 - 1.9 - 1.9 = 0.2: gauss1 0.85, hydrophobic 1, no repulsion), no closer than 3.9 A to any other atom of that LEU and 3.0 A
    to each other.  A LEU gains these contacts, an ALA has none: ddE[LEU] < 0.  The pocket is the other group.
    -> (case, group [1,N])"""
    rng = np.random.default_rng(5)
    t = PO.res_index()["LEU"]
    base = PC._one_residue("ALA")
    bb = base["pos"][0, 0, :4].astype(np.float64)
    at, ex, cb = PO.build_rotamers(bb[:3], t, PO.rotamer_table()[0][t, 3:4])
    leu = np.concatenate([bb, cb[None], at[0][ex]])
    ca = bb[1]
    spots = []
    for tip in (at[0][1], at[0][2]):                        # CD1, CD2
        out = (tip - ca) / np.linalg.norm(tip - ca)
        found = 0
        for _ in range(4000):
            v = rng.normal(size=3)
            v /= np.linalg.norm(v)
            if v @ out < 0.2:
                continue
            c = tip + 4.0 * v
            d = np.linalg.norm(leu - c, axis=1)
            if (np.sort(d)[1] >= 3.9) and all(np.linalg.norm(c - s) >= 3.0 for s in spots):
                spots.append(c)
                found += 1
                if found == n_per_tip:
                    break
        assert found == n_per_tip
    case = _lone_plus("ALA", len(spots))
    for k, c in enumerate(spots):
        case["pos"][0, 1 + k, 4] = c
        case["atom_mask"][0, 1 + k, 4] = True
    group = np.zeros((1, 1 + len(spots)), bool)
    group[0, 0] = True
    return case, group


def hand_cys():
    """An ALA beside a CYS that has nothing but its SG, which sits 0.5 A from where the first rotamer of a CYS on the ALA's backbone
    puts its own SG: as a candidate CYS adds nothing (SG against SG is never evaluated: the lone residue's energies, bit for bit),
    while a SER's OG, built about where the SG is, is deep inside it (d < -2: a repulsion term above 4)."""
    case = _lone_plus("ALA", 1)
    t = PO.res_index()["CYS"]
    at, ex, cb = PO.build_rotamers(case["pos"][0, 0, :3], t, PO.rotamer_table()[0][t, :1])
    case["aa"][0, 1] = t
    case["pos"][0, 1, 5] = at[0, 0] + np.array([0.5, 0.0, 0.0])
    case["atom_mask"][0, 1, 5] = True
    return case


def hand_pro(bonded=True):
    """Two residues of a helix, the second scanned: as a candidate, PRO's CD is 2.5 A from the previous residue's C and closer than
    the radii to its CA and O: fewer than four bonds apart, so these pairs (and CG against C) are not evaluated when the previous
    residue's residue_index is the scanned one's - 1 (bonded), and are a repulsion when the index has a gap."""
    import dssp_build
    bb = dssp_build.helix(2, dssp_build.ALPHA) + PC.SHIFT
    idx = PO.res_index()
    pos, mask = np.zeros((1, 2, 15, 3), np.float32), np.zeros((1, 2, 15), bool)
    pos[0, :, :4], mask[0, :, :4] = bb, True
    aa = np.full((1, 2), idx["GLY"], np.int64)
    aa[0, 1] = idx["ALA"]
    return dict(pos=pos, atom_mask=mask, aa=aa, residue_index=np.array([[4, 5 if bonded else 7]], np.int32),
                positions=np.array([[False, True]]))
