"""Seeded inputs, the small enumerable cases, the hand-made pair and the comparison rule of test_seqdesign_cpu.py and
test_gpu_seqdesign.py: test infrastructure.

The rule is pack_cases.bound, unchanged, and no new tolerance.  pf_sequence_design_fwd's E_self is pf_mutation_scan_fwd's E (the same
rows, pair function, sums and order; + one addition of ref_energy, which `table` carries).  A conditional energy adds P and F: the same
pair function over built atoms on both sides (POS(M) already allows two built atoms), row sums of the same kind, and a fixed number of
further fp32 additions that seqdesign_oracle adds to n (N_EXTRA).  The total is a float64 sum of fp32 row energies, as the packer's.  A
decision (an argmin over the candidate (type, rotamer) pairs) is judged by test_gpu_pack.within on the flattened candidates.

Inputs are scan_cases.make_case(N) with designed = positions, so the cap on pairs near the cutoff is asserted per case on this
oracle's numbers before any device runs."""
import functools

import numpy as np

import lddt_cases as LC
import pack_cases as PC
import pack_oracle as PO
import scan_cases as SC
import seqdesign_oracle as DO

bound = PC.bound
B = SC.B
KEYS = ("pos", "atom_mask", "aa", "residue_index", "designed")


def make_case(N, limit=None):
    """scan_cases.make_case(N) with designed = positions (structure 0: a peptide of <= 12 residues, 1: every residue, 2: none, 3: a
    random 40 %; N = 16 has 14 atom slots); limit: only the first `limit` of them in each structure"""
    case = SC.make_case(N)
    des = case.pop("positions")
    case.pop("group")
    if limit is not None:
        des = des & (np.cumsum(des, 1) <= limit)
    case["designed"] = des
    return case


def max_coord(case):
    return PC.max_coord(case)


_ORACLES = {}


def oracle(case, key=None, **kw):
    """the seqdesign_oracle.Design of every structure of the case (kept under `key`); asserts the cap on pairs near the cutoff"""
    if key is not None and key in _ORACLES:
        return _ORACLES[key]
    near = PC.pos_err(max_coord(case))
    cand = kw.pop("candidates", None)
    res = [DO.Design(*[case[k][b] for k in KEYS], candidates=None if cand is None else cand[b], near=near, **kw)
           for b in range(case["pos"].shape[0])]
    counted = sum(float(z["pairs"].sum()) for o in res for s in o.self_ for z in s.values())
    n_near = sum(float(z["n_near"].sum()) for o in res for s in o.self_ for z in s.values())
    assert n_near <= LC.NEAR_CAP * max(counted, 1.0), ("a bad case: too many pairs near the cutoff", n_near, counted)
    if key is not None:
        _ORACLES[key] = res
    return res


def many_case(n_designed, N=80):
    """two structures of N = 80 residues (every N, CA and C present): `designed` is set at the first n_designed residues of the first
    that can be designed and at four of the second"""
    case = PC.make_case(380, 2, N)
    case["atom_mask"][:, :, :3] = True
    ok = (case["aa"] >= 0) & (case["aa"] <= 19) & case["atom_mask"][:, :, :3].all(-1)
    assert ok[0].sum() >= n_designed
    des = np.zeros((2, N), bool)
    des[0, np.flatnonzero(ok[0])[:n_designed]] = True
    des[1, np.flatnonzero(ok[1])[:4]] = True
    case.pop("movable")
    case["designed"] = des
    return case


# ---- the seeded small cases: three designed residues, three types, <= 6 rotamers each: every state enumerable --------------------------

SMALL_POOL = ("LEU", "ILE", "PHE", "MET", "VAL", "SER", "THR", "ASN", "ALA", "TYR", "HIS")
SMALL_CANDIDATES = range(40)
SMALL_WANTED, SMALL_CLEAR = 12, 6
SMALL_ROT = 6


@functools.lru_cache(maxsize=None)
def small_table():
    """a caller's table: of every type's default rotamers at most SMALL_ROT, evenly spread over its rows"""
    chi, count, energy = PO.rotamer_table()
    out = np.zeros((21, SMALL_ROT, 4), np.float32)
    cnt = np.minimum(count, SMALL_ROT).astype(np.int32)
    for t in range(21):
        rows = np.round(np.linspace(0, count[t] - 1, cnt[t])).astype(int)
        out[t, :cnt[t]] = chi[t, rows]
    return out, cnt, np.zeros((21, SMALL_ROT), np.float32)


def small_case(seed):
    """pack_cases.small_case(seed) (two facing 5-residue helices, residues 2, 3 of the one against 1, 2 of the other): residues 2, 3
    and 6 are designed over three types drawn from SMALL_POOL, residue 7 keeps its side chain and is environment
    -> (case, candidates [1,N,20])"""
    case = PC.small_case(seed)
    rng = np.random.default_rng(5000 + seed)
    idx = PO.res_index()
    des = np.zeros_like(case.pop("movable"))
    des[0, [2, 3, 6]] = True
    case["designed"] = des
    cand = np.zeros(des.shape + (20,), bool)
    cand[0, :, [idx[n] for n in rng.choice(SMALL_POOL, 3, replace=False)]] = True
    return case, cand


def small_design(seed, **kw):
    case, cand = small_case(seed)
    M = max_coord(case)
    return DO.Design(*[case[k][0] for k in KEYS], candidates=cand[0], rotamers=small_table(), near=PC.pos_err(M), **kw), M


@functools.lru_cache(maxsize=None)
def small_report(seed):
    """-> dict(global_min: the oracle's ICM reaches the brute-force minimum, clear: every decision's runner-up is more than ten
    bounds away, late: something changes after the first sweep, bound, best, state)"""
    o, M = small_design(seed)
    run = o.icm(8)
    best, arg = o.brute_force()
    final = o.total(run["state"])
    b = float(bound(final, M))
    margins = np.asarray(run["margins"])
    margins = margins[np.isfinite(margins)]
    return dict(global_min=bool(abs(final["E"] - best) <= 1e-9), clear=bool((margins > 10.0 * b).all()),
                late=bool(any(c > 0 for c in run["changed"][1:])), bound=b, best=best, state=arg, run=run)


def small_seeds():
    """the first SMALL_WANTED of the SMALL_CANDIDATES whose oracle run reaches the brute-force minimum"""
    out = []
    for s in SMALL_CANDIDATES:
        if small_report(s)["global_min"]:
            out.append(s)
        if len(out) == SMALL_WANTED:
            break
    return out


# ---- hand-made cases -------------------------------------------------------------------------------------------------------------------

def hand_lone(name="MET"):
    case = PC.hand_lone(name)
    case["designed"] = case.pop("movable")
    return case


def hand_pocket():
    """scan_cases.hand_pocket with the pocket residue (an ALA facing lone carbons where a LEU's CD1 and CD2 would sit) designed"""
    case, _ = SC.hand_pocket()
    case = dict(case)
    case["designed"] = case.pop("positions")
    return case


PAIR_TYPES = ("ALA", "LEU", "PHE", "MET", "ILE", "VAL")
PAIR_DISTANCE = 6.0


def hand_pair():
    """pack_cases.hand_leu's construction (the second backbone is the first turned by 180 degrees about an axis through the midpoint,
    so that the CA-CB bonds point at each other) with the CAs PAIR_DISTANCE = 6 A apart, both residues ALA as given and both designed
    over PAIR_TYPES.  Each alone -- the other an ALA that does not move, which is all pf_mutation_scan_fwd can ask -- takes a PHE
    pointed at the other; two of them there overlap and no rotamer of a large type avoids it, so the joint answer differs from the
    independent one in TYPE: the first residue visited gives its side chain up because of the partner's.
    -> (case, candidates [1,2,20])"""
    idx = PO.res_index()
    case = PC._one_residue("ALA", extra=1)
    bb = case["pos"][0, 0, :4].astype(np.float64)
    _, _, cb = PO.build_rotamers(bb[:3], idx["LEU"], np.zeros((1, 4)))
    ca = bb[1]
    axis = (cb - ca) / np.linalg.norm(cb - ca)
    centre = ca + 0.5 * PAIR_DISTANCE * axis
    perp = np.cross(axis, [0.0, 0.0, 1.0])
    perp /= np.linalg.norm(perp)
    rot = 2.0 * np.outer(perp, perp) - np.eye(3)
    case["pos"][0, 1, :4] = ((bb - centre) @ rot.T + centre).astype(np.float32)
    case["atom_mask"][0, 1, :4] = True
    des = case.pop("movable")
    des[0, 1] = True
    case["designed"] = des
    cand = np.zeros((1, 2, 20), bool)
    cand[:, :, [idx[n] for n in PAIR_TYPES]] = True
    return case, cand
