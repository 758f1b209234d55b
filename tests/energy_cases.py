"""Seeded inputs, hand-computed cases and the comparison rule shared by test_energy_cpu.py and test_gpu_energy.py: test infrastructure.

The rule (derived from csrc/interface_energy.hip as written, not tuned to an observed error).  u = 2^-24 is the unit roundoff of
fp32, eps32 = 2^-23 = 2 u, M = max|coord| of the case.

Counts.  The kernel decides r < cutoff, hbond > 0 (d < 0) and hydrophobic > 0 (d < 1.5) in fp32 from the same coordinates as the
float64 oracle, so a decision whose float64 margin is below POS = 8 * 2^-23 * M (lddt_cases.ULP8 * M, the project's positional bound)
may fall on the other side, and no other: |count - oracle| <= the row's near decisions.  The cap is a condition on the case, stated
on the oracle's numbers before any device runs: near decisions <= lddt_cases.NEAR_CAP (5e-4) of the counted pairs.

Float terms, per row atom and term k:  |dev - oracle| <= eps32 * (K_sum * t_k + K_POS * M * sum|dt_k/dr|)  (+ the terms of the row's
pairs that are near the cutoff, which may be in or out).
  K_sum = n + 1, n = the row's partners inside the cutoff.  The kernel adds only those (a skipped pair adds nothing, which is
        exact), one after the other in ascending column order: n - 1 roundings of u.  expf carries HIP's documented 1 ulp = 2 u.
        What else rounds a term's value relative to itself is at most 2 u (repulsion: the product d * d; hbond: the constant -1/0.7
        and one product).  (n - 1 + 2 + 2) u <= (n + 1) eps32 for n >= 1.
  K_POS = 8: the roundings between the coordinates and d, as an error of d.  dx, dy, dz round once each (u relative: the coordinates
        are exact inputs), the squares and the two sums give r^2 to 5 u, the correctly rounded square root leaves r to 3.5 u r <= 28 u;
        the two radii are off by <= u each and their sum by 2 u; d = r - (R_i + R_j) rounds by u |d| <= 4.6 u; the roundings inside a
        term that act like an error of d (the square in a Gaussian's argument, d - 3, 1.5 - d) are <= 1.5 |d - 3| u <= 5.5 u.
        Together <= 42.1 u = 21.1 eps32 <= 8 eps32 M once M >= 2.64: MIN_COORD, which every case here meets (a pair at distance r
        and |d| <= 4.6 needs less: the hand-computed pairs at 2.8 and 4.3 A need 22.8 u and 30 u against 44.8 u and 68.8 u).
Per residue the kernel adds the 15 slots in slot order: the atoms' bounds plus 15 eps32 t; energy_residue is five products and four
sums in fp32: 6 eps32 sum|w_k t_k| on top of sum|w_k| bound_k.  The per-structure totals are float64 sums of those fp32 numbers."""
import numpy as np

import energy_oracle as EO
import lddt_cases as LC

EPS32 = 2.0 ** -23
K_POS = 8.0
EXP_ULP = 1.0
MIN_COORD = 2.64
GAUSS_SLOPE = 40.0          # |dt_k/dr| <= 40 t_k for every term at d <= 4.6 (gauss1: 8 |d|): the slope of a near-cutoff pair's terms


def make_case(seed, B, N, scale):
    """-> dict of pos [B,N,15,3] fp32, atom_mask [B,N,15] bool (random missing atoms and residues), aa [B,N] int64 (types 0..20, a few
    outside), group [B,N] bool: random; structure 0 a peptide of <= 12 residues at the end (most column tiles are skipped);
    structure 2 (B > 2) one group only; query [B,N] bool (lddt_cases.queries)."""
    rng = np.random.default_rng(seed)
    _, y = LC.make_pair_batch(rng, B, N, scale, mask_last_x=False)
    aa = y["aa"].copy()
    odd = rng.random((B, N)) < 0.05
    aa[odd] = rng.choice(np.array([-1, 21, 25, 1000], np.int64), size=int(odd.sum()))
    group = rng.random((B, N)) < 0.4
    group[0] = np.arange(N) >= N - min(N, 12)
    if B > 2:
        group[2] = False
    return dict(pos=y["pos"], atom_mask=y["atom_mask"], aa=aa, group=group, query=LC.queries(rng, B, N))


def max_coord(case):
    return float(np.abs(case["pos"][:, :, :15]).max())


def oracle(case, query=None, cutoff=8.0, weights=EO.WEIGHTS, group=None):
    """the oracle of every structure of the case; asserts the case's cap on near decisions"""
    bound = LC.ULP8 * max_coord(case)
    group = case["group"] if group is None else group
    res = [EO.interface_energy(case["pos"][b], case["atom_mask"][b], case["aa"][b], group[b], None if query is None else query[b],
                               cutoff, weights, bound) for b in range(case["pos"].shape[0])]
    counted = sum(int(np.clip(o["pairs"], 0, None).sum()) for o in res)
    near = sum(int(o["near_cutoff"].sum() + o["near_hbond"].sum() + o["near_hydrophobic"].sum()) for o in res)
    assert near <= LC.NEAR_CAP * counted, ("a bad case: too many decisions near a threshold", near, counted)
    return res


def bounds(o, M, weights=EO.WEIGHTS):
    """-> the allowances of terms_atom [N,15,5], terms_residue [N,5], energy_residue [N] for the oracle dict o of one structure"""
    assert M >= MIN_COORD, M
    w = np.abs(np.asarray(weights, np.float64))
    n = np.clip(o["pairs"], 0, None) + o["near_cutoff"]
    t = o["terms"] + o["jump"]
    atom = EPS32 * ((n + EXP_ULP)[..., None] * t + K_POS * M * (o["dterms"] + GAUSS_SLOPE * o["jump"])) + o["jump"]
    res = atom.sum(1) + 15 * EPS32 * t.sum(1)
    energy = res @ w + 6 * EPS32 * (t.sum(1) @ w)
    return atom, res, energy


def check(got, case, oracles, query=None, weights=EO.WEIGHTS):
    """got: the numpy outputs of geometry.interface_energy (query: as the oracles were made) -> the largest ratio of error to
    allowance seen (<= 1, asserted)"""
    M, worst, half = max_coord(case), 0.0, 0.5 if query is None else 1.0
    for b, o in enumerate(oracles):
        near_c = o["near_cutoff"]
        for key, ref, near in (("pairs_atom", "pairs", near_c), ("hbond_pairs_atom", "hbond_pairs", near_c + o["near_hbond"]),
                               ("hydrophobic_pairs_atom", "hydrophobic_pairs", near_c + o["near_hydrophobic"])):
            diff = np.abs(got[key][b].astype(np.int64) - o[ref])
            assert (diff <= near).all(), (b, key, int(diff.max()))
            assert ((got[key][b] == -1) == (o[ref] == -1)).all(), (b, key)
        atom, res, energy = bounds(o, M, weights)
        for key, ref, allow in (("terms_atom", o["terms"], atom), ("terms_residue", o["terms_residue"], res),
                                ("energy_residue", o["energy_residue"], energy), ("terms", o["terms_total"], half * res.sum(0)),
                                ("energy", o["energy_total"], half * energy.sum())):
            err = np.abs(got[key][b].astype(np.float64) - ref)
            assert (err <= allow).all(), (b, key, float(err.max()), float(np.max(err / np.maximum(allow, 1e-300))))
            if np.any(allow > 0):
                worst = max(worst, float(np.max(err[allow > 0] / allow[allow > 0])))
        assert not got["terms_atom"][b][~o["is_row"]].any(), b
    return worst


# ---- hand-computed cases --------------------------------------------------------------------------------------------------------------

ALA, PRO = 0, 12
CB, N_SLOT, O_SLOT = 4, 0, 3


def _two(slot0, slot1, r, aa0=ALA, groups=(0, 1), dtype=np.float32):
    pos = np.zeros((1, 2, 15, 3), dtype)
    pos[0, 1, slot1, 0] = r
    mask = np.zeros((1, 2, 15), bool)
    mask[0, 0, slot0] = mask[0, 1, slot1] = True
    return dict(pos=pos, atom_mask=mask, aa=np.array([[aa0, ALA]], np.int64), group=np.array([groups], np.uint8)), (slot0, slot1)


def hand_cases(dtype=np.float32):
    """[(name, case, (slot of residue 0, slot of residue 1), the five terms of the one pair or None when nothing is evaluated)]"""
    e = np.exp
    cb = [e(-1.0), e(-(2.5 / 2.0) ** 2), 0.0, 1.0, 0.0]                    # r = 4.3: d = 4.3 - 3.8 = 0.5
    no = [e(-1.4 ** 2), e(-(3.7 / 2.0) ** 2), 0.49, 0.0, 1.0]              # r = 2.8: d = 2.8 - 3.5 = -0.7
    return [("two CB at 4.3", *_two(CB, CB, 4.3, dtype=dtype), cb),
            ("N and O at 2.8", *_two(N_SLOT, O_SLOT, 2.8, dtype=dtype), no),
            ("proline's N and O at 2.8", *_two(N_SLOT, O_SLOT, 2.8, aa0=PRO, dtype=dtype), no[:4] + [0.0]),
            ("N and O in one group", *_two(N_SLOT, O_SLOT, 2.8, groups=(1, 1), dtype=dtype), None),
            ("N and O at the cutoff", *_two(N_SLOT, O_SLOT, 8.0, dtype=dtype), None)]
