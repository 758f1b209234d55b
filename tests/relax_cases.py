"""Seeded inputs, hand-computed cases and the comparison rule shared by test_relax_cpu.py and test_gpu_relax.py: test infrastructure.

The rule (derived from csrc/relax.hip as written, not tuned to an observed error).  u = 2^-24 is the unit roundoff of fp32, eps32 =
2 u, M = max|coord| of the case, POS = K_POS eps32 M with K_POS = 8 the bound on the error of a distance that energy_cases.py derives
for the same chain of operations (three differences of exact inputs, squares, two sums, a correctly rounded square root, a sum of two
radii and a difference: <= 42 u, below 8 eps32 M once M >= MIN_COORD = 2.64).  Here the radii sum takes two more additions (the
tolerance and the margin, <= 2 u * 3.6) and a reference distance d0 is a second such distance; both stay inside the same 8 eps32 M.
A cosine of a connection is a quotient of such quantities: its error is at most 4 POS / (the shorter arm).

Per moving atom, with n = the additions behind its sums (3 for the restraint, 1 per restrained pair, 1 per clash partner that overlaps
or comes within POS of overlapping, 8 per term of a connection):
  |energy terms - oracle|   <= eps32 (n + 4) e + POS * sum |de_i/dd_i|          e: the atom's four terms together
  |gradient_k - oracle|     <= eps32 (n + 6) sum |g_i| + POS * sum H_i          per component k
where |de/dd| is k |d - d0| (twice: d and d0), k o (clash), k |x - x_ref| (restraint), k_bond |dl| + 4 k_angle |dc| / l per connection
term, and H_i bounds the change of term i's gradient per unit of distance error: k (1 + |d - d0| / d), k (1 + o / d), k_rest, k_bond (1
+ |dl| / l) + 12 k_angle (1 + |dc|) / l^2 (|grad cos| <= 2 / l and |hess cos| <= 6 / l^2 over the three atoms of an angle).  E is C1, so a
clash pair on the other side of its threshold in fp32 changes the energy by <= 1/2 k POS^2 and the gradient by <= k POS: inside H_i.
(n + 4) and (n + 6): the roundings of the products behind a term (the square, the stiffness, the half; the quotient, the direction)
on top of the additions.  A sample's terms and energy are float64 sums of the fp32 per-atom numbers: the sum of the atoms' bounds."""
import numpy as np

import dssp_build as DB
import relax_oracle as RO

EPS32 = 2.0 ** -23
K_POS = 8.0
MIN_COORD = 2.64
ALA, PRO = 0, 12


def make_case(seed, B, N, pep=12, noise=0.15):
    """-> dict of ref_pos, pos [B,N,15,3] fp32, atom_mask [B,N,15] bool, aa [B,N] int64, residue_index [B,N] int32, movable [B,N] bool.
    ref_pos: a receptor blob of NeRF chains of up to 30 residues (side-chain atoms 1.5 - 4 A from CA) and, at the end, a peptide of
    min(pep, max(1, N // 3)) residues placed on a receptor CA, so that the two overlap; pos = ref_pos + Gaussian noise.  movable: the
    peptide; structure 0 has nothing movable; structure 1 has gaps in residue_index and absent backbone atoms.  A few residue types
    lie outside 0..19; about 5 % of the atoms are absent."""
    rng = np.random.default_rng(seed)
    n_pep = min(pep, max(1, N // 3))
    ref = np.zeros((B, N, 15, 3))
    index = np.zeros((B, N), np.int32)
    radius = 3.0 + 2.2 * N ** (1.0 / 3.0)
    for b in range(B):
        k, at = 0, 0
        starts = []
        while k < N - n_pep:
            n = int(min(N - n_pep - k, rng.integers(4, 31)))
            seg = DB.random_chain(rng, n) @ DB.rotation(rng.standard_normal(3) * 2.0).T
            ref[b, k:k + n, :4] = seg - seg.mean((0, 1)) + rng.uniform(-1, 1, 3) * radius * 0.5
            index[b, k:k + n] = at + np.arange(n)
            starts.append(k)
            at += n + 1
            k += n
        seg = DB.random_chain(rng, n_pep) @ DB.rotation(rng.standard_normal(3) * 2.0).T
        anchor = ref[b, rng.integers(0, N - n_pep), 1] if N > n_pep else np.zeros(3)
        ref[b, N - n_pep:, :4] = seg - seg.mean((0, 1)) + anchor + rng.standard_normal(3)
        index[b, N - n_pep:] = at + np.arange(n_pep)
        d = rng.standard_normal((N, 11, 3))
        ref[b, :, 4:] = ref[b, :, 1:2] + d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(1.5, 4.0, (N, 11, 1))
    ref += 3.0                                              # away from the origin: M >= MIN_COORD whatever the shape
    aa = rng.integers(0, 20, size=(B, N)).astype(np.int64)
    odd = rng.random((B, N)) < 0.05
    aa[odd] = rng.choice(np.array([-1, 20, 21, 1000], np.int64), size=int(odd.sum()))
    mask = rng.random((B, N, 15)) > 0.05
    mask[:, :, :3] = True
    movable = np.zeros((B, N), bool)
    movable[:, N - n_pep:] = True
    movable[0] = False
    if B > 1:
        index[1] += np.cumsum(rng.random(N) < 0.15).astype(np.int32)
        mask[1, :, :3] = rng.random((N, 3)) > 0.1
    ref = ref.astype(np.float32)
    pos = (ref + noise * rng.standard_normal(ref.shape)).astype(np.float32)
    return dict(ref_pos=ref, pos=pos, atom_mask=mask, aa=aa, residue_index=index, movable=movable)


def max_coord(case):
    return float(max(np.abs(case["pos"]).max(), np.abs(case["ref_pos"]).max()))


def oracle(case, movable=None, **kw):
    """the oracle of every structure of the case, clash partners within POS of overlapping counted"""
    movable = case["movable"] if movable is None else movable
    delta = K_POS * EPS32 * max_coord(case)
    return [RO.energy(case["pos"][b], case["ref_pos"][b], case["atom_mask"][b], case["aa"][b], case["residue_index"][b], movable[b],
                      delta=delta, **kw) for b in range(case["pos"].shape[0])]


def bounds(o, M):
    """-> the allowances (terms_atom and energy_atom [N,15], gradient [N,15], a sample's terms and energy) for the oracle dict o"""
    assert M >= MIN_COORD, M
    pos = K_POS * EPS32 * M
    e = EPS32 * (o["n_terms"] + 4) * o["terms_atom"].sum(-1) + pos * o["e_slope"]
    g = EPS32 * (o["n_terms"] + 6) * o["g_abs"] + pos * o["g_slope"]
    return e, g, float(e.sum())


def check(got, case, oracles):
    """got: the numpy outputs of geometry.relax_energy -> the largest ratio of error to allowance seen (<= 1, asserted)"""
    M, worst = max_coord(case), 0.0
    for b, o in enumerate(oracles):
        e, g, total = bounds(o, M)
        for key, ref, allow in (("terms_atom", o["terms_atom"], e[..., None]), ("energy_atom", o["energy_atom"], e + 3 * EPS32 * o["energy_atom"]),
                                ("gradient", o["gradient"], g[..., None]), ("terms", o["terms"], total), ("energy", o["energy"], total)):
            err = np.abs(got[key][b].astype(np.float64) - ref)
            allow = np.broadcast_to(allow, err.shape)
            assert (err <= allow).all(), (b, key, float(err.max()), float(np.max(err / np.maximum(allow, 1e-300))))
            if np.any(allow > 0):
                worst = max(worst, float(np.max(err[allow > 0] / allow[allow > 0])))
        still = ~o["moving"]
        assert not got["gradient"][b][still].any() and not got["terms_atom"][b][still].any() and not got["energy_atom"][b][still].any(), b
    return worst


# ---- hand-computed cases ----------------------------------------------------------------------------------------------------------

R_C, TOL, MARGIN = 1.7, 1.5, 0.2


def two_atoms(o0=0.3):
    """(a) two residues of one atom each (CA) on a line, residue 0 fixed at the origin, residue 1 movable at 2 R_C - TOL - o0: they
    overlap by o0 beyond the tolerance.  With x the movable atom's coordinate, x0 its start and lim = 2 R_C - TOL + MARGIN, E(x) =
    1/2 k_rest (x - x0)^2 + 1/2 k_clash (lim - x)^2 for x < lim, whose minimum is at
        x - x0 = k_clash (o0 + MARGIN) / (k_rest + k_clash)
    (the 1e-10 inside the clash's square root moves d by 5e-11 / d).  -> (case, x0, the displacement for the default stiffnesses)"""
    x0 = 2 * R_C - TOL - o0
    pos = np.zeros((1, 2, 15, 3), np.float32)
    pos[0, 1, 1, 0] = x0
    mask = np.zeros((1, 2, 15), bool)
    mask[0, :, 1] = True
    case = dict(pos=pos, ref_pos=pos.copy(), atom_mask=mask, aa=np.full((1, 2), ALA, np.int64),
                residue_index=np.array([[0, 5]], np.int32), movable=np.array([[False, True]]))
    k_r, k_c = RO.DEFAULTS["k_rest"], RO.DEFAULTS["k_clash"]
    return case, float(pos[0, 1, 1, 0]), k_c * (o0 + MARGIN) / (k_r + k_c)


STRETCH_K_REST, STRETCH_STEPS, STRETCH_TOL = 0.01, 1000, 2e-4


def stretched_bond(s=0.2):
    """(b) two backbone residues (N, CA, C, O) in a plane with an ideal connection -- |C0 - N1| = 1.329, cos(CA0, C0, N1) = -0.4473,
    cos(C0, N1, CA1) = -0.5203 -- then residue 1 (movable; residue 0 is fixed) moved by s along the C0 -> N1 axis.  A rigid shift of
    residue 1 back by t along that axis leaves both cosines and every internal distance as they are, so along it E(t) = 1/2 k_bond (s
    - t)^2 + 1/2 (4 k_rest) t^2 with its minimum at
        t = k_bond s / (k_bond + 4 k_rest).
    For this to be the minimum in all coordinates, two things are arranged.  The axis passes through the centroid of residue 1's
    four atoms (C1 and O1 are placed for that), so the bond's pull on N and the restraints' pull on all four exert no torque.  And
    k_rest = 0.01 (STRETCH_K_REST): the restraint pulls on four atoms and the bond on one, so the residue deforms by about k_rest t /
    k_intra -- 6e-3 A and an intra term of 5e-2 with the default k_rest = 10, which is the true minimum there and not the minimiser's
    doing -- against 7e-6 A and an intra term of 1e-8 here.  A steepest descent first bends the residue slightly (N is pulled before
    its neighbours follow) and the turn that leaves decays only at alpha k_rest = 2e-5 per iteration; what 1000 iterations
    (STRETCH_STEPS) leave of it in the float64 oracle is 8e-5 A, so the tolerance is 2e-4 A (STRETCH_TOL): a thousandth of the stretch.
    -> (case, the unit axis, t for k_rest = STRETCH_K_REST)"""
    c1, c2 = RO.COS_CA_C_N, RO.COS_C_N_CA
    s1, s2 = np.sqrt(1 - c1 * c1), np.sqrt(1 - c2 * c2)
    C0, N1 = np.zeros(3), np.array([RO.CN_LEN, 0.0, 0.0])
    CA0 = 1.525 * np.array([c1, s1, 0.0])
    N0 = CA0 + 1.458 * np.array([-0.5, 0.8660254, 0.0])
    O0 = C0 + 1.231 * np.array([-0.35, -0.9367497, 0.0])
    CA1 = N1 + 1.458 * np.array([-c2, -s2, 0.0])
    C1 = CA1 + np.array([0.0, 1.525, 0.0])
    sin_o = -(CA1[1] + 2 * C1[1]) / 1.231                   # the four y sum to 0
    O1 = C1 + 1.231 * np.array([np.sqrt(1 - sin_o * sin_o), sin_o, 0.0])
    pos = np.zeros((1, 2, 15, 3))
    pos[0, 0, :4] = [N0, CA0, C0, O0]
    pos[0, 1, :4] = [N1, CA1, C1, O1]
    pos[0, 1, :4, 0] += s
    pos += np.array([4.0, 3.0, 5.0])
    mask = np.zeros((1, 2, 15), bool)
    mask[:, :, :4] = True
    pos = pos.astype(np.float32)
    case = dict(pos=pos, ref_pos=pos.copy(), atom_mask=mask, aa=np.full((1, 2), ALA, np.int64),
                residue_index=np.array([[3, 4]], np.int32), movable=np.array([[False, True]]))
    return case, np.array([1.0, 0.0, 0.0]), RO.DEFAULTS["k_bond"] * s / (RO.DEFAULTS["k_bond"] + 4 * STRETCH_K_REST)


def lone_residue():
    """(c) one movable residue at its reference: E = 0, no gradient, nothing moves"""
    case = make_case(77, 1, 1)
    case["movable"][:] = True
    case["pos"] = case["ref_pos"].copy()
    return case


# ---- the minimiser's seeded cases ---------------------------------------------------------------------------------------------------

# Seeds of the clashing complexes the replay and effect tests start from (B = 1, N = 52: a 12-residue peptide on a 40-residue blob),
# chosen on the CPU (test_relax_cpu.py::test_seeds_of_the_minimiser_cases repeats the checks): the free-running float64 oracle has
# |dE| above ten times the bound of the comparison (`decision_bounds`) in at least 90 % of its 40 iterations, violation_oracle.clashes
# flags moving atoms at the start, and the oracle's own relaxation strictly lowers that count.
REPLAY_SEED, REPLAY_N, REPLAY_STEPS = 4106, 52, 40


def start_case(seed=REPLAY_SEED, N=REPLAY_N, B=1):
    """the structure a minimiser test starts from: the case's ref_pos as the input, the peptide movable in every structure"""
    case = make_case(seed, B, N)
    case["movable"][:] = False
    case["movable"][:, N - min(12, max(1, N // 3)):] = True
    case["pos"] = case["ref_pos"].copy()
    return case


def decision_bounds(case, b=0):
    """Keywords for RO.minimise that make it record `decision_bound` per iteration.  The device accepts a trial when E(y) <= E(x),
    each a float64 sum of fp32 per-atom numbers; the oracle's dE = E(y) - E(x) is a difference of two such sums, and each of them is
    off from the device's by at most its own allowance (`bounds`: the sum of the atoms' bounds, evaluated at that state with M = its
    largest coordinate).  So the sign of dE is the device's decision whenever |dE| > bound(x) + bound(y): the sum of the two, not one
    of them, because the two errors need not cancel.  Clash partners within POS of overlapping are counted with the case's own M
    (the atoms move by an angstrom or so of some thirty)."""
    M0 = max_coord(case)

    def bound(o, x):
        return bounds(o, max(M0, float(np.abs(x).max())))[2]
    return dict(bound=bound, delta=K_POS * EPS32 * M0)


def flagged(case, b, pos15):
    """the moving atoms that violation_oracle.clashes flags at positions pos15 (slots 0..13)"""
    import violation_oracle as VO
    rad_t, _ = RO.tables()
    aa = case["aa"][b]
    rad = rad_t[np.where((aa < 0) | (aa > 20), 20, aa)][:, :14]
    ex = case["atom_mask"][b][:, :14] & (rad > 0)
    out = VO.clashes(pos15[:, :14].astype(np.float64), ex, rad, case["residue_index"][b])
    return int((out["clash_atom"].reshape(-1, 14) & case["movable"][b][:, None]).sum())
