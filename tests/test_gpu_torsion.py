"""GPU checks of the torsion angles and the side-chain packing comparison: pf_torsions_fwd and pf_sidechain_compare_fwd (through
geometry.torsion_angles / sidechain_compare) against the numpy float64 oracle (torsion_oracle.py) on seeded shapes around the 64-residue
tile, translation, preprocess.get_torsion_angle, the constructed cases of the CPU tests, repeatability and peak memory;
metrics.sidechain_packing after a short sample() run.

Bounds (derived, not tuned; ULP = 2^-23, all in radians).

Angle.  Kernel and oracle read the same fp32 coordinates.  Each bond b = p - q is one correctly rounded fp32 subtraction: relative
error 2^-24 of the DIFFERENCE, whatever the size of the coordinates -- that is the exact-subtraction term, and why a translation
changes nothing; it is part of k below.  u = b1 / |b1| carries at most 6 * 2^-24 (three products, two sums, a root, a quotient), t0 =
b0.u at most 10 * 2^-24 |b0|, so v = b0 - t0 u is off by at most 2^-24 (1 + 10 + 7 + 1) |b0| < 20 * 2^-24 |b0| = 10 ULP |b0| in
length, which turns its direction by at most 10 ULP |b0| / |v|; likewise w.  We take k = 12.  y and x of the atan2 are sums of three
products each, 8 ULP relative to |v| |w| together; atan2f is good to 2 ulp of a result below pi (2 * 2^-22 = 4 ULP); adding 2 pi
rounds to half an ulp of [4, 8) (2 ULP) and the fp32 2 pi is 1.5 ULP above 2 pi: 16 ULP in all.  Hence
    |angle - oracle| (mod 2 pi) <= ULP * (12 * (|b0| / |v| + |b2| / |w|) + 16),
with the lengths from the oracle.  For ideal side-chain geometry the ratio sum is about 2.2: 5e-6 rad.
Worst observed ratio to this bound: not recorded yet; every case prints it and asserts that it is at most 1.

get_torsion_angle.  Its angle is acos of a cosine that carries about 8 ULP of rounding: 8 ULP / sin(theta), at theta = 0.01 from 0 or
pi 8 * 2^-23 / sin(0.01) = 9.5e-5.  So: angle bound + 9.5e-5 for angles farther than 0.01 from 0 and pi.

Round trip (the model's angles -> rebuilt atoms -> measured angles).  The rebuilt coordinates are fp32 at the scale S of the structure:
coordinate rounding ulp(S) over the shortest bond of a heavy-atom chain, 1.2 A (C=O is 1.23 A), plus the angle bound of the rebuilt
structure with the lengths from the oracle on those coordinates.

Comparison, on the kernel's own fp32 angles.  |a_x - a_y| rounds to half an ulp of [4, 8) (2 ULP), each wrap subtracts from an fp32
constant 1.5 ULP (2 pi) or 0.7 ULP (pi) off and rounds again (1 ULP): E1 = 8 ULP per error, count * E1 per sum.  Frame-local
coordinates: d = p - CA 2^-24, e1 6 * 2^-24, e2 (N - CA is 111 degrees from e1) 12 * 2^-24, e3 20 * 2^-24, the dot product 3 * 2^-24:
at most 25 * 2^-24 < 16 ULP of |d| <= D per coordinate, twice that per difference: delta = 32 ULP D, D the largest distance of a
compared atom from its CA.  With M = 3 n differences e_i of a residue, |sum (e_i + delta_i)^2 - sum e_i^2| <= 2 delta sqrt(M sum e_i^2)
+ M delta^2 (Cauchy-Schwarz), plus 16 ULP of the sum for the fp32 accumulation.  An exchange is decided alike when the two sums
differ by more than twice that."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import torsion_cases as TC  # noqa: E402
import torsion_oracle as TO  # noqa: E402
import pepflowww_amd  # noqa: E402
from pepflowww_amd import geometry, metrics, synth  # noqa: E402
from pepflowww_amd.preprocess import get_torsion_angle  # noqa: E402

ULP = 2.0 ** -23
E1 = 8 * ULP
ACOS_ERR = 8 * ULP / math.sin(0.01)
TOL20 = math.radians(20.0)
BREAKS = (63, 64, 65)


def cu(t):
    return None if t is None else torch.as_tensor(t).cuda()


def angle_bound(geom):
    with np.errstate(all="ignore"):
        return ULP * (12.0 * (geom["b0"] / geom["v"] + geom["b2"] / geom["w"]) + 16.0)


def run(pos, mask, aa, index=None):
    out = geometry.torsion_angles(cu(pos), cu(mask), cu(aa), cu(index))
    torch.cuda.synchronize()
    assert out["angles"].dtype == torch.float32 and out["defined"].dtype == torch.bool
    assert out["angles"].shape == out["defined"].shape == (*aa.shape, 8)
    return out["angles"].cpu().numpy(), out["defined"].cpu().numpy()


def check_angles(pos, mask, aa, index):
    """the kernel against the oracle, sample by sample -> the worst ratio of a difference to its bound"""
    ang, dfn = run(pos, mask, aa, index)
    assert np.isfinite(ang).all() and (ang >= 0).all() and (ang < 2 * np.pi).all() and not ang[~dfn].any()
    worst = 0.0
    for b in range(len(aa)):
        o = TO.torsions(pos[b], mask[b], aa[b], TC.CHI, None if index is None else index[b])
        assert np.array_equal(dfn[b], o["defined"]), np.argwhere(dfn[b] != o["defined"])[:4]
        d = o["defined"]
        ratio = TO.wrap(ang[b].astype(np.float64) - o["angles"])[d] / angle_bound(o["geom"])[d]
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
    return worst


# ---- the angle kernel ----------------------------------------------------------------------------------------------------------------

SHAPES = [(3, 1), (3, 2), (3, 3), (2, 63), (2, 64), (2, 65), (2, 129), (1, 400)]


@pytest.mark.parametrize("A", [14, 15])
@pytest.mark.parametrize("B,N", SHAPES)
def test_angles_match_oracle(B, N, A):
    """see the module docstring for the bound; segments also start at 63, 64 and 65, so both halos of a 64-residue tile see a break"""
    rng = np.random.default_rng(7000 + 10 * N + A)
    pos, mask, aa, index = TC.make_batch(rng, B, N, A=A, breaks=BREAKS)
    if B == 1:
        mask[0] = TC.make_batch(rng, 2, N, A=A)[1][0]       # (the last sample of a batch is all masked: keep this one)
    assert aa.min() == -1 and (N < 30 or aa.max() == 21)
    for idx in (index, None):
        worst = check_angles(pos, mask, aa, idx)
        print(f"B {B} N {N} A {A} residue_index {idx is not None}: worst ratio to the bound {worst:.3f}")
        assert worst <= 1.0
    ang, dfn = run(pos, mask, aa, index)
    assert not dfn[B - 1].any() or B == 1
    if N > 65:                                              # the breaks are breaks, and only with the index
        for c in BREAKS:
            assert not dfn[:, c, :2].any() and not dfn[:, c - 1, 2].any()
        assert run(pos, mask, aa, None)[1][0, 63:66, :3].any()


def test_translation_changes_no_bit():
    """coordinates that are multiples of 2^-10 A within +-64 A: every bond is exact there and after a shift by (1024, -2048, 512)"""
    rng = np.random.default_rng(7100)
    pos, mask, aa, index = TC.make_batch(rng, 3, 70, breaks=BREAKS)
    pos = (np.round(pos * 1024.0) / 1024.0).astype(np.float32)
    shift = np.array([1024.0, -2048.0, 512.0], np.float32)
    shifted = pos + shift
    assert np.array_equal(shifted.astype(np.float64) - shift.astype(np.float64), pos.astype(np.float64))
    a, b = run(pos, mask, aa, index), run(shifted, mask, aa, index)
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1]) and a[1].sum() > 200


def test_against_get_torsion_angle():
    """slots 3..7 against preprocess.get_torsion_angle on the same fp32 coordinates, every atom of the type present and types 0..19
    (that function reads no atom mask and has no psi for an unknown type): equal masks, values within the angle bound + the acos
    error for every angle farther than 0.01 from 0 and pi"""
    rng = np.random.default_rng(7200)
    n = 200
    aa = rng.integers(0, 20, n)
    R = np.stack([TC.DB.rotation(rng.standard_normal(3) * 2.0) for _ in range(n)])
    pos, mask = TC.residues(aa, rng.uniform(0, 2 * np.pi, (n, 5)), R, rng.uniform(-50, 50, (n, 3)))
    ang, dfn = run(pos[None], mask[None], aa[None])
    ref, ref_mask = get_torsion_angle(torch.from_numpy(pos), torch.from_numpy(aa))
    assert np.array_equal(dfn[0, :, 3:], ref_mask.numpy())
    o = TO.torsions(pos, mask, aa, TC.CHI)
    away = np.minimum(TO.wrap(o["angles"]), np.pi - TO.wrap(o["angles"]))[:, 3:] > 0.01
    use = ref_mask.numpy() & away
    diff = TO.wrap(ang[0, :, 3:].astype(np.float64) - ref.numpy())
    bound = angle_bound(o["geom"])[:, 3:] + ACOS_ERR
    print(f"{use.sum()} angles, worst {diff[use].max():.2e} rad, worst ratio {(diff / bound)[use].max():.3f}")
    assert use.sum() > 400 and (diff[use] <= bound[use]).all()


# ---- the comparison kernel -----------------------------------------------------------------------------------------------------------

def device_side(pos, mask, aa, index=None):
    t = geometry.torsion_angles(cu(pos), cu(mask), cu(aa), cu(index))
    return dict(pos=cu(pos), atom_mask=cu(mask), aa=cu(aa), angles=t["angles"], defined=t["defined"])


def host_side(d, b):
    return {k: v[b].cpu().numpy() for k, v in d.items()}


def sc_bound(o, x, y):
    """per residue: the bound on |sc_sq - oracle| of the module docstring"""
    D = 0.0
    for s in (x, y):
        d = np.linalg.norm(s["pos"][:, :14].astype(np.float64) - s["pos"][:, 1:2], axis=-1)
        D = max(D, float(np.where(s["atom_mask"][:, :14] != 0, d, 0.0).max()))
    delta = 32 * ULP * D
    M = 3.0 * o["sc_n"]
    return 2 * delta * np.sqrt(M * o["sc_sq"]) + M * delta * delta + 16 * ULP * o["sc_sq"]


def check_compare(X, Y, pairs, tol=TOL20):
    """both modes of the kernel against the oracle on the kernel's own angles -> (excused angles, compared angles)"""
    out = geometry.sidechain_compare(X, Y, torch.as_tensor(pairs), correct_tol=tol, per_residue=True)
    lean = geometry.sidechain_compare(X, Y, torch.as_tensor(pairs), correct_tol=tol)
    torch.cuda.synchronize()
    P, N = len(pairs), X["aa"].shape[1]
    per_pair = {"err_sum": torch.float64, "err_count": torch.int32, "within": torch.int32, "res_with_chi": torch.int32,
                "res_correct": torch.int32, "sc_sq_sum": torch.float64, "sc_atoms": torch.int32, "sc_rmsd": torch.float32}
    assert set(lean) == set(per_pair) and set(out) == set(per_pair) | {"err", "sc_sq", "sc_n", "swapped"}
    for k, dt in per_pair.items():
        assert out[k].dtype == dt and out[k].shape[0] == P
        assert torch.equal(out[k].view(torch.int64 if dt == torch.float64 else torch.int32), lean[k].view(torch.int64 if dt == torch.float64 else torch.int32)), k
    assert out["err"].shape == (P, N, 8) and out["sc_sq"].shape == out["sc_n"].shape == out["swapped"].shape == (P, N)
    assert out["swapped"].dtype == torch.bool and out["sc_n"].dtype == torch.int32
    got = {k: v.cpu().numpy() for k, v in out.items()}
    excused = compared = 0
    for p, (i, j) in enumerate(pairs):
        x, y = host_side(X, i), host_side(Y, j)
        o = TO.compare(x, y, TC.PERIODIC, TC.SWAP, tol)
        cmp = o["compared"]
        assert np.array_equal(~np.isnan(got["err"][p]), cmp), p
        assert np.array_equal(got["err_count"][p], o["err_count"]) and got["sc_atoms"][p] == o["sc_atoms"], p
        assert got["res_with_chi"][p] == o["res_with_chi"] and np.array_equal(got["sc_n"][p], o["sc_n"]), p
        assert (np.abs(got["err"][p] - o["err"])[cmp] <= E1).all(), p
        assert (np.abs(got["err_sum"][p] - o["err_sum"]) <= E1 * o["err_count"] + 1e-12).all(), p
        # the tolerance: only an error within E1 of it may fall on the other side
        marginal = cmp & (np.abs(np.nan_to_num(o["err"]) - tol) <= E1)
        inside = cmp & (got["err"][p] <= np.float32(tol))
        assert np.array_equal(inside.sum(0), got["within"][p]), p
        assert (np.abs(got["within"][p] - o["within"]) <= marginal.sum(0)).all(), p
        assert abs(int(got["res_correct"][p]) - o["res_correct"]) <= int(marginal[:, 4:].any(1).sum()), p
        excused += int(np.abs(got["within"][p] - o["within"]).sum())
        compared += int(cmp.sum())
        # the side chains
        bound = sc_bound(o, x, y)
        sure = o["swap_margin"] > 2 * bound
        assert np.array_equal(got["swapped"][p][sure], o["swapped"][sure]), p
        assert (np.abs(got["sc_sq"][p] - o["sc_sq"]) <= bound + 2 * ~sure * bound).all(), p
        assert abs(got["sc_sq_sum"][p] - o["sc_sq_sum"]) <= (bound + 2 * ~sure * bound).sum() + 1e-12, p
        if o["sc_atoms"]:
            want = math.sqrt(got["sc_sq_sum"][p] / got["sc_atoms"][p])
            assert abs(got["sc_rmsd"][p] - want) <= 2 * ULP * want, p
        else:
            assert np.isnan(got["sc_rmsd"][p]), p
    return excused, compared, got


@pytest.mark.parametrize("N", [1, 2, 65, 129])
def test_compare_matches_oracle(N):
    """x != y, Bx = 4, By = 3; y's types are x's with a fifth changed, y[2] has no type in common with x[0]; repeated and reversed
    pairs, and indices out of range"""
    rng = np.random.default_rng(7300 + N)
    px, mx, ax, ix = TC.make_batch(rng, 4, N, breaks=BREAKS)
    ay = ax[[1, 0, 0]].copy()
    change = rng.random(ay.shape) < 0.2
    ay[change] = rng.integers(0, 21, int(change.sum()))
    ay[2] = (np.clip(ax[0], 0, 19) + 1 + rng.integers(0, 18, N)) % 20
    py, my, _, iy = TC.make_batch(rng, 4, N, breaks=BREAKS, aa=np.concatenate([ay, ay[:1]]))
    py, my, iy = py[:3], my[:3], iy[:3]                     # (the all-masked fourth sample is dropped)
    X, Y = device_side(px, mx, ax, ix), device_side(py, my, ay, iy)
    pairs = [(0, 1), (1, 0), (0, 1), (2, 2), (0, 2), (1, 1), (3, 0), (0, 0), (2, 1)]
    excused, compared, got = check_compare(X, Y, pairs)
    print(f"N {N}: excused {excused} of {compared} compared angles")
    assert excused <= 1e-3 * compared
    assert np.array_equal(got["err_sum"][0].view(np.int64), got["err_sum"][2].view(np.int64)) and got["sc_atoms"][0] == got["sc_atoms"][2]
    assert not got["err_count"][4, 3:].any() and got["sc_atoms"][4] == 0 and got["res_with_chi"][4] == 0      # no type in common
    assert not got["err_count"][6].any() and np.isnan(got["sc_rmsd"][6])                                       # x[3] is all masked
    if N >= 65:
        print("pair 0:", got["err_count"][0], got["within"][0], got["res_with_chi"][0], got["res_correct"][0], int(got["swapped"].sum()))
        assert got["err_count"][0, 4] > 5 and got["swapped"].any() and got["res_with_chi"][0] > got["res_correct"][0]
        assert 0 < got["within"][:, 4:].sum() < got["err_count"][:, 4:].sum()
    # a structure against itself, y is x: no error, no exchange; indices out of range give an empty row
    self_pairs = [(0, 0), (2, 2), (1, 0), (4, 0), (0, -1)]
    out = geometry.sidechain_compare(X, X, torch.tensor(self_pairs), per_residue=True)
    assert not out["err_sum"][:2].any() and not out["sc_sq_sum"][:2].any() and not out["swapped"][:2].any()
    assert torch.equal(out["within"][:2], out["err_count"][:2]) and torch.equal(out["res_correct"][:2], out["res_with_chi"][:2])
    assert out["err_sum"][2].sum() > 0 or N < 3
    for p in (3, 4):
        assert not out["err_count"][p].any() and out["sc_atoms"][p] == 0 and torch.isnan(out["sc_rmsd"][p]) and torch.isnan(out["err"][p]).all()
    empty = geometry.sidechain_compare(X, Y, torch.zeros(0, 2, dtype=torch.int32), per_residue=True)
    assert empty["err_sum"].shape == (0, 8) and empty["err"].shape == (0, N, 8)


def test_compare_takes_views_at_odd_offsets():
    """angles / defined that are contiguous views one element into a buffer (not 16 / 8 byte aligned) give the same bits"""
    rng = np.random.default_rng(7350)
    X = device_side(*TC.make_batch(rng, 3, 65, breaks=BREAKS))
    Y = dict(X)
    for k in ("angles", "defined"):
        buf = torch.zeros(X[k].numel() + 1, dtype=X[k].dtype, device="cuda")
        buf[1:] = X[k].reshape(-1)
        Y[k] = buf[1:].view(X[k].shape)
        assert Y[k].is_contiguous() and Y[k].data_ptr() % 8 != 0
    pairs = torch.tensor([(0, 1), (1, 0), (1, 1)], dtype=torch.int32)
    want, got = geometry.sidechain_compare(X, X, pairs, per_residue=True), geometry.sidechain_compare(Y, Y, pairs, per_residue=True)
    assert int(want["err_count"].sum()) > 0
    for k, v in want.items():
        assert torch.equal(torch.nan_to_num(v.double(), nan=-1.0), torch.nan_to_num(got[k].double(), nan=-1.0)), k


# ---- constructed answers through the kernels ----------------------------------------------------------------------------------------

def one(s, index=None):
    return device_side(s[0][None], s[1][None], np.asarray(s[2])[None], None if index is None else np.asarray(index, np.int32)[None])


def compare_one(x, y, **kw):
    out = geometry.sidechain_compare(one(x), one(y), torch.zeros(1, 2, dtype=torch.int32), correct_tol=TOL20, per_residue=True, **kw)
    return {k: v[0].cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("deg", [0.0, 60.0, -60.0, 90.0, 180.0])
def test_known_dihedrals(deg):
    t = one(TC.four_atoms(deg))
    assert t["defined"][0, 0].tolist() == [False, False, False, True] + [False] * 4
    assert abs(float(TO.wrap(float(t["angles"][0, 0, 3]) - math.radians(deg)))) <= ULP * (12 * 2.2 + 16)


def test_breaks_gaps_missing_and_collinear_atoms():
    rng = np.random.default_rng(6100)
    pos, mask, aa = TC.chain4(rng)
    want = np.zeros((4, 8), bool)
    want[1:, :2] = True
    want[:3, 2] = True
    want[:, 3] = True
    assert np.array_equal(one((pos, mask, aa))["defined"][0].cpu().numpy(), want)
    for index in ([0, 1, 3, 4], [0, 1, 1, 2], [5, 6, 4, 5], [0, 1, 2 ** 31 - 1, -2 ** 31]):
        d = one((pos, mask, aa), index)["defined"][0].cpu().numpy()
        assert np.array_equal(np.argwhere(want & ~d)[:3], [[1, 2], [2, 0], [2, 1]]) and not (d & ~want).any()
    uses = {(1, 0): [(0, 2), (1, 0), (1, 1), (1, 2), (1, 3)], (1, 1): [(1, 0), (1, 1), (1, 2), (1, 3), (2, 0)],
            (1, 2): [(1, 1), (1, 2), (1, 3), (2, 0), (2, 1)], (1, 3): [(1, 3)], (1, 4): []}
    for (r, s), gone in uses.items():
        m = mask.copy()
        m[r, s] = False
        d = one((pos, m, aa))["defined"][0].cpu().numpy()
        assert sorted(map(tuple, np.argwhere(want & ~d))) == sorted(gone), (r, s)
    p, m = TC.residues([TC.LYS], rng.uniform(0, 2 * np.pi, (1, 5)))
    m[0, 4] = False
    assert one((p, m, [TC.LYS]))["defined"][0, 0].tolist() == [False] * 3 + [True] + [False] * 3 + [True]
    m[0, 4] = True
    for t in (20, 21, -1, 2 ** 40):
        assert one((p, m, [t]))["defined"][0, 0].tolist() == [False] * 3 + [True] + [False] * 4
    # degenerate geometry: undefined, 0, no NaN
    cases = [TC.collinear()]
    pos, mask, aa = TC.four_atoms(60.0)
    pos[0, 3] = pos[0, 2]
    cases.append((pos.copy(), mask, aa))
    pos[0, 2] = pos[0, 1]
    cases.append((pos.copy(), mask, aa))
    pos[0, :4] = np.nan                                      # a NaN coordinate under a set mask
    cases.append((pos.copy(), mask, aa))
    for c in cases:
        t = one(c)
        assert not t["defined"].any() and not t["angles"].any()


def test_chi_errors_and_the_periodic_wrap():
    c = compare_one(*TC.chi_error_pair(TC.LYS, 2))
    assert np.abs(np.degrees(c["err"][:, 5]) - [10, 19, 21, 170, 180]).max() <= 1e-3
    assert c["err_count"].tolist() == [4, 4, 4, 5, 5, 5, 5, 5] and c["within"].tolist() == [4, 4, 4, 5, 5, 2, 5, 5]
    assert c["res_with_chi"] == 5 and c["res_correct"] == 2
    c = compare_one(*TC.chi_error_pair(TC.ASP, 2))
    assert np.abs(np.degrees(c["err"][:, 5]) - [10, 19, 21, 10, 0]).max() <= 1e-3 and (c["err"][:, 5] >= 0).all()
    assert c["err_count"].tolist() == [4, 4, 4, 5, 5, 5, 0, 0] and c["within"].tolist() == [4, 4, 4, 5, 5, 4, 0, 0]
    assert c["res_with_chi"] == 5 and c["res_correct"] == 4 and np.isnan(c["err"][:, 6:]).all()
    c = compare_one(*TC.chi_error_pair(TC.ASP, 1))
    assert np.abs(np.degrees(c["err"][:, 4]) - [10, 19, 21, 170, 180]).max() <= 1e-3
    x, y = TC.chi_error_pair(TC.LYS, 2)
    c = compare_one(x, (y[0], y[1], np.full(5, TC.LEU)))
    assert c["err_count"].tolist() == [4, 4, 4, 0, 0, 0, 0, 0] and c["res_with_chi"] == 0 and c["sc_atoms"] == 0 and np.isnan(c["sc_rmsd"])


def test_exchanged_equivalent_atoms():
    for aa, names, n_atoms in ((TC.ASP, (("OD1", "OD2"),), 4), (TC.PHE, (("CD1", "CD2"), ("CE1", "CE2")), 7)):
        c = compare_one(*TC.exchanged(aa, names))
        assert c["swapped"].tolist() == [True] and c["sc_n"].tolist() == [n_atoms] and c["sc_sq"][0] <= 1e-9 and c["sc_rmsd"] <= 1e-4
    c = compare_one(*TC.exchanged(TC.LEU, (("CD1", "CD2"),)))
    assert c["swapped"].tolist() == [False] and c["sc_sq"][0] > 1.0
    assert compare_one(*TC.exchanged(TC.PHE, (("CD1", "CD2"),)))["sc_sq"][0] > 1.0
    x, y = TC.exchanged(TC.ASP, (("OD1", "OD2"),))
    y[1][0, 7] = False
    c = compare_one(x, y)
    assert c["swapped"].tolist() == [False] and c["sc_n"].tolist() == [3] and c["sc_sq"][0] > 1.0
    c = compare_one(x, x)
    assert c["swapped"].tolist() == [False] and c["sc_sq"][0] == 0.0 and c["sc_atoms"] == 4
    x[1][0, 0] = False
    assert compare_one(x, x)["sc_atoms"] == 0


# ---- repeatability and memory --------------------------------------------------------------------------------------------------------

def _bits(out):
    view = {torch.float32: torch.int32, torch.float64: torch.int64}
    return {k: (v.view(view[v.dtype]) if v.dtype in view else v).cpu() for k, v in out.items()}


def test_deterministic_and_independent_of_the_list():
    rng = np.random.default_rng(7500)
    B, N = 6, 150
    pos, mask, aa, index = TC.make_batch(rng, B, N, breaks=BREAKS)
    aa[1], aa[3] = aa[0], aa[2]
    runs = [_bits(geometry.torsion_angles(cu(pos), cu(mask), cu(aa), cu(index))) for _ in range(3)]
    for r in runs[1:]:
        for k in r:
            assert torch.equal(r[k], runs[0][k]), k
    part = _bits(geometry.torsion_angles(cu(pos[2:4]), cu(mask[2:4]), cu(aa[2:4]), cu(index[2:4])))
    for k in part:
        assert torch.equal(part[k], runs[0][k][2:4]), k
    X = device_side(pos, mask, aa, index)
    pairs = torch.tensor([(i, j) for i in range(B) for j in range(B)], dtype=torch.int32)
    full = [_bits(geometry.sidechain_compare(X, X, pairs, per_residue=True)) for _ in range(3)]
    for r in full[1:]:
        for k in r:
            assert torch.equal(r[k], full[0][k]), k
    rows = torch.tensor([1, 20, 7, 7, 33])
    sub = _bits(geometry.sidechain_compare(X, X, pairs[rows], per_residue=True))
    for k in sub:
        assert torch.equal(sub[k], full[0][k][rows]), k
    assert full[0]["err_count"][1, 4] > 0 and full[0]["sc_atoms"][1] > 0


def test_peak_memory_is_the_outputs():
    """B = 64, N = 144: beyond its inputs each call allocates its outputs only (plus the allocator's rounding of each to 512 bytes);
    a pairwise list of 64 x 64 pairs stays pair-sized without per_residue"""
    rng = np.random.default_rng(7600)
    B, N = 64, 144
    pos, mask, aa, index = TC.make_batch(rng, 4, N)
    mask[3] = mask[0]
    rep = lambda x: cu(np.concatenate([x] * (B // 4)))  # noqa: E731
    P, M, T, I = rep(pos), rep(mask), rep(aa), rep(index)
    geometry.torsion_angles(P[:1], M[:1], T[:1])                        # the cached tables are not the call's

    def measured(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - base - sum(v.numel() * v.element_size() for v in out.values())
        return out, extra

    t, extra = measured(lambda: geometry.torsion_angles(P, M, T, I))
    assert extra <= 512 * 3, extra
    assert int(t["defined"].sum()) > 10000
    X = dict(pos=P, atom_mask=M, aa=T, angles=t["angles"], defined=t["defined"])
    ids = torch.arange(B, dtype=torch.int32, device="cuda")
    diag = torch.stack([ids, ids], 1)
    out, extra = measured(lambda: geometry.sidechain_compare(X, X, diag, per_residue=True))
    assert extra <= 512 * (len(out) + 1), extra
    allp = torch.cartesian_prod(ids, ids)
    out, extra = measured(lambda: geometry.sidechain_compare(X, X, allp))
    assert extra <= 512 * (len(out) + 1) and sum(v.numel() * v.element_size() for v in out.values()) <= B * B * 160, extra
    assert int(out["sc_atoms"].sum()) > 0


# ---- metrics.sidechain_packing -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(seeded_sd):
    m = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
    m.load_state_dict(seeded_sd)
    return m.cuda().eval()


PER_SAMPLE = {"chi_mae": 4, "chi_correct": 4, "residue_correct": 0, "psi_o_mae": 0, "phi_mae": 0, "psi_mae": 0, "sc_rmsd": 0, "n_chi": 4,
              "cis_fraction": 0}


@pytest.mark.parametrize("fixed", [False, True])
def test_sidechain_packing_after_sample(model, fixed):
    """fixed: sample(..., sample_bb=False, sample_seq=False), the mode whose output the packing table judges.  There chi_err is the
    wrap of the model's angles minus the native's get_torsion_angle.  The sample's side of that is the round-trip bound of the module
    docstring, ulp(S) / 1.2 A + the angle bound of the rebuilt structure; the native's side is the bound of the check against
    get_torsion_angle, its angle bound + the acos error, for native angles farther than 0.01 from 0 and pi; the comparison adds E1."""
    B, L, NS = 2, 64, 2
    batch = synth.make_pocket_batch(B, L, 8, seed=81)
    noise = synth.make_noise(B, L, NS, seed=82)
    dev_batch = {k: cu(v) for k, v in batch.items()}
    kw = dict(sample_bb=False, sample_ang=True, sample_seq=False) if fixed else {}
    final = model.sample(dev_batch, num_steps=NS, noise=noise, **kw)[-1]
    out = metrics.sidechain_packing(final, dev_batch)
    gen = (dev_batch["generate_mask"].bool() & dev_batch["res_mask"].bool())
    for k, n in PER_SAMPLE.items():
        assert out[k].shape == ((B, n) if n else (B,)) and out[k].is_cuda, k
    assert out["n_chi"].dtype == torch.int32 and out["chi_mae"].dtype == torch.float64
    for k in ("chi_mae_pooled", "chi_correct_pooled"):
        assert out[k].shape == (4,) and out[k].dtype == torch.float64
    assert out["residue_correct_pooled"].shape == () and out["chi_mae_by_type"].shape == out["n_chi_by_type"].shape == (20, 4)
    assert out["chi_err"].shape == (B, L, 4) and out["residue_sc_rmsd"].shape == out["swapped"].shape == (B, L)
    assert out["swapped"].dtype == torch.bool and out["angles_sample"].shape == out["angles_native"].shape == (B, L, 8)

    seqs, seqs_1 = cu(final["seqs"]), cu(final["seqs_1"])
    pos_n, mask_n = dev_batch["pos_heavyatom"], dev_batch["mask_heavyatom"].bool() & dev_batch["res_mask"].bool()[:, :, None]
    idx = metrics.residue_index(dev_batch["chain_nb"], dev_batch["res_nb"], dev_batch["res_mask"].bool())
    nat = geometry.torsion_angles(pos_n, mask_n, seqs_1, idx)
    assert torch.equal(out["angles_native"], nat["angles"])
    pos_s, mask_s = pepflowww_amd.full_atom.reconstruct_sample(cu(final["rotmats"]), cu(final["trans"]), cu(final["angles"]), seqs, gen, pos_n)
    sam = geometry.torsion_angles(pos_s, torch.where(gen[:, :, None], mask_s, mask_n) & dev_batch["res_mask"].bool()[:, :, None],
                                  torch.where(gen, seqs, seqs_1), idx)
    assert torch.equal(out["angles_sample"], sam["angles"])
    # chi_err is NaN exactly where the residue is not generated, the types differ or a chi is undefined on a side
    want = (gen & (seqs == seqs_1) & (seqs_1 < 20))[:, :, None] & sam["defined"][:, :, 4:] & nat["defined"][:, :, 4:]
    assert torch.equal(~torch.isnan(out["chi_err"]), want)
    assert torch.equal(out["n_chi"].long(), want.sum(1))
    if fixed:
        assert torch.equal(seqs[gen], seqs_1[gen]) and int(want.sum()) > 8
    # psi_o of the rebuilt residues is the model's first angle + pi
    model_ang = cu(final["angles"]).double()
    d = TO.wrap((out["angles_sample"][:, :, 3].double() - (model_ang[:, :, 0] + math.pi)).cpu().numpy())[gen.cpu().numpy()]
    scale = float(pos_s.abs().max())
    coord = 2.0 ** (math.floor(math.log2(scale)) - 23) / 1.2
    aa_s, idx_h, g = torch.where(gen, seqs, seqs_1).cpu().numpy(), idx.cpu().numpy(), gen.cpu().numpy()
    sam_o = [TO.torsions(pos_s[b].cpu().numpy(), (mask_s[b] & gen[b][:, None]).cpu().numpy(), aa_s[b], TC.CHI, idx_h[b]) for b in range(B)]
    sam_bound = coord + np.stack([angle_bound(o["geom"]) for o in sam_o])
    ratio = d / sam_bound[:, :, 3][g]
    print(f"psi_o round trip: worst {d.max():.2e} rad, worst ratio to the bound {ratio.max():.3f}")
    assert (ratio <= 1.0).all()
    # pooled = the count-weighted means of the per-sample values
    n = out["n_chi"].double()
    for key, pooled in (("chi_mae", "chi_mae_pooled"), ("chi_correct", "chi_correct_pooled")):
        want_pooled = torch.nan_to_num(out[key] * n).sum(0) / n.sum(0)
        ok = n.sum(0) > 0
        assert torch.allclose(out[pooled][ok], want_pooled[ok], rtol=1e-12, atol=0) and torch.isnan(out[pooled][~ok]).all()
    with_chi = (~torch.isnan(out["chi_err"])).any(-1).sum(1).double()
    want_res = torch.nan_to_num(out["residue_correct"] * with_chi).sum() / with_chi.sum()
    assert torch.isnan(out["residue_correct_pooled"]) if with_chi.sum() == 0 else torch.allclose(out["residue_correct_pooled"], want_res, rtol=1e-12, atol=0)
    by_n = out["n_chi_by_type"]
    assert int(by_n.sum()) == int(n.sum()) and torch.equal(torch.isnan(out["chi_mae_by_type"]), by_n == 0)
    tot = torch.nan_to_num(out["chi_mae_by_type"] * by_n).sum(0) / by_n.sum(0)
    ok = by_n.sum(0) > 0
    assert torch.allclose(tot[ok], out["chi_mae_pooled"][ok], rtol=1e-6)        # (chi_err is fp32 per residue)
    cis = out["cis_fraction"]
    assert ((cis >= 0) & (cis <= 1)).all()
    if fixed:
        # against the model's angles and the reference's function on the native
        chi_err = out["chi_err"].cpu().numpy().astype(np.float64)
        cmp = want.cpu().numpy()
        worst = 0.0
        for b in range(B):
            ref, ref_mask = get_torsion_angle(batch["pos_heavyatom"][b], final["seqs_1"][b].cpu())
            o = TO.torsions(batch["pos_heavyatom"][b].numpy(), mask_n[b].cpu().numpy(), final["seqs_1"][b].cpu().numpy(), TC.CHI)
            t = np.clip(final["seqs_1"][b].cpu().numpy(), 0, 20)
            expect = np.degrees(TO.wrap(model_ang[b, :, 1:].cpu().numpy() - ref[:, 1:].double().numpy(), TC.PERIODIC[t]))
            a = TO.wrap(o["angles"][:, 4:])
            use = cmp[b] & ref_mask[:, 1:].numpy() & (np.minimum(a, np.pi - a) > 0.01)
            bound = np.degrees(sam_bound[b][:, 4:] + angle_bound(o["geom"])[:, 4:] + ACOS_ERR + E1)
            assert use.sum() >= 4
            worst = max(worst, float((np.abs(chi_err[b] - expect) / bound)[use].max()))
        print(f"chi_err against the model's angles: worst ratio to the bound {worst:.3f}")
        assert worst <= 1.0
    # a sample without generated residues: NaN
    none = dict(dev_batch)
    none["generate_mask"] = dev_batch["generate_mask"].clone()
    none["generate_mask"][1] = False
    out = metrics.sidechain_packing(final, none, correct_tol_deg=40.0)
    for k in ("chi_mae", "chi_correct", "residue_correct", "psi_o_mae", "phi_mae", "psi_mae", "sc_rmsd", "cis_fraction"):
        assert torch.isnan(out[k][1]).all(), k
    assert not out["n_chi"][1].any() and torch.isnan(out["chi_err"][1]).all()
    # the other sample keeps its values: phi needs no equal types, psi_o does, so with sampled sequences it may have nothing to compare
    assert not torch.isnan(out["phi_mae"][0]) and not torch.isnan(out["psi_mae"][0])
    if fixed:
        assert not torch.isnan(out["psi_o_mae"][0])
