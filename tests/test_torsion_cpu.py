"""CPU checks of the torsion angles and the side-chain packing comparison: the numpy float64 oracle (torsion_oracle.py) against the
recorded fixture F11, against the round trip through the full-atom reconstruction and against constructed answers; the name-derived
tables; the argument checks of the wrappers and the C ABI's."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import torsion_cases as TC  # noqa: E402
import torsion_oracle as TO  # noqa: E402
from pepflowww_amd import _capi, geometry, metrics  # noqa: E402
from pepflowww_amd.preprocess import _tables, residue_type  # noqa: E402

TOL20 = math.radians(20.0)


def angles_of(s, residue_index=None):
    """(pos, mask, aa) -> the dict `compare` takes, with the oracle's own angles"""
    o = TO.torsions(s[0], s[1], s[2], TC.CHI, residue_index)
    return dict(pos=s[0], atom_mask=s[1], aa=s[2], angles=o["angles"], defined=o["defined"])


def compare(x, y, tol=TOL20):
    return TO.compare(angles_of(x), angles_of(y), TC.PERIODIC, TC.SWAP, tol)


def test_tables_from_the_atom_names():
    names, index = _tables()["atom_names"], _tables()["res_index"]
    per = geometry.pi_periodic_table()
    assert per.shape == (21, 4) and per.dtype == torch.bool and int(per.sum()) == 4
    for name, chi in (("ASP", 2), ("GLU", 3), ("PHE", 2), ("TYR", 2)):
        assert per[index[name], chi - 1]
        # the periodic chi ends on the first atom of an exchanged pair, and is the type's last chi
        end = names[index[name]][int(TC.CHI[index[name], chi - 1, 3])]
        assert end == geometry.EQUIVALENT_ATOMS[name][0][0]
        assert chi == 4 or (TC.CHI[index[name], chi] == -1).all()
    swap = geometry.swap_table()
    assert swap.shape == (21, 4) and swap.dtype == torch.uint8
    for t in range(21):
        res = [n for n, i in index.items() if i == t][0]
        got = [(names[t][int(swap[t, 2 * k])], names[t][int(swap[t, 2 * k + 1])]) for k in range(2) if swap[t, 2 * k] != swap[t, 2 * k + 1]]
        assert tuple(got) == geometry.EQUIVALENT_ATOMS.get(res, ())
    chi = geometry.chi_atom_table()
    assert chi.shape == (21, 4, 4) and chi.dtype == torch.int32 and int(chi.max()) <= 13 and (chi[20] == -1).all()
    assert len(geometry.TORSION_NAMES) == 8


def test_oracle_against_the_recorded_fixture(golden_dir):
    """Slots 3..7 against F11's `torsion` (recorded from the reference's get_torsion_angle), mod 2 pi, within the project's parity
    tolerance 1e-4 rad (measured: 4.5e-6, the reference's fp32 acos); `defined` equals the recorded mask.  The fixture has no atom
    mask: every heavy atom of the type is present, an unknown type has none."""
    f = np.load(os.path.join(golden_dir, "f11_torsion.npz"))
    worst, n = 0.0, 0
    for b in range(f["pos"].shape[0]):
        aa = f["aa"][b]
        o = TO.torsions(f["pos"][b], TC.HEAVY_MASK[np.clip(aa, 0, 20)], aa, TC.CHI)
        assert np.array_equal(o["defined"][:, 3:], f["mask"][b])
        e = TO.wrap(o["angles"][:, 3:] - f["torsion"][b])[f["mask"][b]]
        worst, n = max(worst, float(e.max())), n + e.size
    print(f"{n} angles, worst {worst:.2e} rad")
    assert n == 236 and worst <= 1e-4


def test_oracle_round_trip_through_full_atom():
    """Coordinates rebuilt in float64 for all 20 types from random angles in random frames: chi1-4 come back (mod 2 pi) and psi_o is
    the model's angle + pi, within 1e-6 rad (measured 1e-7: the tables are fp32)."""
    rng = np.random.default_rng(6000)
    aa = np.repeat(np.arange(20), 8)
    n = len(aa)
    ang = rng.uniform(0, 2 * np.pi, (n, 5))
    R = np.stack([TC.DB.rotation(rng.standard_normal(3) * 2.0) for _ in range(n)])
    pos = TC.rebuild(R, rng.uniform(-50, 50, (n, 3)), ang, aa)
    o = TO.torsions(pos, TC.HEAVY_MASK[aa, :14], aa, TC.CHI, residue_index=np.arange(n) * 2)
    has = (TC.CHI[aa] >= 0).all(-1)
    assert np.array_equal(o["defined"][:, 4:], has) and o["defined"][:, 3].all() and not o["defined"][:, :3].any()
    worst = max(float(TO.wrap(o["angles"][:, 4:] - ang[:, 1:])[has].max()), float(TO.wrap(o["angles"][:, 3] - (ang[:, 0] + np.pi)).max()))
    print(f"worst {worst:.2e} rad")
    assert worst <= 1e-6


@pytest.mark.parametrize("deg", [0.0, 60.0, -60.0, 90.0, 180.0])
def test_oracle_known_dihedrals(deg):
    o = TO.torsions(*TC.four_atoms(deg), TC.CHI)
    assert o["defined"][0].tolist() == [False, False, False, True] + [False] * 4
    assert abs(float(TO.wrap(o["angles"][0, 3] - math.radians(deg)))) <= 1e-7          # the coordinates are fp32
    assert 0.0 <= o["angles"][0, 3] < 2 * np.pi


def test_oracle_breaks_gaps_and_missing_atoms():
    rng = np.random.default_rng(6100)
    pos, mask, aa = TC.chain4(rng)
    full = TO.torsions(pos, mask, aa, TC.CHI)["defined"]
    want = np.zeros((4, 8), bool)
    want[1:, :2] = True
    want[:3, 2] = True
    want[:, 3] = True
    assert np.array_equal(full, want)                       # alanine: no chi; the ends lack a neighbour
    for index in ([0, 1, 3, 4], [0, 1, 1, 2], [5, 6, 4, 5]):         # a gap, a repeat, a step back between residues 1 and 2
        d = TO.torsions(pos, mask, aa, TC.CHI, np.array(index))["defined"]
        lost = want & ~d
        assert np.array_equal(np.argwhere(lost), [[1, 2], [2, 0], [2, 1]]) and not (d & ~want).any()
    # a missing atom removes exactly the angles that use it: (residue, slot) -> (residue, angle) list
    uses = {(1, 0): [(0, 2), (1, 0), (1, 1), (1, 2), (1, 3)], (1, 1): [(1, 0), (1, 1), (1, 2), (1, 3), (2, 0)],
            (1, 2): [(1, 1), (1, 2), (1, 3), (2, 0), (2, 1)], (1, 3): [(1, 3)], (1, 4): []}
    for (r, s), gone in uses.items():
        m = mask.copy()
        m[r, s] = False
        d = TO.torsions(pos, m, aa, TC.CHI)["defined"]
        assert sorted(map(tuple, np.argwhere(want & ~d))) == sorted(gone), (r, s)
    # chi: a lysine without CB loses chi1-3 and keeps chi4 (CG, CD, CE, NZ)
    p, m = TC.residues([TC.LYS], rng.uniform(0, 2 * np.pi, (1, 5)))
    assert TO.torsions(p, m, [TC.LYS], TC.CHI)["defined"][0, 3:].all()
    m[0, 4] = False
    assert TO.torsions(p, m, [TC.LYS], TC.CHI)["defined"][0].tolist() == [False] * 3 + [True] + [False] * 3 + [True]
    # the type decides: the same atoms as an unknown type, or as one outside the table, have no chi
    m[0, 4] = True
    for t in (20, 21, -1):
        assert TO.torsions(p, m, [t], TC.CHI)["defined"][0].tolist() == [False] * 3 + [True] + [False] * 4


def test_oracle_collinear_atoms_give_no_nan():
    o = TO.torsions(*TC.collinear(), TC.CHI)
    assert not o["defined"].any() and not o["angles"].any() and np.isfinite(o["angles"]).all()
    pos, mask, aa = TC.four_atoms(60.0)
    pos[0, 3] = pos[0, 2]                                    # O on C: a zero-length outer bond
    o = TO.torsions(pos, mask, aa, TC.CHI)
    assert not o["defined"].any() and np.isfinite(o["angles"]).all()
    pos[0, 2] = pos[0, 1]                                    # C on CA: a zero-length central bond
    o = TO.torsions(pos, mask, aa, TC.CHI)
    assert not o["defined"].any() and np.isfinite(o["angles"]).all()


def test_oracle_chi_errors_and_the_periodic_wrap():
    """errors of 10, 19, 21, 170, 180 degrees: as they are on an ordinary chi (LYS chi2), 10, 19, 21, 10, 0 on a pi-periodic one
    (ASP chi2); tolerance 20 degrees"""
    c = compare(*TC.chi_error_pair(TC.LYS, 2))
    assert np.abs(np.degrees(c["err"][:, 5]) - [10, 19, 21, 170, 180]).max() <= 1e-4
    assert c["err_count"].tolist() == [4, 4, 4, 5, 5, 5, 5, 5] and c["within"].tolist() == [4, 4, 4, 5, 5, 2, 5, 5]
    assert c["res_with_chi"] == 5 and c["res_correct"] == 2
    assert abs(c["err_sum"][5] - math.radians(400.0)) <= 1e-5
    c = compare(*TC.chi_error_pair(TC.ASP, 2))
    assert np.abs(np.degrees(c["err"][:, 5]) - [10, 19, 21, 10, 0]).max() <= 1e-4
    assert c["err_count"].tolist() == [4, 4, 4, 5, 5, 5, 0, 0] and c["within"].tolist() == [4, 4, 4, 5, 5, 4, 0, 0]
    assert c["res_with_chi"] == 5 and c["res_correct"] == 4
    assert np.isnan(c["err"][:, 6:]).all() and not np.isnan(c["err"][:, 3:6]).any()
    # chi1 of the same type is not periodic
    c = compare(*TC.chi_error_pair(TC.ASP, 1))
    assert np.abs(np.degrees(c["err"][:, 4]) - [10, 19, 21, 170, 180]).max() <= 1e-4
    # another type on one side: only the backbone angles are compared
    x, y = TC.chi_error_pair(TC.LYS, 2)
    c = compare(x, (y[0], y[1], np.full(5, TC.LEU)))
    assert c["err_count"].tolist() == [4, 4, 4, 0, 0, 0, 0, 0] and c["res_with_chi"] == 0 and c["sc_atoms"] == 0 and np.isnan(c["sc_rmsd"])


def test_oracle_exchanged_equivalent_atoms():
    for aa, names, n_atoms in ((TC.ASP, (("OD1", "OD2"),), 4), (TC.PHE, (("CD1", "CD2"), ("CE1", "CE2")), 7)):
        c = compare(*TC.exchanged(aa, names))
        assert c["swapped"].tolist() == [True] and c["sc_n"].tolist() == [n_atoms] and c["sc_sq"][0] <= 1e-10 and c["sc_rmsd"] <= 1e-5
    c = compare(*TC.exchanged(TC.LEU, (("CD1", "CD2"),)))            # not equivalent: CG is tetrahedral
    assert c["swapped"].tolist() == [False] and c["sc_sq"][0] > 1.0
    c = compare(*TC.exchanged(TC.PHE, (("CD1", "CD2"),)))            # half an exchange is no flip of the ring
    assert c["sc_sq"][0] > 1.0
    # an exchanged atom missing on one side: no exchange is tried
    x, y = TC.exchanged(TC.ASP, (("OD1", "OD2"),))
    y[1][0, 7] = False
    c = compare(x, y)
    assert c["swapped"].tolist() == [False] and c["sc_n"].tolist() == [3] and c["sc_sq"][0] > 1.0
    # identical structures: a tie keeps the unexchanged one; a missing backbone atom leaves the residue out
    c = compare(x, x)
    assert c["swapped"].tolist() == [False] and c["sc_sq"][0] == 0.0 and c["sc_atoms"] == 4
    x[1][0, 0] = False
    assert compare(x, x)["sc_atoms"] == 0


def test_wrapper_argument_checks():
    pos = torch.zeros(2, 5, 15, 3)
    ok = dict(atom_mask=torch.ones(2, 5, 15, dtype=torch.bool), aa=torch.zeros(2, 5, dtype=torch.int64))
    with pytest.raises(ValueError):
        geometry.torsion_angles(torch.zeros(2, 5, 13, 3), torch.ones(2, 5, 13, dtype=torch.bool), ok["aa"])
    with pytest.raises(ValueError):
        geometry.torsion_angles(pos, ok["atom_mask"][:, :, :14], ok["aa"])
    with pytest.raises(ValueError):
        geometry.torsion_angles(pos, ok["atom_mask"], ok["aa"][:, :4])
    with pytest.raises(ValueError):
        geometry.torsion_angles(pos, **ok, residue_index=torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(_capi.PepflowHipError):              # CPU tensors: no fall-back
        geometry.torsion_angles(pos, **ok)
    x = dict(pos=pos, **ok, angles=torch.zeros(2, 5, 8), defined=torch.zeros(2, 5, 8, dtype=torch.bool))
    pairs = torch.zeros(1, 2, dtype=torch.int32)
    for bad in (dict(x, angles=torch.zeros(2, 5, 5)), dict(x, defined=torch.zeros(2, 5, dtype=torch.bool)),
                {k: v for k, v in x.items() if k != "aa"}, dict(x, pos=torch.zeros(2, 5, 13, 3))):
        with pytest.raises(ValueError):
            geometry.sidechain_compare(bad, x, pairs)
        with pytest.raises(ValueError):
            geometry.sidechain_compare(x, bad, pairs)
    y6 = dict(pos=torch.zeros(2, 6, 15, 3), atom_mask=torch.ones(2, 6, 15), aa=torch.zeros(2, 6), angles=torch.zeros(2, 6, 8),
              defined=torch.zeros(2, 6, 8))
    with pytest.raises(ValueError):
        geometry.sidechain_compare(x, y6, pairs)
    with pytest.raises(ValueError):
        geometry.sidechain_compare(x, x, torch.zeros(3, dtype=torch.int32))
    for bad in (-0.1, 4.0, float("nan")):
        with pytest.raises(ValueError):
            geometry.sidechain_compare(x, x, pairs, correct_tol=bad)
    with pytest.raises(_capi.PepflowHipError):
        geometry.sidechain_compare(x, x, pairs)
    for bad in (-1.0, 181.0, float("nan")):
        with pytest.raises(ValueError):
            metrics.sidechain_packing({}, {}, correct_tol_deg=bad)


def test_c_abi_bounds():
    lib = _capi.load()
    assert lib.pf_abi_version() == _capi.ABI_VERSION == 65
    buf = (C.c_char * 64)()

    def filled(cls, optional, **kw):
        a = cls()
        for name, typ in cls._fields_:
            if typ is C.c_void_p and name not in optional:
                setattr(a, name, C.addressof(buf))
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert "pf_torsions_fwd" in _capi.EXPORTED_SYMBOLS and "pf_sidechain_compare_fwd" in _capi.EXPORTED_SYMBOLS
    assert lib.pf_torsions_fwd(None, None) == -1
    assert lib.pf_torsions_fwd(C.byref(_capi.TorsionsArgs()), None) == -1
    good = dict(B=1, N=4, n_atoms=15)
    for kw in (dict(n_atoms=13), dict(B=-1), dict(N=-1), dict(pos=None), dict(chi_atoms=None), dict(defined=None)):
        assert lib.pf_torsions_fwd(C.byref(filled(_capi.TorsionsArgs, ("residue_index",), **{**good, **kw})), None) == -1, kw
    assert lib.pf_torsions_fwd(C.byref(filled(_capi.TorsionsArgs, ("residue_index",), **{**good, "B": 65536})), None) == -2
    for kw in (dict(B=0), dict(N=0)):                        # nothing to do: nothing is launched
        assert lib.pf_torsions_fwd(C.byref(filled(_capi.TorsionsArgs, ("residue_index",), **{**good, **kw})), None) == 0

    per_residue = ("err", "sc_sq", "sc_n", "swapped")
    assert lib.pf_sidechain_compare_fwd(None, None) == -1
    assert lib.pf_sidechain_compare_fwd(C.byref(_capi.SidechainCompareArgs()), None) == -1
    good = dict(Bx=1, By=2, N=4, P=3, n_atoms_x=15, n_atoms_y=14, correct_tol=0.3)
    for kw in (dict(n_atoms_x=13), dict(n_atoms_y=0), dict(Bx=0), dict(By=-1), dict(N=0), dict(P=-1), dict(correct_tol=-0.5),
               dict(correct_tol=float("nan")), dict(pairs=None), dict(swap=None), dict(sc_rmsd=None), dict(err=C.addressof(buf)),
               dict(err=C.addressof(buf), sc_sq=C.addressof(buf), sc_n=C.addressof(buf))):
        assert lib.pf_sidechain_compare_fwd(C.byref(filled(_capi.SidechainCompareArgs, per_residue, **{**good, **kw})), None) == -1, kw
    assert lib.pf_sidechain_compare_fwd(C.byref(filled(_capi.SidechainCompareArgs, per_residue, **{**good, "N": 2 ** 28})), None) == -2
    assert lib.pf_sidechain_compare_fwd(C.byref(filled(_capi.SidechainCompareArgs, per_residue, **{**good, "P": 0})), None) == 0
