"""CPU checks of the empirical interface energy (the functional form of AutoDock Vina's scoring function, written from the publication;
not checked against the Vina program): the type and radius tables against pinned lists and against the oracle's own statement of
them, the ctypes struct layout against the header, the exported symbol, the wrappers' argument checks, and the numpy float64 oracle
(energy_oracle.py) against hand-computed cases and its own symmetry."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import energy_cases as EC  # noqa: E402
import energy_oracle as EO  # noqa: E402
from test_lddt_cpu import HEADER, header_fields  # noqa: E402
from pepflowww_amd import _capi, geometry, metrics  # noqa: E402
from pepflowww_amd.preprocess import _tables  # noqa: E402

# the carbons that are NOT hydrophobic, besides CA and C of every type
POLAR_CARBONS = {"PRO": {"CD"}, "SER": {"CB"}, "THR": {"CB"}, "CYS": {"CB"}, "MET": {"CG", "CE"}, "ASP": {"CG"}, "GLU": {"CD"},
                 "ASN": {"CG"}, "GLN": {"CD"}, "LYS": {"CE"}, "ARG": {"CD", "CZ"}, "HIS": {"CG", "CD2", "CE1"}, "TRP": {"CD1", "CE2"},
                 "TYR": {"CZ"}}
DONORS = {"ARG": {"NE", "NH1", "NH2"}, "ASN": {"ND2"}, "GLN": {"NE2"}, "LYS": {"NZ"}, "TRP": {"NE1"}, "SER": {"OG"}, "THR": {"OG1"},
          "TYR": {"OH"}, "HIS": {"ND1", "NE2"}}
ACCEPTORS = {"ASP": {"OD1", "OD2"}, "GLU": {"OE1", "OE2"}, "ASN": {"OD1"}, "GLN": {"OE1"}, "SER": {"OG"}, "THR": {"OG1"}, "TYR": {"OH"},
             "HIS": {"ND1", "NE2"}}


# ---- the tables ----------------------------------------------------------------------------------------------------------------------

def test_type_table_matches_the_pinned_lists():
    tab, t = geometry.interface_type_table(), _tables()
    assert tab.shape == (21, 15) and tab.dtype == torch.uint8
    assert (geometry.TYPE_HYDROPHOBIC, geometry.TYPE_DONOR, geometry.TYPE_ACCEPTOR) == (1, 2, 4)
    assert len(t["res_index"]) == 21
    for res, r in t["res_index"].items():
        if r == 20:
            continue
        names = t["atom_names"][r][:15]
        carbons = {n for n in names if n.startswith("C")}
        got = {k: {n for s, n in enumerate(names) if n and int(tab[r, s]) & bit} for k, bit in (("h", 1), ("d", 2), ("a", 4))}
        assert carbons - got["h"] == {"CA", "C"} | POLAR_CARBONS.get(res, set()), res
        assert got["h"] <= carbons, res                                          # sulfur, nitrogen and oxygen are never hydrophobic
        assert got["d"] == (set() if res == "PRO" else {"N"}) | DONORS.get(res, set()), res
        assert got["a"] == {"O", "OXT"} | ACCEPTORS.get(res, set()), res
        assert not tab[r][[not n for n in names]].any(), res
    assert not int(tab[t["res_index"]["PRO"], 0]) & geometry.TYPE_DONOR          # proline's N has no hydrogen
    assert tab[20].tolist() == [2, 0, 0, 4] + [0] * 11                           # row 20: N (donor), CA, C, O (acceptor)
    his = t["res_index"]["HIS"]
    for nm in ("ND1", "NE2"):                                                    # the convention: both ring nitrogens, both ways
        assert int(tab[his, t["atom_names"][his].index(nm)]) == geometry.TYPE_DONOR | geometry.TYPE_ACCEPTOR


def test_radius_table():
    rad, t = geometry.xs_radius_table(), _tables()
    assert rad.shape == (21, 15) and rad.dtype == torch.float32
    assert geometry.XS_RADIUS == {"C": 1.9, "N": 1.8, "O": 1.7, "S": 2.0}
    for r in range(20):
        for s, n in enumerate(t["atom_names"][r][:15]):
            assert float(rad[r, s]) == (np.float32(geometry.XS_RADIUS[n[0]]) if n else 0.0), (r, s)
    assert (rad[:20, 14] == np.float32(1.7)).all()                               # OXT
    assert rad[20].tolist() == [np.float32(v) for v in (1.8, 1.9, 1.9, 1.7)] + [0.0] * 11
    cys = t["res_index"]["CYS"]
    assert float(rad[cys, t["atom_names"][cys].index("SG")]) == np.float32(2.0)


def test_oracle_states_the_same_tables():
    rad, typ = EO.tables()
    assert np.array_equal(typ, geometry.interface_type_table().numpy())
    assert np.array_equal(rad.astype(np.float32), geometry.xs_radius_table().numpy())
    assert geometry.ENERGY_TERMS == EO.TERMS == ("gauss1", "gauss2", "repulsion", "hydrophobic", "hbond")
    assert tuple(geometry.VINA_WEIGHTS) == EO.WEIGHTS == (-0.0356, -0.00516, 0.840, -0.0351, -0.587)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------

def test_struct_layout_agrees_with_the_header():
    cls = _capi.InterfaceEnergyArgs
    assert [(n, t) for n, t in cls._fields_] == header_fields("pf_interface_energy_args")
    last = cls._fields_[-1][0]
    assert getattr(cls, last).offset + 4 <= C.sizeof(cls) and C.sizeof(cls) % 8 == 0


def test_header_keeps_the_abi_version_and_the_order():
    text = open(HEADER).read()
    assert "#define PF_ABI_VERSION 65" in text and _capi.ABI_VERSION == 65
    assert text.index("} pf_contacts_args;") < text.index("} pf_interface_energy_args;")
    assert text.index("int pf_contacts_fwd(") < text.index("int pf_interface_energy_fwd(")
    assert "#define PF_INTERFACE_ENERGY_MAX_N 512" in text and geometry.ENERGY_MAX_N == 512
    assert "#define PF_INTERFACE_ENERGY_SLOTS 15" in text and geometry.ENERGY_SLOTS == 15


def test_library_exports_the_entry_point():
    assert "pf_interface_energy_fwd" in _capi.EXPORTED_SYMBOLS
    lib = _capi.load()
    assert lib.pf_abi_version() == _capi.ABI_VERSION == 65
    assert lib.pf_interface_energy_fwd(None, None) == -1
    assert lib.pf_interface_energy_fwd(C.byref(_capi.InterfaceEnergyArgs()), None) == -1


def test_wrapper_argument_checks():
    B, N = 2, 5
    pos, mask = torch.zeros(B, N, 15, 3), torch.ones(B, N, 15, dtype=torch.bool)
    aa, group = torch.zeros(B, N, dtype=torch.int64), torch.zeros(B, N, dtype=torch.bool)
    f = geometry.interface_energy
    for args in ((torch.zeros(B, N, 4, 3), mask, aa, group), (pos[0], mask, aa, group), (pos, mask[:, :, :14], aa, group),
                 (pos, mask, aa[:, :4], group), (pos, mask, aa, group[:1]), (pos, mask, aa, None)):
        with pytest.raises(ValueError):
            f(*args)
    with pytest.raises(ValueError):
        f(pos, mask, aa, group, query=torch.zeros(B, N + 1, dtype=torch.bool))
    for kw in (dict(cutoff=0.0), dict(cutoff=-8.0), dict(cutoff=float("nan")), dict(weights=(1.0, 2.0, 3.0, 4.0)),
               dict(weights=(1.0, 2.0, 3.0, 4.0, float("inf"))), dict(weights=(1.0, 2.0, 3.0, 4.0, float("nan"))), dict(weights=None),
               dict(weights="abcde")):
        with pytest.raises(ValueError):
            f(pos, mask, aa, group, **kw)
    big = 513                                               # above the kernel's bound
    with pytest.raises(ValueError):
        f(torch.zeros(1, big, 15, 3), torch.ones(1, big, 15, dtype=torch.bool), torch.zeros(1, big, dtype=torch.int64),
          torch.zeros(1, big, dtype=torch.bool))
    with pytest.raises(_capi.PepflowHipError):              # CPU tensors: no fall-back
        f(pos, mask, aa, group)
    with pytest.raises(ValueError):
        metrics.binding_energy({}, {}, backbone="atoms")


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------

def run_oracle(case, **kw):
    return EO.interface_energy(case["pos"][0], case["atom_mask"][0], case["aa"][0], case["group"][0], **kw)


@pytest.mark.parametrize("k", range(5))
def test_oracle_on_hand_computed_cases(k):
    name, case, (s0, s1), want = EC.hand_cases(np.float64)[k]
    o = run_oracle(case)
    rows = [(0, s0), (1, s1)]
    others = np.ones((2, 15), bool)
    for r in rows:
        others[r] = False
    assert not o["terms"][others].any() and not o["pairs"][others].any(), name
    if want is None:
        assert not o["terms"].any() and not o["pairs"].any() and o["energy_total"] == 0.0, name
        return
    for r in rows:
        assert np.abs(o["terms"][r] - want).max() <= 1e-12, (name, o["terms"][r], want)
        assert o["pairs"][r] == 1 and o["hbond_pairs"][r] == (want[4] > 0) and o["hydrophobic_pairs"][r] == (want[3] > 0), name
    assert np.abs(o["terms_total"] - want).max() <= 1e-12, name                 # one pair: half of its two rows
    assert abs(o["energy_total"] - float(np.dot(EO.WEIGHTS, want))) <= 1e-12, name
    assert abs(o["energy_residue"][0] - o["energy_total"]) <= 1e-12 and abs(o["energy_residue"][1] - o["energy_total"]) <= 1e-12


def test_hand_computed_values_are_the_issue_s():
    cases = {name: want for name, _, _, want in EC.hand_cases(np.float64)}
    cb, no, pro = cases["two CB at 4.3"], cases["N and O at 2.8"], cases["proline's N and O at 2.8"]
    assert abs(cb[0] - np.exp(-1.0)) < 1e-15 and cb[2:] == [0.0, 1.0, 0.0]
    assert no[2:] == [0.49, 0.0, 1.0] and pro[2:] == [0.49, 0.0, 0.0]
    assert cases["N and O in one group"] is None and cases["N and O at the cutoff"] is None
    # just inside the cutoff the pair is evaluated
    _, case, _, _ = EC.hand_cases(np.float64)[4]
    case["pos"][0, 1, EC.O_SLOT, 0] = 8.0 - 1e-9
    o = run_oracle(case)
    assert o["pairs"][0, EC.N_SLOT] == 1 and o["near_cutoff"].sum() == 0
    assert run_oracle(case, bound=1e-6)["near_cutoff"].sum() == 2
    assert abs(run_oracle(case)["margin_cutoff"][0, EC.N_SLOT] - 1e-9) < 1e-12


def test_oracle_margins_and_derivatives():
    _, case, (s0, s1), want = EC.hand_cases(np.float64)[1]                      # d = -0.7
    o = run_oracle(case, bound=1e-6)
    assert abs(o["margin_hb_lo"][0, s0]) < 1e-12 and abs(o["margin_hb_hi"][0, s0] - 0.7) < 1e-12
    assert np.isinf(o["margin_hp_lo"][0, s0]) and abs(o["margin_cutoff"][0, s0] - 5.2) < 1e-12
    assert o["near_hbond"].sum() == 0
    d = -0.7
    g = [8 * 0.7 * want[0], abs((d - 3) / 2) * want[1], 1.4, 0.0, 1 / 0.7]
    assert np.abs(o["dterms"][0, s0][:4] - g[:4]).max() <= 1e-12
    assert o["dterms"][0, s0, 4] in (0.0, 1 / 0.7)          # d sits on the kink of the hbond ramp: either side's slope
    g[4] = o["dterms"][0, s0, 4]
    assert abs(o["abs_w"][0, s0] - np.abs(np.array(EO.WEIGHTS) * want).sum()) <= 1e-12
    assert abs(o["dabs_w"][0, s0] - np.abs(np.array(EO.WEIGHTS) * g).sum()) <= 1e-12
    # a finite difference of the terms agrees with the stated derivatives away from the kinks
    for d0 in (-0.3, 0.2, 0.9, 2.0, 4.0):
        t, g = EO.pair_terms(np.array([d0]), np.array([True]), np.array([True]))
        t1, _ = EO.pair_terms(np.array([d0 + 1e-6]), np.array([True]), np.array([True]))
        assert np.abs(np.abs(t1 - t) / 1e-6 - g).max() <= 1e-4, d0


def test_oracle_symmetry_and_options():
    case = EC.make_case(3101, 3, 40, 14.0)
    for o, group in zip(EC.oracle(case), case["group"]):
        a, b = o["terms_residue"][group].sum(0), o["terms_residue"][~group].sum(0)
        assert np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(a).max())
        assert np.abs(o["terms_total"] - a).max() <= 1e-9 * max(1.0, np.abs(a).max())
        assert o["pairs"][group].sum() == o["pairs"][~group].sum()
        assert o["hbond_pairs"][group].sum() == o["hbond_pairs"][~group].sum()
    assert o["pairs"].sum() == 0 and o["energy_total"] == 0.0                   # structure 2 has one group only
    full = EC.oracle(case)[1]
    assert full["pairs"].sum() > 0 and full["hbond_pairs"].sum() > 0 and full["hydrophobic_pairs"].sum() > 0
    # a query: the rows it names are unchanged, the participating atoms it leaves out are -1, and the totals are the plain sums
    query = case["query"]
    q = EC.oracle(case, query=query)[2 if query[2].any() else 1]
    b = 2 if query[2].any() else 1
    ref = EC.oracle(case)[b]
    assert np.array_equal(q["terms"][query[b]], ref["terms"][query[b]])
    assert (q["pairs"][~query[b]][ref["part"][~query[b]]] == -1).all() and not q["terms"][~query[b]].any()
    assert np.abs(q["terms_total"] - ref["terms_residue"][query[b]].sum(0)).max() <= 1e-9


def test_oracle_against_a_dense_form():
    """one structure of 40 residues with every atom pair written out"""
    case = EC.make_case(2102, 2, 40, 14.0)
    o = EC.oracle(case)[1]
    rad, typ = EO.tables()
    aa = case["aa"][1]
    row = np.where((aa < 0) | (aa > 20), 20, aa)
    R, T = rad[row].reshape(-1), typ[row].reshape(-1)
    part = (case["atom_mask"][1] & (rad[row] > 0)).reshape(-1)
    X, G = case["pos"][1].astype(np.float64).reshape(-1, 3), np.repeat(case["group"][1], 15)
    r = np.sqrt(((X[:, None] - X[None]) ** 2).sum(-1))
    m = part[:, None] & part[None] & (G[:, None] != G[None]) & (r < 8.0)
    d = r - R[:, None] - R[None]
    both = lambda bit: ((T & bit) != 0)[:, None] & ((T & bit) != 0)[None]  # noqa: E731
    da = ((T & 2) != 0)[:, None] & ((T & 4) != 0)[None]
    hb = (da | da.T) & m
    dense = [np.exp(-(d / 0.5) ** 2) * m, np.exp(-((d - 3) / 2) ** 2) * m, np.where(d < 0, d * d, 0) * m,
             np.clip(1.5 - d, 0, 1) * (both(1) & m), np.clip(-d / 0.7, 0, 1) * hb]
    assert m.sum() > 100 and hb.sum() > 0 and (both(1) & m).sum() > 0
    assert np.array_equal(o["pairs"].reshape(-1), m.sum(1))
    for k in range(5):
        assert np.abs(o["terms"].reshape(-1, 5)[:, k] - dense[k].sum(1)).max() <= 1e-10, k
    assert np.array_equal(o["hbond_pairs"].reshape(-1), (dense[4] > 0).sum(1))
    assert np.array_equal(o["hydrophobic_pairs"].reshape(-1), (dense[3] > 0).sum(1))
    assert abs(o["energy_total"] - 0.5 * sum(w * t.sum() for w, t in zip(EO.WEIGHTS, dense))) <= 1e-9
