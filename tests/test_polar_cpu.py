"""CPU checks of the hydrogen bonds and salt bridges (heavy-atom criteria written from the publications -- Baker & Hubbard 1984,
McDonald & Thornton 1994, Barlow & Thornton 1983 -- and not checked against HBPLUS, PLIP or Rosetta): the numpy float64 oracle
(polar_oracle.py) on the cases with known answers, its invariance and symmetry; the charge and antecedent tables against the oracle's
own statement of them; the ctypes struct layout against the header, the exported symbol and the entry point's argument checks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import dssp_build as DB  # noqa: E402
import dssp_oracle as DO  # noqa: E402
import polar_cases as PC  # noqa: E402
import polar_oracle as PO  # noqa: E402
from test_lddt_cpu import HEADER, header_fields  # noqa: E402
from pepflowww_amd import _capi, build, geometry, metrics  # noqa: E402
from pepflowww_amd.preprocess import _tables  # noqa: E402


# ---- the oracle on cases with known answers ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def known():
    return PC.known_cases()


@pytest.mark.parametrize("k", range(5))
def test_oracle_gives_the_known_counts(known, k):
    name, case, criteria, want, key = known[k]
    o = PC.oracle(case, **criteria)[0]
    assert o["near_pairs"] == 0 and o[key] == want, (name, o[key], want)
    assert o["n_salt_bridges"] == 0, name
    bonds = PC.bond_offsets(o)
    assert all(abs(a - d) != 1 or case["chain"][0][a] != case["chain"][0][d] for d, a in bonds), name   # no N(i+1)...O(i)
    steps = sorted({d - a for d, a in bonds})
    if name == "alpha helix":
        assert steps == [3, 4] and sum(d - a == 4 for d, a in bonds) == 8 and sum(d - a == 3 for d, a in bonds) == 9
    elif name == "alpha helix, donor angle 100":
        assert steps == [4]
    elif name == "3-10 helix":
        assert steps == [3]
    else:
        assert o["n_hbonds"] == want, name              # every bond of a strand pair is between the strands


@pytest.mark.parametrize("k", range(8))
def test_oracle_on_hand_cases(k):
    name, case, criteria, hb, sb = PC.hand_cases()[k]
    o = PC.oracle(case, **criteria)[0]
    assert o["near_pairs"] == 0, name
    for pairs, key in ((hb, "hbond"), (sb, "salt")):
        rows, n = PC.expected_rows(pairs)
        assert o["n_hbonds" if key == "hbond" else "n_salt_bridges"] == n, (name, key)
        for i in range(2):
            for s in range(15):
                assert o[key + "_list"][i][s] == rows.get((i, s), []), (name, key, i, s)


def test_oracle_keeps_every_partner_of_an_overfull_row():
    case = PC.overflow_case()
    o = PC.oracle(case)[0]
    s = PC.slot("ALA", "O")
    assert o["hbonds"][0, s] == 6 and o["hbond_list"][0][s] == [15 * r for r in range(1, 7)]
    assert PO.partner_array(o["hbond_list"])[0, s].tolist() == [15, 30, 45, 60]
    assert o["n_hbonds"] == 6 and o["n_hbonds_cross"] == 6


def test_oracle_is_invariant_under_rigid_motion_and_symmetric():
    case = PC.make_case(4052, 3, 52)
    moved = dict(case, pos=(case["pos"].astype(np.float64) @ DB.rotation(np.array([0.3, -1.1, 0.7])).T + [11.0, -7.0, 3.0]))
    a, b = PC.oracle(case), PC.oracle(moved)
    assert sum(o["n_hbonds"] for o in a) > 0 and sum(o["n_salt_bridges"] for o in a) > 0
    for x, y in zip(a, b):
        assert x["near_pairs"] == y["near_pairs"] == 0
        for key in ("hbonds", "salt", "hbonds_cross", "salt_cross"):
            assert np.array_equal(x[key], y[key]), key
        assert x["hbond_list"] == y["hbond_list"] and x["salt_list"] == y["salt_list"]
        for key in ("hbond_list", "salt_list"):                                 # every bond is in both of its rows
            for i, row in enumerate(x[key]):
                for s, partners in enumerate(row):
                    for flat in partners:
                        assert i * 15 + s in x[key][flat // 15][flat % 15], (key, i, s, flat)
    g = case["group"][1]
    assert a[1]["hbonds_cross"][g].sum() == a[1]["hbonds_cross"][~g].sum() == a[1]["n_hbonds_cross"]
    assert a[2]["n_hbonds_cross"] == 0 and a[2]["n_salt_bridges_cross"] == 0    # structure 2 has one group only


def test_oracle_query_restricts_the_rows_only():
    case = PC.make_case(4052, 3, 52)
    full, q = PC.oracle(case), PC.oracle(case, query=case["query"])
    for b in range(3):
        rows = case["query"][b]
        assert np.array_equal(q[b]["hbonds"][rows], full[b]["hbonds"][rows])
        assert (q[b]["hbonds"][~rows][full[b]["part"][~rows]] == -1).all()
        assert q[b]["n_hbonds"] == full[b]["hbonds_residue"][rows].sum()


@pytest.mark.parametrize("k", (0, 2, 3, 4))
def test_dssp_bonds_are_polar_bonds(known, k):
    """two definitions of a backbone hydrogen bond, on structures where both must agree: every donor -> acceptor pair of the DSSP
    oracle with energy < -0.5 is a bond here at default criteria"""
    name, case, _, _, _ = known[k]
    n = case["pos"].shape[1]
    d = DO.hbonds(case["pos"][0].astype(np.float64), np.ones(n, bool), case["chain"][0])
    o = PC.oracle(case)[0]
    pairs = set(PC.bond_offsets(o))
    assert d["bonds"].sum() > 0, name
    for donor, acc in zip(*np.nonzero(d["bonds"])):
        assert (int(donor), int(acc)) in pairs, (name, donor, acc)


# ---- the tables ---------------------------------------------------------------------------------------------------------------------

def test_tables_agree_with_the_oracle_s_lists():
    types, ante, names = geometry.interface_type_table(), geometry.antecedent_table(), PO.atom_names()
    assert ante.shape == (21, 15, 2) and ante.dtype == torch.int8
    don, acc, chg, o_ante = PO.tables()
    assert np.array_equal(don, (types.numpy() & geometry.TYPE_DONOR) != 0)
    assert np.array_equal(acc, (types.numpy() & geometry.TYPE_ACCEPTOR) != 0)
    bonds = geometry.bond_table()
    for his in (False, True):
        charge = geometry.charge_table(his)
        assert charge.shape == (21, 15) and charge.dtype == torch.uint8
        assert np.array_equal(PO.tables(his)[2], charge.numpy())
        for t in range(21):
            for s in range(15):
                if int(charge[t, s]):                                           # charge classes sit only on N (1) or O (2) slots
                    assert names[t][s][0] == {1: "N", 2: "O"}[int(charge[t, s])], (t, s)
    n_charged = int((geometry.charge_table() != 0).sum())
    assert n_charged == 1 + 3 + 2 + 2 and int((geometry.charge_table(True) != 0).sum()) == n_charged + 2
    for t in range(21):
        for s in range(15):
            got = [int(v) for v in ante[t, s] if v >= 0]
            assert (len(got) > 0) == bool(names[t][s]), (t, s)                  # the type has the slot <=> it has an antecedent
            assert got == sorted(got) and all(bool(bonds[t, s, v]) for v in got), (t, s)
            if don[t, s] or acc[t, s] or chg[t, s]:
                assert int(bonds[t, s].sum()) >= 1 and got == sorted(o_ante[t][s]), (t, s, got, o_ante[t][s])
                assert int(bonds[t, s].sum()) <= 2 or names[t][s] == "N", (t, s)
    assert ante[20].tolist() == [[1, -1], [0, 2], [1, 3], [2, -1]] + [[-1, -1]] * 11     # row 20: N-CA, CA-C, C-O
    assert not geometry.charge_table(True)[20].any() and types[20].tolist() == [2, 0, 0, 4] + [0] * 11


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------

def test_struct_layout_agrees_with_the_header():
    cls = _capi.PolarArgs
    assert [(n, t) for n, t in cls._fields_] == header_fields("pf_polar_args")
    last = cls._fields_[-1][0]
    assert getattr(cls, last).offset + 4 <= C.sizeof(cls) and C.sizeof(cls) % 8 == 0


def test_header_keeps_the_abi_version_and_names_the_bounds():
    text = open(HEADER).read()
    assert "#define PF_ABI_VERSION 65" in text and _capi.ABI_VERSION == 65
    assert "#define PF_POLAR_MAX_N 512" in text and geometry.POLAR_MAX_N == 512
    assert "#define PF_POLAR_MAX_PARTNERS 4" in text and geometry.POLAR_MAX_PARTNERS == PO.K == 4
    assert text.index("int pf_sidechain_compare_fwd(") < text.index("int pf_polar_fwd(") < text.index("} pf_lddt_args;")
    assert "polar.hip" in build.SOURCES


def _host_args(B=1, N=4, A=15):
    """a fully bound argument struct over host buffers: the entry point must refuse before it launches anything"""
    keep = {k: np.zeros(n, dt) for k, n, dt in (
        ("pos", B * N * A * 3, np.float32), ("atom_mask", B * N * A, np.uint8), ("aa", B * N, np.int64),
        ("residue_index", B * N, np.int64), ("group", B * N, np.uint8), ("types", 21 * 15, np.uint8), ("charge", 21 * 15, np.uint8),
        ("antecedents", 21 * 15 * 2, np.int8), ("work", B * N * 4, np.float32), ("hbonds_atom", B * N * 15, np.int32),
        ("salt_atom", B * N * 15, np.int32), ("hbonds_atom_cross", B * N * 15, np.int32), ("salt_atom_cross", B * N * 15, np.int32),
        ("hbond_partner", B * N * 60, np.int32), ("salt_partner", B * N * 60, np.int32), ("hbonds_residue", B * N, np.int32),
        ("salt_residue", B * N, np.int32), ("hbonds_residue_cross", B * N, np.int32), ("salt_residue_cross", B * N, np.int32))}
    a = _capi.PolarArgs()
    for k, v in keep.items():
        setattr(a, k, v.ctypes.data)
    a.B, a.N, a.n_atoms, a.d_max, a.cos_acc, a.cos_don, a.salt_max = B, N, A, 3.5, 0.0, 0.0, 4.0
    return a, keep


def test_entry_point_refuses_bad_arguments_before_any_launch():
    assert "pf_polar_fwd" in _capi.EXPORTED_SYMBOLS
    lib = _capi.load()
    assert lib.pf_abi_version() == _capi.ABI_VERSION == 65
    assert lib.pf_polar_fwd(None, None) == -1
    assert lib.pf_polar_fwd(C.byref(_capi.PolarArgs()), None) == -1
    for field in ("pos", "atom_mask", "aa", "residue_index", "types", "charge", "antecedents", "work", "hbonds_atom", "salt_atom",
                  "hbond_partner", "salt_partner", "hbonds_residue", "salt_residue", "group", "hbonds_atom_cross",
                  "salt_residue_cross"):
        a, keep = _host_args()
        setattr(a, field, None)
        assert lib.pf_polar_fwd(C.byref(a), None) == -1, field
    inf, nan = float("inf"), float("nan")
    for field, value in (("N", 513), ("N", -1), ("B", -1), ("n_atoms", 13), ("d_max", 0.0), ("d_max", -3.5), ("d_max", inf),
                         ("d_max", nan), ("salt_max", 0.0), ("salt_max", nan), ("salt_max", inf), ("cos_acc", 1.5), ("cos_acc", nan),
                         ("cos_don", -1.5), ("cos_don", inf)):
        a, keep = _host_args()
        setattr(a, field, value)
        assert lib.pf_polar_fwd(C.byref(a), None) == -1, (field, value)
    a, keep = _host_args()
    a.B = 0                                                 # an empty batch is fine and launches nothing
    assert lib.pf_polar_fwd(C.byref(a), None) == 0


def test_wrapper_argument_checks():
    B, N = 2, 5
    pos, mask = torch.zeros(B, N, 15, 3), torch.ones(B, N, 15, dtype=torch.bool)
    aa, idx = torch.zeros(B, N, dtype=torch.int64), torch.arange(N).repeat(B, 1)
    f = geometry.polar_interactions
    for args in ((torch.zeros(B, N, 4, 3), mask, aa, idx), (pos[0], mask, aa, idx), (pos, mask[:, :, :14], aa, idx),
                 (pos, mask, aa[:, :4], idx), (pos, mask, aa, idx[:1]), (pos, mask, aa, None)):
        with pytest.raises(ValueError):
            f(*args)
    for kw in (dict(d_max=0.0), dict(d_max=float("nan")), dict(salt_max=-4.0), dict(acc_angle_min=181.0), dict(don_angle_min=-1.0),
               dict(acc_angle_min=float("nan")), dict(don_angle_min=None), dict(group=torch.zeros(B, N + 1, dtype=torch.bool)),
               dict(query=torch.zeros(B + 1, N, dtype=torch.bool))):
        with pytest.raises(ValueError):
            f(pos, mask, aa, idx, **kw)
    big = 513                                               # above the kernel's bound
    with pytest.raises(ValueError):
        f(torch.zeros(1, big, 15, 3), torch.ones(1, big, 15, dtype=torch.bool), torch.zeros(1, big, dtype=torch.int64),
          torch.arange(big)[None])
    with pytest.raises(_capi.PepflowHipError):              # CPU tensors: no fall-back
        f(pos, mask, aa, idx)
    with pytest.raises(ValueError):
        metrics.polar_satisfaction({}, {}, backbone="atoms")
    with pytest.raises(ValueError):
        metrics.polar_satisfaction({}, {}, max_sasa=-1.0)
    assert len(_tables()["res_index"]) == 21
