"""CPU checks of lDDT, interface contacts and DockQ: the numpy float64 oracle (lddt_oracle.py) against the fixture recorded from the
reference's OpenFold functions (golden F15), hand-checked cases of the oracle, the ctypes struct layouts against the header, the
exported symbols, and the wrappers' argument checks.

The allowance against the reference (derived, not tuned): the reference decides every pair in fp32, so a pair whose float64 margin is
below 8 * 2^-23 * max|coord| may fall on the other side: a row with `scored` pairs may move by 0.25 (near_kept + 4 near_scored) /
scored; on top of that its two fp32 sums are exact (multiples of 0.25 below 2^24) and the reciprocal and the product round once each:
4 * 2^-24 relative."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import lddt_oracle as LO  # noqa: E402
from pepflowww_amd import _capi, geometry, metrics  # noqa: E402

ULP8 = 8.0 * 2.0 ** -23
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pepflow_hip.h")


@pytest.fixture(scope="module")
def gold(golden_dir):
    path = os.path.join(golden_dir, "f15_lddt.npz")
    assert os.path.getsize(path) < 200 * 1024
    return dict(np.load(path))


def reference_expression(kept, scored):
    return (1e-10 + 0.25 * kept) / (1e-10 + scored)


def allowance(o, tag=""):
    near = 0.25 * (o["near_kept" + tag] + 4 * o["near_scored" + tag])
    return near / np.maximum(o["scored" + tag], 1) + 4 * 2.0 ** -24


def test_oracle_matches_the_reference_fixture(gold):
    S, N = gold["aa"].shape
    y = (gold["pos"][0], gold["atom_mask"][0], gold["aa"][0])
    for s in range(S):
        x = (gold["pos"][s], gold["atom_mask"][s], gold["aa"][s])
        bound = ULP8 * float(max(np.abs(x[0]).max(), np.abs(y[0]).max()))
        o = LO.lddt(*x, *y, 0x3FFF, float(gold["cutoff"]), group=gold["group"], bound=bound)
        for k in ("scored", "kept", "scored_cross", "kept_cross", "scored_atom", "kept_atom"):
            assert np.array_equal(o[k], gold[k][s]), (s, k)
        # per atom (per_residue=True on the flattened atoms): the near counts are per row residue, which bounds each of its atoms
        near = 0.25 * (o["near_kept"] + 4 * o["near_scored"])[:, None]
        mine = reference_expression(o["kept_atom"], o["scored_atom"])
        err = np.abs(mine - gold["ref_lddt_atom"][s].reshape(N, 14))
        assert (err <= near / np.maximum(o["scored_atom"], 1) + 4 * 2.0 ** -24).all(), (s, float(err.max()))
        # the whole structure (per_residue=False)
        tot = reference_expression(o["kept"].sum(), o["scored"].sum())
        slack = 0.25 * (o["near_kept"].sum() + 4 * o["near_scored"].sum()) / max(o["scored"].sum(), 1) + 4 * 2.0 ** -24
        assert abs(tot - float(gold["ref_lddt"][s])) <= slack, s
        # a masked atom's row is (eps + 0) / (eps + 0) = 1 in the reference, NaN here
        off = ~gold["compared"][s]
        assert (gold["ref_lddt_atom"][s].reshape(N, 14)[off] == 1.0).all() and (o["scored_atom"][off] == 0).all()
        assert np.isnan(LO.score(o["kept_atom"], o["scored_atom"])[off]).all()
        # lddt_ca
        c = LO.lddt(*x, *y, 0x2, float(gold["cutoff"]), group=gold["group"], bound=bound)
        assert np.array_equal(c["scored"], gold["scored_ca"][s]) and np.array_equal(c["kept"], gold["kept_ca"][s])
        err = np.abs(reference_expression(c["kept"], c["scored"]) - gold["ref_lddt_ca_residue"][s])
        assert (err <= allowance(c)).all(), (s, float(err.max()))
        tot = reference_expression(c["kept"].sum(), c["scored"].sum())
        slack = 0.25 * (c["near_kept"].sum() + 4 * c["near_scored"].sum()) / max(c["scored"].sum(), 1) + 4 * 2.0 ** -24
        assert abs(tot - float(gold["ref_lddt_ca"][s])) <= slack, s
    assert float(gold["ref_lddt"][0]) > 0.9999 and 0.2 < float(gold["ref_lddt"][2]) < 0.95


def test_oracle_options_against_a_dense_form(gold):
    """query, group, exclude_same_residue and the slot masks against the [N*14, N*14] matrices written out (52 residues)"""
    rng = np.random.default_rng(150)
    N = 52
    X, Y = gold["pos"][2].astype(np.float64).reshape(N * 14, 3), gold["pos"][0].astype(np.float64).reshape(N * 14, 3)
    res = np.repeat(np.arange(N), 14)
    d_x = np.sqrt(1e-10 + ((X[:, None] - X[None]) ** 2).sum(-1))
    d_y = np.sqrt(1e-10 + ((Y[:, None] - Y[None]) ** 2).sum(-1))
    k4 = (np.abs(d_y - d_x)[:, :, None] < LO.THRESHOLDS).sum(-1)
    for slots, excl in ((0x3FFF, False), (0x3FFF, True), (0xF, False), (0x2, True), (0x35, False)):
        query, group = rng.random(N) < 0.3, rng.random(N) < 0.4
        cmp_ = LO.compared_atoms(gold["atom_mask"][2], gold["aa"][2], gold["atom_mask"][0], gold["aa"][0], slots).reshape(-1)
        o = LO.lddt(gold["pos"][2], gold["atom_mask"][2], gold["aa"][2], gold["pos"][0], gold["atom_mask"][0], gold["aa"][0], slots, 15.0,
                    excl, group, query)
        m = (cmp_ & query[res])[:, None] & cmp_[None, :] & (d_y < 15.0) & ~np.eye(N * 14, dtype=bool)
        if excl:
            m &= res[:, None] != res[None, :]
        cross = group[res][:, None] != group[res][None, :]
        assert np.array_equal(o["scored_atom"].reshape(-1), m.sum(1)) and np.array_equal(o["kept_atom"].reshape(-1), (m * k4).sum(1))
        assert np.array_equal(o["scored_cross"], (m & cross).sum(1).reshape(N, 14).sum(1))
        assert np.array_equal(o["kept_cross"], ((m & cross) * k4).sum(1).reshape(N, 14).sum(1))
        assert not o["scored"][~query].any()


def two_atoms(d_x, d_y):
    """residues 0 and 1 of different groups with a CA each, d apart in each structure"""
    pos = np.zeros((2, 2, 14, 3), np.float32)
    pos[0, 1, 1, 0], pos[1, 1, 1, 0] = d_x, d_y
    mask = np.zeros((2, 14), bool)
    mask[:, 1] = True
    return pos[0], pos[1], mask, np.array([0, 1])


def test_two_atoms_around_the_contact_cutoff():
    x, y, mask, group = two_atoms(4.9, 5.1)
    c = LO.contacts(x, mask, y, mask, group, bound=0.15)
    assert c["contacts_x"].tolist() == [1, 1] and c["contacts_y"].tolist() == [0, 0] and c["contacts_shared"].tolist() == [0, 0]
    assert c["interface_x"].all() and c["interface_y"].all()
    assert np.allclose(c["min_dist_x"], 4.9, atol=1e-6) and np.allclose(c["min_dist_y"], 5.1, atol=1e-6)
    assert c["near_contact_x"].tolist() == [1, 1] and c["near_contact_y"].tolist() == [1, 1] and not c["near_interface_x"].any()
    d = LO.dockq(x, mask, y, mask, group)
    assert np.isnan(d["fnat"]) and d["fnonnat"] == 1.0 and d["n_native_contacts"] == 0 and d["n_sample_contacts"] == 1
    # the same group on both: nothing counts
    c = LO.contacts(x, mask, y, mask, np.array([1, 1]))
    assert not c["contacts_x"].any() and np.isinf(c["min_dist_x"]).all() and not c["interface_x"].any()
    # lDDT of the pair: |5.1 - 4.9| = 0.2 keeps all four thresholds; 6.2 against 5.1 keeps 2 and 4
    same = np.zeros(2, np.int64)
    o = LO.lddt(x, mask, same, y, mask, same, 0x2)
    assert o["scored"].tolist() == [1, 1] and o["kept"].tolist() == [4, 4]
    x2 = x.copy()
    x2[1, 1, 0] = 6.2
    o = LO.lddt(x2, mask, same, y, mask, same, 0x2, group=group)
    assert o["kept"].tolist() == [2, 2] and o["kept_cross"].tolist() == [2, 2]
    assert LO.lddt(x, mask, same, y, mask, same, 0x2, cutoff=5.0)["scored"].tolist() == [0, 0]      # 5.1 in y is outside


def test_identical_structures(gold):
    pos, mask, aa, group = gold["pos"][0], gold["atom_mask"][0], gold["aa"][0], gold["group"]
    o = LO.lddt(pos, mask, aa, pos, mask, aa, group=group)
    assert np.array_equal(o["kept"], 4 * o["scored"]) and o["scored"].sum() > 0 and o["scored_cross"].sum() > 0
    c = LO.contacts(pos, mask, pos, mask, group)
    assert np.array_equal(c["contacts_x"], c["contacts_y"]) and np.array_equal(c["contacts_x"], c["contacts_shared"])
    assert c["contacts_x"][group].sum() == c["contacts_x"][~group].sum() > 0            # each residue pair shows in both rows
    d = LO.dockq(pos, mask, pos, mask, group)
    assert d["fnat"] == 1.0 and d["fnonnat"] == 0.0 and d["irmsd"] < 1e-6 and d["lrmsd"] < 1e-6 and abs(d["dockq"] - 1.0) < 1e-9
    # the ligand moved by 3 A with the receptor fixed: LRMSD 3
    moved = pos.copy()
    moved[group] += np.array([0.0, 3.0, 0.0], np.float32)
    assert abs(LO.dockq(moved, mask, pos, mask, group)["lrmsd"] - 3.0) < 1e-5


def test_dockq_formula():
    for f in (LO.dockq_score, geometry.dockq_score):
        assert f(1.0, 0.0, 0.0) == 1.0
        assert abs(f(0.0, 1.5, 8.5) - 1.0 / 3.0) < 1e-15
    assert geometry.DOCKQ_CLASSES == ("incorrect", "acceptable", "medium", "high")
    assert geometry.SLOT_MASKS == LO.SLOT_MASKS


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

CTYPES = {"float": C.c_float, "int": C.c_int}


def header_fields(struct):
    """[(name, ctype)] of `typedef struct { ... } struct;` in the header, in order"""
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} " + struct + ";", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        if "*" in decl:
            fields.append((decl.split("*")[-1].strip(), C.c_void_p))
        else:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), CTYPES[ctype]) for n in names.split(",")]
    return fields


@pytest.mark.parametrize("struct,cls", [("pf_lddt_args", _capi.LddtArgs), ("pf_contacts_args", _capi.ContactsArgs)])
def test_struct_layout_agrees_with_the_header(struct, cls):
    assert [(n, t) for n, t in cls._fields_] == header_fields(struct)
    last = cls._fields_[-1][0]
    assert getattr(cls, last).offset + 4 <= C.sizeof(cls) and C.sizeof(cls) % 8 == 0


def test_header_keeps_the_abi_version_and_the_order():
    text = open(HEADER).read()
    assert "#define PF_ABI_VERSION 65" in text and _capi.ABI_VERSION == 65
    assert text.index("} pf_sidechain_compare_args;") < text.index("} pf_lddt_args;") < text.index("} pf_contacts_args;")
    assert "#define PF_LDDT_MAX_N 512" in text and geometry.LDDT_MAX_N == 512


def test_library_exports_the_entry_points():
    assert "pf_lddt_fwd" in _capi.EXPORTED_SYMBOLS and "pf_contacts_fwd" in _capi.EXPORTED_SYMBOLS
    lib = _capi.load()
    assert lib.pf_abi_version() == _capi.ABI_VERSION
    assert lib.pf_lddt_fwd(None, None) == -1 and lib.pf_contacts_fwd(None, None) == -1
    assert lib.pf_lddt_fwd(C.byref(_capi.LddtArgs()), None) == -1
    assert lib.pf_contacts_fwd(C.byref(_capi.ContactsArgs()), None) == -1


def test_wrapper_argument_checks():
    def side(B=2, N=5, A=14):
        return dict(pos=torch.zeros(B, N, A, 3), atom_mask=torch.ones(B, N, A, dtype=torch.bool), aa=torch.zeros(B, N, dtype=torch.int64))
    x, pairs, group = side(), torch.tensor([[0, 0], [1, 1]]), torch.zeros(2, 5, dtype=torch.bool)
    for bad in (dict(x, pos=torch.zeros(2, 5, 4, 3)), dict(x, atom_mask=x["atom_mask"][:, :, :4]), dict(x, aa=x["aa"][:, :4]),
                {"pos": x["pos"]}, side(N=6)):              # shapes, a missing key, another number of residues than the other side
        with pytest.raises(ValueError):
            geometry.lddt(bad, x, pairs)
        with pytest.raises(ValueError):
            geometry.interface_contacts(x, bad, pairs, group)
    big = side(N=513)                                       # above the kernels' bound
    with pytest.raises(ValueError):
        geometry.lddt(big, big, pairs)
    with pytest.raises(ValueError):
        geometry.interface_contacts(big, big, pairs, torch.zeros(2, 513, dtype=torch.bool))
    with pytest.raises(ValueError):
        geometry.lddt(x, x, torch.tensor([0, 1]))
    with pytest.raises(ValueError):
        geometry.lddt(x, x, pairs, group=torch.zeros(2, 4, dtype=torch.bool))
    with pytest.raises(ValueError):
        geometry.lddt(x, x, pairs, query=torch.zeros(3, 5, dtype=torch.bool))
    for kw in (dict(slots="sidechain"), dict(slots=0), dict(cutoff=0.0), dict(cutoff=float("nan"))):
        with pytest.raises(ValueError):
            geometry.lddt(x, x, pairs, **kw)
    with pytest.raises(ValueError):
        geometry.interface_contacts(x, x, pairs, None)
    with pytest.raises(ValueError):
        geometry.dockq(x, x, pairs, None)
    with pytest.raises(ValueError):
        geometry.interface_contacts(x, x, pairs, group, contact_cutoff=-1.0)
    with pytest.raises(_capi.PepflowHipError):              # CPU tensors: no fall-back
        geometry.lddt(x, x, pairs)
    with pytest.raises(_capi.PepflowHipError):
        geometry.interface_contacts(x, x, pairs, group)
    with pytest.raises(ValueError):
        metrics.local_accuracy({}, {}, backbone="atoms")
    with pytest.raises(ValueError):
        metrics.docking_quality({}, {}, backbone="atoms")
