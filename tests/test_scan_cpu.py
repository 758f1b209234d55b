"""CPU checks of the point-mutation scan (pf_mutation_scan_fwd; the packer's self energy of every candidate type on an unmoved
environment; not FoldX, not Rosetta): the scan oracle against pack_oracle's own E_self on mutated inputs, the oracle in float32 against
the rule, the recorded seeds against the cap, the ctypes struct layout against the header, the entry points' argument checks and work
sizes, and the wrappers' argument checks and `candidates` normalisation.  The comparison rule is pack_cases.bound (scan_cases.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import pack_cases as PC  # noqa: E402
import pack_oracle as PO  # noqa: E402
import scan_cases as SC  # noqa: E402
import scan_oracle as SO  # noqa: E402
from test_lddt_cpu import HEADER, header_fields  # noqa: E402
from pepflowww_amd import _capi, build, geometry, metrics  # noqa: E402


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------

def _scan(case, b, **kw):
    return SO.Scan(case["pos"][b], case["atom_mask"][b], case["aa"][b], case["residue_index"][b], case["positions"][b], **kw)


def test_oracle_equals_the_packing_oracle_on_mutated_inputs():
    """E[q,t,.] is pack_oracle's own E_self on the input with aa[q] := t and q alone movable: the same numbers, to the last bit of
    float64 but for the order of two additions"""
    case = SC.make_case(17)
    idx = PO.res_index()
    b = 1                                                   # every residue is a position
    scan = _scan(case, b)
    qs = np.flatnonzero(scan.scanned)
    pairs = [(int(qs[0]), idx["ARG"]), (int(qs[1]), idx["PRO"]), (int(qs[2]), idx["CYS"]), (int(qs[3]), idx["TRP"]),
             (int(qs[4]), idx["ALA"]), (int(qs[-1]), idx["GLN"]), (int(qs[-2]), int(case["aa"][b, qs[-2]]))]
    for q, t in pairs:
        aa = case["aa"][b].copy()
        aa[q] = t
        o = PO.Structure(case["pos"][b], case["atom_mask"][b], aa, case["residue_index"][b], np.arange(len(aa)) == q)
        assert list(o.plist) == [q]
        want, got = o.self_[0], scan.res[q, t]
        assert len(want["E"]) == len(got["E"]) == PO.rotamer_table()[1][t]
        np.testing.assert_allclose(got["E"], want["E"], rtol=0, atol=1e-12 * max(1.0, float(np.abs(want["absw"]).max())))
        assert np.array_equal(got["n"], want["n"]) and np.array_equal(got["pairs"], want["pairs"])
    # and the environment is the input as given: the other scanned residues keep their side chains
    assert scan.env_ok[qs[1], 5:14].any()


def test_oracle_fill_candidates_and_group():
    case = SC.make_case(15)
    b = 3
    cand = np.zeros((15, 20), bool)
    cand[:, PO.res_index()["ALA"]] = True
    scan = _scan(case, b, candidates=cand, group=case["group"][b])
    e, rot, cnt = scan.energy()
    qs = np.flatnonzero(scan.scanned)
    assert len(qs) > 0 and len(qs) < 15
    for q in range(15):
        wt, ala = int(case["aa"][b, q]), PO.res_index()["ALA"]
        want = {wt, ala} if scan.scanned[q] else set()
        assert set(np.flatnonzero(rot[q] >= 0)) == want and set(np.flatnonzero(np.isfinite(e[q]))) == want
        if scan.scanned[q]:
            assert e[q, ala] == 0.0 and cnt[q, ala] == 1
    one = _scan(case, b, candidates=cand)                   # one group: nothing is across
    assert all(not z["Ei"].any() for z in one.res.values())
    assert any(z["Ei"].any() for z in scan.res.values())


def test_oracle_in_float32_stays_inside_the_rule():
    case = {k: v[:2] for k, v in SC.make_case(17).items()}
    M = SC.max_coord(case)
    o64 = SC.oracle(case)
    o32 = SC.oracle(case, dtype=np.float32)
    worst = 0.0
    for s64, s32 in zip(o64, o32):
        assert s64.res.keys() == s32.res.keys() and len(s64.res) > 0
        for key, z in s64.res.items():
            bnd = SC.bound(z, M)
            err = np.abs(z["E"] - s32.res[key]["E"])
            assert (err <= bnd).all(), (key, err.max())
            worst = max(worst, float((err / np.maximum(bnd, 1e-300)).max()))
    assert worst > 0.0
    print(f"float32 build against float64: largest |dE| / bound = {worst:.4f}")


def test_recorded_seeds_meet_the_cap():
    for N in (1, 2, 17):                                    # (15, 16, 33 are asserted where test_gpu_scan.py prepares them)
        SC.oracle(SC.make_case(N), key=N)                   # asserts inside
    chi, count, energy = SC.edge_table()
    rows = SC.rows_of_type() * count[:20]
    near = {int(r) - SC.ROW_TILE * round(int(r) / SC.ROW_TILE) for r in rows if r >= SC.ROW_TILE - 4}
    assert {-1, 0, 1} <= near, sorted(near)                 # rows one below, at and one above a multiple of the row tile
    assert {1, 63, 64, 65, 128} <= set(count.tolist())


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------

def test_struct_layout_agrees_with_the_header():
    cls = _capi.MutationScanArgs
    assert [(n, t) for n, t in cls._fields_] == header_fields("pf_mutation_scan_args")
    last = cls._fields_[-1][0]
    assert getattr(cls, last).offset + 4 <= C.sizeof(cls) and C.sizeof(cls) % 8 == 0
    names = [n for n, _ in cls._fields_]
    assert names[:7] == ["pos", "atom_mask", "aa", "residue_index", "positions", "candidates", "group"]
    pack = [n for n, _ in _capi.PackArgs._fields_]
    assert names[7:19] == pack[pack.index("radius"):pack.index("work") + 1]         # the same tables, rotamer table and workspace


def test_header_keeps_the_abi_version():
    text = open(HEADER).read()
    assert "#define PF_ABI_VERSION 65" in text and _capi.ABI_VERSION == 65
    assert text.index("int pf_pack_work_bytes(") < text.index("} pf_mutation_scan_args;") < text.index("int pf_mutation_scan_fwd(")
    assert text.index("int pf_mutation_scan_fwd(") < text.index("int pf_mutation_scan_work_bytes(") < text.index("} pf_interface_energy_args;")
    assert "#define PF_MUTATION_SCAN_TYPES 20" in text and geometry.SCAN_TYPES == SO.TYPES == 20
    assert "mutscan.hip" in build.SOURCES
    assert {"pf_mutation_scan_fwd", "pf_mutation_scan_work_bytes"} <= set(_capi.EXPORTED_SYMBOLS)


def test_library_exports_the_entry_points_and_work_bytes():
    lib = _capi.load()
    assert lib.pf_abi_version() == _capi.ABI_VERSION == 65
    assert lib.pf_mutation_scan_fwd(None, None) == -1
    assert lib.pf_mutation_scan_fwd(C.byref(_capi.MutationScanArgs()), None) == -1
    per = 15 * 16 + 16 + 16                                 # environment atoms, bounds, type bytes: nothing per type or rotamer
    assert lib.pf_mutation_scan_work_bytes(1, 1) == per == 272
    assert lib.pf_mutation_scan_work_bytes(64, 144) == 64 * 144 * per
    assert lib.pf_mutation_scan_work_bytes(2, 512) == 2 * 512 * per
    assert lib.pf_mutation_scan_work_bytes(0, 7) == 0 and lib.pf_mutation_scan_work_bytes(3, 0) == 0
    for bad in ((-1, 4), (4, -1), (1, 513), (65535, 512)):              # as pf_pack_work_bytes: negative, N > 512, more than INT_MAX
        assert lib.pf_mutation_scan_work_bytes(*bad) == -1, bad
        assert lib.pf_pack_work_bytes(*bad, 1) == -1, bad


# ---- the wrappers --------------------------------------------------------------------------------------------------------------------

def test_wrapper_argument_checks():
    B, N = 2, 5
    pos, mask = torch.zeros(B, N, 15, 3), torch.ones(B, N, 15, dtype=torch.bool)
    aa, idx = torch.zeros(B, N, dtype=torch.int64), torch.arange(N).repeat(B, 1)
    sel = torch.ones(B, N, dtype=torch.bool)
    p = geometry.mutation_scan
    for args in ((torch.zeros(B, N, 4, 3), mask, aa, idx, sel), (pos[0], mask, aa, idx, sel), (pos, mask[:, :, :14], aa, idx, sel),
                 (pos, mask, aa[:, :4], idx, sel), (pos, mask, aa, idx[:1], sel), (pos, mask, aa, idx, sel[:, :3]),
                 (pos, mask, aa, idx, None), (pos, mask, aa, None, sel),
                 (torch.zeros(1, 513, 15, 3), torch.ones(1, 513, 15), torch.zeros(1, 513), torch.zeros(1, 513), torch.zeros(1, 513))):
        with pytest.raises(ValueError):
            p(*args)
    chi, count, energy = geometry.rotamer_table()
    for kw in (dict(cutoff=0.0), dict(cutoff=float("nan")), dict(weights=(1.0, 2.0)), dict(weights=(1.0, 2.0, 3.0, 4.0, float("inf"))),
               dict(rotamers=(chi, count)), dict(rotamers=(chi[:20], count, energy)), dict(rotamers=(chi, count + 200, energy)),
               dict(rotamers=(torch.zeros(21, 129, 4), torch.ones(21), torch.zeros(21, 129))),
               dict(group=torch.zeros(B, N + 1)), dict(candidates=torch.ones(19)), dict(candidates=torch.ones(B, N, 21)),
               dict(candidates=torch.ones(N, 20)), dict(candidates=torch.ones(B, 20))):
        with pytest.raises(ValueError):
            p(pos, mask, aa, idx, sel, **kw)
    with pytest.raises(_capi.PepflowHipError):              # a CPU tensor is not computed on: there is no fallback
        p(pos, mask, aa, idx, sel)
    for kw in (dict(backbone="atoms"), dict(candidates="XYZ"), dict(candidates=["ALA", "UNK"]), dict(candidates=[]), dict(candidates=3),
               dict(top_k=-1), dict(top_k=2.5), dict(hot_spot=float("nan"))):
        with pytest.raises(ValueError):
            metrics.mutation_scan({}, {}, **kw)


def test_candidates_normalisation():
    B, N = 2, 3
    assert geometry._scan_candidates(None, B, N) is None
    one = torch.zeros(20)
    one[[0, 7]] = 1.0
    c = geometry._scan_candidates(one, B, N)
    assert c.shape == (B, N, 20) and c.dtype == torch.bool and bool((c == (one != 0)).all())
    full = torch.zeros(B, N, 20, dtype=torch.int32)
    full[1, 2, 5] = 3
    c = geometry._scan_candidates(full, B, N)
    assert c.dtype == torch.bool and c.sum() == 1 and bool(c[1, 2, 5])
    assert geometry._scan_candidates(np.ones(20, bool), B, N).all()
    idx = PO.res_index()
    assert metrics._scan_candidate_mask("all") is None
    assert metrics._scan_candidate_mask("ALA").nonzero().flatten().tolist() == [idx["ALA"]]
    assert sorted(metrics._scan_candidate_mask(("TRP", "LEU", "LEU")).nonzero().flatten().tolist()) == sorted([idx["TRP"], idx["LEU"]])
    assert metrics.HOT_SPOT_DDE > 0
