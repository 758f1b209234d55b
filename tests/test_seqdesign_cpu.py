"""CPU checks of the fixed-backbone sequence design (pf_sequence_design_fwd; iterated conditional modes over type and rotamer with the
packer's energy; not ProteinMPNN, not Rosetta fixbb): the design oracle (seqdesign_oracle.py) against pack_oracle.Structure with one-hot
candidates and against scan_oracle.Scan with one designed residue, the descent property that the term F exists for, brute force on the
seeded small cases and their selection condition, the hand-made pair, the ctypes struct layout against the header, the insertion
points, the entry points' refusals and work sizes, and the wrappers' argument checks.  The comparison rule is pack_cases.bound."""
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
import seqdesign_cases as DC  # noqa: E402
import seqdesign_oracle as DO  # noqa: E402
from test_lddt_cpu import HEADER, header_fields  # noqa: E402
from pepflowww_amd import _capi, build, geometry, metrics  # noqa: E402


def design(case, b=0, **kw):
    return DO.Design(*[case[k][b] for k in DC.KEYS], **kw)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b", [0, 1])
def test_one_hot_candidates_are_the_packing_oracle(b):
    """candidates {aa[q]}: the residue is simply repacked.  The total of any state is pack_oracle's (its E_self holds the rows against
    the frames of the other packed residues, here P holds them), and from the same state the search takes pack_oracle's path: the
    conditional energies differ by F, which no rotamer of a fixed type changes.  The START is not the packer's: E_self here leaves
    the other designed residues out altogether (their frames change with their type), the packer's counts their frames in."""
    case = PC.make_case(117, 4, 17)
    N = 17
    mov = case["movable"][b]
    cand = np.zeros((N, 20), bool)
    ok = (case["aa"][b] >= 0) & (case["aa"][b] <= 19)
    cand[np.flatnonzero(ok), case["aa"][b][ok]] = True
    o = DO.Design(case["pos"][b], case["atom_mask"][b], case["aa"][b], case["residue_index"][b], mov, candidates=cand)
    ref = PO.Structure(case["pos"][b], case["atom_mask"][b], case["aa"][b], case["residue_index"][b], mov)
    assert list(o.dlist) == list(ref.plist) and len(o.dlist) >= 4
    types = [int(case["aa"][b][q]) for q in o.dlist]
    want = ref.icm(3)
    run = o.icm(3, start=list(zip(types, want["start"])))
    assert [[r for _, r in row] for row in run["choices"]] == want["choices"] and run["changed"] == want["changed"]
    assert not any(run["changed_types"]) and [t for t, _ in run["state"]] == types
    np.testing.assert_allclose(run["energy_trace"], want["energy_trace"], rtol=0, atol=1e-9)
    assert sum(want["changed"]) > 0
    own = o.icm(3)                                          # from its own start: the same total function, a descent
    assert abs(own["energy_trace"][-1] - ref.total([r for _, r in own["state"]])["E"]) <= 1e-9
    assert abs(own["energy_trace"][0] - ref.total([r for _, r in own["start"]])["E"]) <= 1e-9
    # an empty candidate set is the own type as well
    cand[o.dlist[0]] = False
    again = DO.Design(case["pos"][b], case["atom_mask"][b], case["aa"][b], case["residue_index"][b], mov, candidates=cand)
    assert again.types[0] == [int(case["aa"][b][o.dlist[0]])]


def test_one_designed_residue_is_the_scan():
    case = SC.make_case(17)
    b = 1
    qs = np.flatnonzero(SO.Scan(*[case[k][b] for k in SC.KEYS]).scanned)[[0, 5, -1]]
    for q in qs:
        pos = np.arange(17) == q
        scan = SO.Scan(case["pos"][b], case["atom_mask"][b], case["aa"][b], case["residue_index"][b], pos)
        o = DO.Design(case["pos"][b], case["atom_mask"][b], case["aa"][b], case["residue_index"][b], pos)
        e, rot, _ = scan.energy()
        prof, prot = o.profile(o.start())
        np.testing.assert_allclose(prof[q], e[q], rtol=0, atol=1e-12)
        assert np.array_equal(prot[q], rot[q]) and np.isinf(prof[np.arange(17) != q]).all()
        assert o.start()[0][0] == int(np.argmin(e[q]))
        ref = np.linspace(-1.0, 1.0, 20)
        with_ref = DO.Design(case["pos"][b], case["atom_mask"][b], case["aa"][b], case["residue_index"][b], pos, ref_energy=ref)
        assert with_ref.start()[0][0] == int(np.argmin(e[q] + ref.astype(np.float32)))


def test_every_accepted_move_lowers_the_total_by_the_conditional_difference():
    """the reason F exists: with it every difference of two conditional energies is a difference of the total, so the search is a
    descent; without it (the packer's conditional energy, where a partner's frame never changes) it is not"""
    worst, n_moves, off = 0.0, 0, 0.0
    for seed in DC.small_seeds()[:6]:
        o, _ = DC.small_design(seed)
        run = o.icm(8, audit=True)
        for saved, drop in run["moves"]:
            assert saved > 0.0 and abs(saved - drop) <= 1e-9, (seed, saved, drop)
            worst = max(worst, abs(saved - drop))
            n_moves += 1
        assert all(b <= a + 1e-9 for a, b in zip(run["energy_trace"], run["energy_trace"][1:]))
        bare, _ = DC.small_design(seed, with_F=False)
        for saved, drop in bare.icm(8, audit=True)["moves"]:
            off = max(off, abs(saved - drop))
    case, cand = DC.hand_pair()
    run = design(case, candidates=cand[0]).icm(8, audit=True)
    assert run["moves"] and all(abs(s - d) <= 1e-9 for s, d in run["moves"])
    assert n_moves >= 4
    assert off > 1e-6, off                                  # dropping F from the oracle breaks the identity
    print(f"{n_moves} accepted moves: largest |conditional - total| difference {worst:.2e}; without F {off:.3e}")


def test_brute_force_on_a_small_case():
    seed = DC.small_seeds()[0]
    o, _ = DC.small_design(seed)
    best, arg = o.brute_force()
    assert abs(o.total(arg)["E"] - best) <= 1e-9
    states = list(DO.state_product(o))
    assert 27 <= len(states) <= 5832
    rng = np.random.default_rng(3)
    for k in rng.choice(len(states), 60, replace=False):
        assert o.total(list(states[k]))["E"] >= best - 1e-9
    # and ICM's answer is a local minimum of the total: no single residue's change lowers it
    run = o.icm(8)
    final = o.total(run["state"])["E"]
    for p in range(len(o.dlist)):
        for key in o.flat_self(p)[0]:
            trial = list(run["state"])
            trial[p] = key
            assert o.total(trial)["E"] >= final - 1e-9


def test_small_case_selection_condition():
    """among the first 40 seeds at least 12 whose oracle ICM reaches the brute-force minimum (pack_cases.small_seeds' rule and numbers);
    at least 6 of those kept have every decision clear by ten bounds"""
    seeds = DC.small_seeds()
    assert len(seeds) == DC.SMALL_WANTED == 12 and max(seeds) < 40
    assert sum(DC.small_report(s)["clear"] for s in seeds) >= DC.SMALL_CLEAR == 6
    chi, count, energy = DC.small_table()
    assert count.max() <= 6 and chi.shape == (21, 6, 4)
    for s in seeds[:3]:
        o, _ = DC.small_design(s)
        assert len(o.dlist) == 3 and all(len(t) == 3 for t in o.types)


def test_hand_pair_on_the_oracle():
    """two facing residues: each alone takes a large side chain pointed at the other; together one of them gives way"""
    case, cand = DC.hand_pair()
    o = design(case, candidates=cand[0])
    scan = SO.Scan(case["pos"][0], case["atom_mask"][0], case["aa"][0], case["residue_index"][0], case["designed"][0], candidates=cand[0])
    e, rot, _ = scan.energy()
    alone = [(int(np.argmin(e[q])), int(rot[q, int(np.argmin(e[q]))])) for q in range(2)]
    run = o.icm(8)
    assert run["state"] != alone and sum(run["changed"]) > 0
    assert o.total(alone)["E"] - o.total(run["state"])["E"] > 1.0
    assert all(t != PO.res_index()["ALA"] for t, _ in alone)
    assert run["state"][0][0] != alone[0][0] and run["changed_types"][0] > 0       # the joint answer differs in TYPE
    first = o.flat(0, run["start"])[1]["E"]                                         # the first visit's margin: far beyond any bound
    assert np.sort(first)[1] - np.sort(first)[0] > 10.0 * DC.bound(o.total(run["state"]), DC.max_coord(case))


def test_too_many_designed_residues():
    case = DC.many_case(65)
    o = design(case, 0, candidates=np.zeros((80, 20), bool))
    assert o.status == 1 and not o.designed.any() and len(o.dlist) == 0
    case = DC.many_case(64)
    o = design(case, 0, candidates=np.zeros((80, 20), bool))
    assert o.status == 0 and o.designed.sum() == 64


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------

def test_struct_layout_agrees_with_the_header():
    cls = _capi.SeqDesignArgs
    assert [(n, t) for n, t in cls._fields_] == header_fields("pf_sequence_design_args")
    last = cls._fields_[-1][0]
    assert getattr(cls, last).offset + 4 <= C.sizeof(cls) and C.sizeof(cls) % 8 == 0
    names = [n for n, _ in cls._fields_]
    assert names[:7] == ["pos", "atom_mask", "aa", "residue_index", "designed", "candidates", "ref_energy"]
    pack = [n for n, _ in _capi.PackArgs._fields_]
    assert names[7:19] == pack[pack.index("radius"):pack.index("work") + 1]         # the same tables, rotamer table and workspace


def test_header_keeps_the_abi_version_and_the_insertion_points():
    text = open(HEADER).read()
    assert "#define PF_ABI_VERSION 65" in text and _capi.ABI_VERSION == 65
    assert text.index("int pf_mutation_scan_work_bytes(") < text.index("} pf_sequence_design_args;") < text.index("int pf_sequence_design_fwd(")
    assert text.index("int pf_sequence_design_fwd(") < text.index("int pf_sequence_design_work_bytes(") < text.index("} pf_interface_energy_args;")
    assert "#define PF_SEQ_DESIGN_MAX_RES 64" in text and geometry.SEQ_DESIGN_MAX_RES == DO.MAX_RES == 64
    assert "#define PF_SEQ_DESIGN_TYPES 20" in text and geometry.SEQ_DESIGN_TYPES == DO.TYPES == 20
    i = build.SOURCES.index("seqdesign.hip")
    assert build.SOURCES[i - 1] == "mutscan.hip"
    k = _capi.EXPORTED_SYMBOLS.index("pf_mutation_scan_work_bytes")
    assert _capi.EXPORTED_SYMBOLS[k + 1:k + 3] == ("pf_sequence_design_fwd", "pf_sequence_design_work_bytes")
    kernel = open(os.path.join(os.path.dirname(HEADER), "..", "pepflowww_amd", "csrc", "seqdesign.hip")).read()
    assert "NOT ProteinMPNN" in kernel and "NOT Rosetta fixbb" in kernel and "atomic" not in kernel.split("#include")[1]


def test_library_exports_the_entry_points_and_work_bytes():
    lib = _capi.load()
    assert lib.pf_abi_version() == _capi.ABI_VERSION == 65
    assert lib.pf_sequence_design_fwd(None, None) == -1
    assert lib.pf_sequence_design_fwd(C.byref(_capi.SeqDesignArgs()), None) == -1
    size = lambda B, N, R, M: B * (16 + N * (15 * 16 + 16 + 16 + 4) + M * (4 + 20 * 4 + 20 * 4 * R))  # noqa: E731
    assert lib.pf_sequence_design_work_bytes(1, 1, 1, 1) == size(1, 1, 1, 1) == 456
    assert lib.pf_sequence_design_work_bytes(64, 128, 108, 64) == size(64, 128, 108, 64)
    assert lib.pf_sequence_design_work_bytes(2, 512, 128, 64) == size(2, 512, 128, 64)
    assert lib.pf_sequence_design_work_bytes(0, 7, 5, 64) == 0
    # nothing per residue and type and rotamer and atom: N = 512 costs what its environment costs
    assert lib.pf_sequence_design_work_bytes(1, 512, 128, 64) - lib.pf_sequence_design_work_bytes(1, 1, 128, 64) == 511 * 276
    for bad in ((-1, 4, 4, 4), (4, -1, 4, 4), (1, 513, 4, 4), (1, 4, 0, 4), (1, 4, 129, 4), (1, 4, 4, 0), (1, 4, 4, 65), (65535, 512, 128, 64)):
        assert lib.pf_sequence_design_work_bytes(*bad) == -1, bad


# ---- the wrappers --------------------------------------------------------------------------------------------------------------------

def test_wrapper_argument_checks():
    B, N = 2, 5
    pos, mask = torch.zeros(B, N, 15, 3), torch.ones(B, N, 15, dtype=torch.bool)
    aa, idx = torch.zeros(B, N, dtype=torch.int64), torch.arange(N).repeat(B, 1)
    sel = torch.ones(B, N, dtype=torch.bool)
    p = geometry.design_sequence
    for args in ((torch.zeros(B, N, 4, 3), mask, aa, idx, sel), (pos[0], mask, aa, idx, sel), (pos, mask[:, :, :14], aa, idx, sel),
                 (pos, mask, aa[:, :4], idx, sel), (pos, mask, aa, idx[:1], sel), (pos, mask, aa, idx, sel[:, :3]),
                 (pos, mask, aa, idx, None), (pos, mask, aa, None, sel),
                 (torch.zeros(1, 513, 15, 3), torch.ones(1, 513, 15), torch.zeros(1, 513), torch.zeros(1, 513), torch.zeros(1, 513))):
        with pytest.raises(ValueError):
            p(*args)
    chi, count, energy = geometry.rotamer_table()
    for kw in (dict(cutoff=0.0), dict(cutoff=float("nan")), dict(weights=(1.0, 2.0)), dict(sweeps=-1), dict(sweeps=2.5), dict(sweeps=True),
               dict(rotamers=(chi, count)), dict(rotamers=(chi, count + 200, energy)),
               dict(candidates=torch.ones(19)), dict(candidates=torch.ones(B, N, 21)), dict(candidates=torch.ones(B, 20)),
               dict(ref_energy=torch.zeros(19)), dict(ref_energy=[0.0] * 21), dict(ref_energy=[float("nan")] + [0.0] * 19),
               dict(ref_energy=[float("inf")] * 20), dict(ref_energy="high"), dict(ref_energy=torch.zeros(2, 20))):
        with pytest.raises(ValueError):
            p(pos, mask, aa, idx, sel, **kw)
    with pytest.raises(ValueError, match="inf"):            # the offending value is named
        p(pos, mask, aa, idx, sel, ref_energy=[float("inf")] + [0.0] * 19)
    with pytest.raises(ValueError, match="-3"):
        p(pos, mask, aa, idx, sel, sweeps=-3)
    with pytest.raises(_capi.PepflowHipError):              # a CPU tensor is not computed on: there is no fallback
        p(pos, mask, aa, idx, sel)
    for kw in (dict(backbone="atoms"), dict(backbone="packed"), dict(candidates="XYZ"), dict(candidates=["ALA", "UNK"]), dict(candidates=[]),
               dict(sweeps=-1), dict(trace=True), dict(ref_energy=[1.0, 2.0])):
        with pytest.raises(ValueError):
            metrics.design_sequences({}, {}, **kw)
    assert geometry._ref_energy(None) is None
    r = geometry._ref_energy(np.arange(20))
    assert r.dtype == torch.float32 and r.tolist() == list(range(20))
