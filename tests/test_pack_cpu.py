"""CPU checks of the rotamer side-chain packing (a staggered rotamer grid, the package's Vina-form pair energy, iterated conditional
modes; not SCWRL4, not Rosetta's packer): the ctypes struct layout against the header, the insertion points, the entry points'
refusals, the wrapper's argument checks, the rotamer table, and the numpy oracle (pack_oracle.py): its loop form against its
vectorised form, a hand-placed pair against energy_oracle.pair_terms, the exclusions, its search against brute force on the seeded small
cases of the GPU tests, the fp32 cost of the frame chain against pack_cases.py's bound, and the hand-computed cases."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import energy_oracle as EO  # noqa: E402
import pack_cases as PC  # noqa: E402
import pack_oracle as PO  # noqa: E402
import torsion_oracle as TO  # noqa: E402
from test_lddt_cpu import HEADER, header_fields  # noqa: E402
from pepflowww_amd import _capi, build, geometry, metrics  # noqa: E402
from pepflowww_amd.preprocess import _tables  # noqa: E402

SMALL_SEEDS = [3, 10, 14, 15, 17, 18, 25, 26, 27, 31, 36, 39]       # pack_cases.small_seeds(), repeated below


def structure(case, b=0, **kw):
    return PO.Structure(case["pos"][b], case["atom_mask"][b], case["aa"][b], case["residue_index"][b], case["movable"][b], **kw)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------

def test_struct_layout_agrees_with_the_header():
    cls = _capi.PackArgs
    assert [(n, t) for n, t in cls._fields_] == header_fields("pf_pack_args")
    last = cls._fields_[-1][0]
    assert getattr(cls, last).offset + 4 <= C.sizeof(cls) and C.sizeof(cls) % 8 == 0


def test_header_keeps_the_abi_version_and_the_insertion_points():
    text = open(HEADER).read()
    assert "#define PF_ABI_VERSION 65" in text and _capi.ABI_VERSION == 65
    assert text.index("} pf_cluster_args;") < text.index("int pf_cluster_work_bytes(") < text.index("} pf_pack_args;")
    assert text.index("} pf_pack_args;") < text.index("int pf_pack_sidechains_fwd(") < text.index("int pf_pack_work_bytes(")
    assert text.index("int pf_pack_work_bytes(") < text.index("} pf_interface_energy_args;")
    assert "#define PF_PACK_MAX_N 512" in text and geometry.PACK_MAX_N == 512
    assert "#define PF_PACK_MAX_ROT 128" in text and geometry.PACK_MAX_ROT == 128
    assert "#define PF_PACK_SLOTS 15" in text and geometry.PACK_SLOTS == 15
    assert "#define PF_PACK_ROT_ATOMS 9" in text and geometry.PACK_ROT_ATOMS == PO.RA == 9
    i = build.SOURCES.index("packing.hip")
    assert build.SOURCES[i - 1] == "clustering.hip" and build.SOURCES[i + 1:] == ["interface_energy.hip", "relax.hip"]
    k = _capi.EXPORTED_SYMBOLS.index("pf_cluster_work_bytes")
    assert _capi.EXPORTED_SYMBOLS[k + 1:k + 3] == ("pf_pack_sidechains_fwd", "pf_pack_work_bytes")
    assert _capi.EXPORTED_SYMBOLS[-3:] == ("pf_interface_energy_fwd", "pf_relax_energy_fwd", "pf_relax_fwd")


def test_library_exports_the_entry_points():
    lib = _capi.load()
    assert lib.pf_abi_version() == _capi.ABI_VERSION == 65
    assert lib.pf_pack_sidechains_fwd(None, None) == -1
    assert lib.pf_pack_sidechains_fwd(C.byref(_capi.PackArgs()), None) == -1


def test_work_bytes():
    lib = _capi.load()
    per = lambda R: 15 * 16 + 16 + 16 + 16 + R * (9 * 16 + 4)  # noqa: E731  (environment, two bounds, type bytes; atoms and E_self)
    assert lib.pf_pack_work_bytes(1, 1, 1) == per(1) == 436
    assert lib.pf_pack_work_bytes(64, 144, 108) == 64 * 144 * per(108)
    assert lib.pf_pack_work_bytes(2, 512, 128) == 2 * 512 * per(128)
    assert lib.pf_pack_work_bytes(0, 7, 5) == 0 and lib.pf_pack_work_bytes(3, 0, 5) == 0
    for bad in ((-1, 4, 4), (4, -1, 4), (1, 513, 4), (1, 4, 0), (1, 4, 129), (1, 4, -3), (4096, 512, 128)):
        assert lib.pf_pack_work_bytes(*bad) == -1, bad


def test_wrapper_argument_checks():
    B, N = 2, 5
    pos, mask = torch.zeros(B, N, 15, 3), torch.ones(B, N, 15, dtype=torch.bool)
    aa, idx = torch.zeros(B, N, dtype=torch.int64), torch.arange(N).repeat(B, 1)
    mov = torch.ones(B, N, dtype=torch.bool)
    p = geometry.pack_sidechains
    for args in ((torch.zeros(B, N, 4, 3), mask, aa, idx, mov), (pos[0], mask, aa, idx, mov), (pos, mask[:, :, :14], aa, idx, mov),
                 (pos, mask, aa[:, :4], idx, mov), (pos, mask, aa, idx[:1], mov), (pos, mask, aa, idx, mov[:, :3]),
                 (pos, mask, aa, idx, None), (pos, mask, aa, None, mov),
                 (torch.zeros(1, 513, 15, 3), torch.ones(1, 513, 15), torch.zeros(1, 513), torch.zeros(1, 513), torch.zeros(1, 513))):
        with pytest.raises(ValueError):
            p(*args)
    chi, count, energy = geometry.rotamer_table()
    for kw in (dict(sweeps=-1), dict(sweeps=1.5), dict(sweeps=True), dict(cutoff=0.0), dict(cutoff=float("nan")), dict(weights=(1.0, 2.0)),
               dict(weights=(1.0, 2.0, 3.0, 4.0, float("inf"))), dict(rotamers=(chi, count)), dict(rotamers=(chi[:20], count, energy)),
               dict(rotamers=(chi, count, energy[:, :5])), dict(rotamers=(chi[:, :, :3], count, energy)),
               dict(rotamers=(torch.zeros(21, 129, 4), torch.ones(21), torch.zeros(21, 129))),
               dict(rotamers=(chi, count + 200, energy)), dict(rotamers=(chi, count * 0, energy)),
               dict(rotamers=(chi * float("nan"), count, energy))):
        with pytest.raises(ValueError):
            p(pos, mask, aa, idx, mov, **kw)
    for bad in (0, -30, 200, float("nan"), "x", 2):        # 2 degrees: 9 * 180 rotamers for GLN
        with pytest.raises(ValueError):
            geometry.rotamer_table(bad)
    with pytest.raises(ValueError):
        metrics.pack_samples({}, {}, backbone="atoms")
    with pytest.raises(ValueError):
        metrics.pack_samples({}, {}, sweeps=-2)


# ---- the tables ----------------------------------------------------------------------------------------------------------------------

def test_rotamer_table_counts_and_order():
    chi, count, energy = geometry.rotamer_table()
    idx = _tables()["res_index"]
    assert chi.shape == (21, 108, 4) and chi.dtype == torch.float32 and count.shape == (21,) and energy.shape == (21, 108)
    assert not energy.any() and int(count[20]) == 1
    assert {n: int(count[idx[n]]) for n in PO.COUNTS_30} == PO.COUNTS_30
    ochi, ocount, _ = PO.rotamer_table()
    assert np.array_equal(chi.numpy(), ochi) and np.array_equal(count.numpy(), ocount)
    deg = lambda name: np.degrees(chi[idx[name], :int(count[idx[name]])].double().numpy())  # noqa: E731
    assert np.allclose(deg("PRO"), [[30, -35, 0, 0], [-30, 35, 0, 0]])
    assert np.allclose(deg("SER")[:, 0], [60, 180, 300]) and not deg("ALA").any() and not deg("GLY").any()
    leu = deg("LEU")                                        # chi1 slowest, each ascending
    assert np.allclose(leu[:, :2], [[a, b] for a in (60, 180, 300) for b in (60, 180, 300)])
    assert np.allclose(deg("ASP")[:6, 1], np.arange(0, 180, 30)) and np.allclose(deg("ASN")[:12, 1], np.arange(0, 360, 30))
    gln = deg("GLN")
    assert np.allclose(gln[:12, 2], np.arange(0, 360, 30)) and np.allclose(gln[12, :3], [60, 180, 0]) and np.allclose(gln[-1, :3], [300, 300, 330])
    assert np.allclose(deg("GLU")[:6, 2], np.arange(0, 180, 30))
    for name in PO.COUNTS_30:                               # rows beyond the count are zero
        assert not chi[idx[name], int(count[idx[name]]):].any(), name
    c60 = geometry.rotamer_table(60)[1]
    assert int(c60[idx["GLN"]]) == 54 and int(c60[idx["PHE"]]) == 9 and int(c60[idx["ARG"]]) == 81


def test_every_rotamer_measures_its_own_chi():
    chi, count, _ = geometry.rotamer_table()
    chi_atoms = geometry.chi_atom_table().numpy()
    T = PO.rigid()
    ideal, seen = PC.ideal_backbones(), set()
    nerf = PC.hand_lone()["pos"][0, 0, :3].astype(np.float64)          # N-CA-C 111.2 degrees: off every type's ideal
    worst = 0.0
    for name, t in [(n, t) for n, t in _tables()["res_index"].items() if t < 20] * 2:
        bb = (ideal[t], nerf)[int(name in seen)]
        seen.add(name)
        rows = chi[t, :int(count[t])].numpy()
        atoms, exists, cb = PO.build_rotamers(bb, t, rows)
        pos = np.zeros((len(rows), 15, 3))
        pos[:, :3], pos[:, 4], pos[:, 5:14] = bb, cb, atoms
        mask = np.broadcast_to(T["mask"][t], (len(rows), 15))
        got = TO.torsions(pos, mask, np.full(len(rows), t), chi_atoms)
        n_chi = PO.N_CHI[name]
        assert got["defined"][:, 4:4 + n_chi].all() and not got["defined"][:, 4 + n_chi:].any(), name
        err = TO.wrap(got["angles"][:, 4:4 + n_chi] - rows[:, :n_chi].astype(np.float64))
        worst = max(worst, float(err.max()) if err.size else 0.0)
    # Every type on its own ideal backbone (the rigid-group table's N, CA, C) and on a NeRF backbone whose N is elsewhere: chi1 is
    # measured from the real N, and the chain's first angle is corrected for it (pack_oracle.chi1_offset).  The ideal tables are
    # fp32 (entries rounded by 2^-24, five composed rotations): 2e-6 rad; 7.2e-7 was seen.
    assert worst <= 2e-6, worst


def test_packing_pair_table():
    tab, own = geometry.packing_pair_table(), PO.own_pair_table()
    assert tab.shape == (21, 15, 15) and tab.dtype == torch.bool and np.array_equal(tab.numpy(), own)
    t, names = _tables()["res_index"], _tables()["atom_names"]
    pair = lambda res, a, b: bool(tab[t[res], names[t[res]].index(a), names[t[res]].index(b)])  # noqa: E731
    assert pair("SER", "OG", "O") and not pair("SER", "OG", "N") and not pair("SER", "OG", "C")         # three bonds: left out
    assert pair("LEU", "CD1", "N") and not pair("LEU", "CD1", "CA") and not pair("LEU", "CG", "N")
    assert pair("ARG", "NH1", "CG") and not pair("ARG", "CG", "NH1") and not pair("ARG", "NH1", "CD")   # each pair once
    assert not pair("PRO", "CD", "C") and not pair("PRO", "CD", "N") and pair("PRO", "CD", "O")         # through the ring: CD-N-CA-C
    assert not tab[t["ALA"]].any() and not tab[t["GLY"]].any() and not tab[20].any()
    assert not tab[:, :5].any() and not tab[:, 14].any()
    mask = geometry._pack_own_mask_table()
    assert all(bool(mask[r, a] >> b & 1) == bool(tab[r, a, b]) for r in (1, 12, 14, 18) for a in range(15) for b in range(15))


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------

def test_loop_form_equals_vectorised_form():
    chi, count, _ = PO.rotamer_table()
    rng = np.random.default_rng(5)
    bb = PC.make_case(3, 1, 6)["pos"][0, :, :3].astype(np.float64)
    for t in range(20):
        rows = np.concatenate([chi[t, :count[t]].astype(np.float64), rng.uniform(-4, 4, (3, 4))])
        at, ex, cb = PO.build_rotamers(bb[t % 6], t, rows)
        for r in (0, len(rows) // 2, len(rows) - 1):
            a1, e1, c1 = PO.build_rotamer_loop(bb[t % 6], t, rows[r])
            assert np.array_equal(e1, ex) and np.abs(a1 - at[r]).max() <= 1e-12 and np.abs(c1 - cb).max() <= 1e-12
        assert ex.sum() == PO.rigid()["mask"][t, 5:14].sum()


def test_hand_placed_pair_against_pair_terms():
    # a SER whose OG (an acceptor and donor, radius 1.7) sees one fixed backbone N (a donor, 1.8) of another residue at 3.0 A
    case = PC.hand_lone("SER")
    case = {k: np.concatenate([v, v], 1) for k, v in case.items()}
    case["residue_index"][0, 1], case["movable"][0, 1] = 5, False
    case["atom_mask"][0, 1] = False
    ser = _tables()["res_index"]["SER"]
    at, _, _ = PO.build_rotamers(case["pos"][0, 0, :3], ser, PO.rotamer_table()[0][ser, :3])
    cb = structure(PC.hand_lone("SER")).env_X[0, 4]
    away = (at[1, 0] - cb) / np.linalg.norm(at[1, 0] - cb)
    case["pos"][0, 1, 0] = at[1, 0] + 3.0 * away
    case["atom_mask"][0, 1, 0] = True
    with_n, alone = structure(case), structure(PC.hand_lone("SER"))
    r = np.linalg.norm(at[1, 0] - case["pos"][0, 1, 0].astype(np.float64))
    t, _ = EO.pair_terms(np.array(r - 1.7 - 1.8), np.array(False), np.array(True))
    assert t[4] > 0.5                                       # d = -0.5: a hydrogen bond
    assert abs((with_n.self_[0]["E"][1] - alone.self_[0]["E"][1]) - float(t @ np.asarray(EO.WEIGHTS))) <= 1e-12


def test_exclusions():
    idx = _tables()["res_index"]
    # SG - SG: a packed CYS beside a fixed CYS whose SG sits on the packed one's SG
    case = PC.hand_lone("CYS")
    case = {k: np.concatenate([v, v], 1) for k, v in case.items()}
    case["residue_index"][0, 1], case["movable"][0, 1] = 7, False
    case["atom_mask"][0, 1] = False
    at, _, _ = PO.build_rotamers(case["pos"][0, 0, :3], idx["CYS"], PO.rotamer_table()[0][idx["CYS"], :3])
    case["pos"][0, 1, 5] = at[0, 0] + np.array([0.0, 0.0, 2.0])
    case["atom_mask"][0, 1, 5] = True
    alone = structure(PC.hand_lone("CYS")).self_[0]["E"]
    assert np.array_equal(structure(case).self_[0]["E"], alone)         # the SG is never a partner
    case["aa"][0, 1] = idx["SER"]                                       # the same atom as a serine's OG is
    assert structure(case).self_[0]["E"][0] > alone[0] + 0.1
    # the PRO ring against the previous residue: CD and CG against C, CA, O of residue_index - 1
    case = PC.make_case(2, 1, 6)
    case["aa"][0, 3], case["movable"][0] = idx["PRO"], np.arange(6) == 3
    case["residue_index"][0] = np.arange(6)
    case["atom_mask"][0, :, :4] = True
    o = structure(case)
    case["residue_index"][0] = [0, 1, 2, 4, 5, 6]                       # a gap before the proline: nothing is excluded now
    gap = structure(case)
    extra = gap.self_[0]["pairs"] - o.self_[0]["pairs"]
    assert (extra == 4).all()                                           # CD - CA, C, O and CG - C, all within the cutoff
    # own-residue pairs at most three bonds apart are never evaluated: a lone LEU has exactly the table's pairs
    lone = structure(PC.hand_lone("LEU"))
    assert (lone.self_[0]["pairs"] == PO.own_pair_table()[idx["LEU"]][:, :14].sum()).all()     # (no OXT in the case)


def test_small_seeds_icm_against_brute_force():
    assert PC.small_seeds() == SMALL_SEEDS
    late = 0
    for s in SMALL_SEEDS:
        r = PC.small_report(s)
        assert r["global_min"] and r["clear"] >= 0.9, (s, r)
        late += r["late"]
    assert late >= 2, late


def test_frame_chain_bound_against_the_oracle_in_fp32():
    case = PC.make_case(11, 2, 33)
    M = PC.max_coord(case)
    worst = 0.0
    for b in range(2):
        o64, o32 = structure(case, b), structure(case, b, dtype=np.float32)
        for a64, a32, ex in zip(o64.atoms, o32.atoms, o64.exists):
            if ex.any():
                worst = max(worst, float(np.abs(a64[:, ex] - a32[:, ex]).max()))
        worst = max(worst, float(np.abs(o64.env_X[:, 4] - o32.env_X[:, 4]).max()))
        assert float(np.abs(o64.env_X).max()) <= M and max(float(np.abs(a).max()) for a in o64.atoms) <= M
        assert max(o64.ext) <= PC.REACH
    assert 0.0 < worst <= PC.build_err(M), (worst, PC.build_err(M))
    # and what that costs an energy stays inside the rule
    for b in range(2):
        o64, o32 = structure(case, b, near=PC.pos_err(M)), structure(case, b, dtype=np.float32)
        for s64, s32 in zip(o64.self_, o32.self_):
            assert (np.abs(s64["E"] - s32["E"]) <= PC.bound(s64, M)).all()


def test_near_cap_holds_on_the_gpu_cases():
    for seed, B, N in ((1, 6, 17), (2, 3, 33)):
        PC.oracle(PC.make_case(seed, B, N))                 # asserts inside


# ---- hand-computed cases ---------------------------------------------------------------------------------------------------------------

def test_hand_ser():
    case, want, d = PC.hand_ser()
    assert d[0] > 3.7 and abs(d[1] - 2.1) < 1e-3 and abs(d[2] - 2.1) < 1e-3
    o = structure(case)
    assert o.start() == [want] and o.icm(8)["rotamer"] == [want]
    e = o.self_[0]
    lone = structure(PC.hand_lone("SER")).self_[0]
    assert abs(e["rep"][0] - lone["rep"][0]) < 1e-12                     # the carbon adds no repulsion to chi1 = 60
    assert abs(e["rep"][1] - lone["rep"][1] - 2.25) < 0.01 and abs(e["rep"][2] - lone["rep"][2] - 2.25) < 0.01      # (2.1 - 3.6)^2
    assert e["E"][1] - e["E"][0] > 1.5 and e["E"][2] - e["E"][0] > 1.5


def test_hand_leu():
    o = structure(PC.hand_leu())
    run = o.icm(8)
    assert run["start"] == [3, 3] and run["rotamer"] == [8, 8] and run["sweeps_run"] == 2 and run["changed"] == [2, 0]
    between = lambda cur: float(o.pair(0, 1, cur[1], rows=cur[0])["rep"][0])  # noqa: E731
    assert between(run["start"]) > 10.0 and between(run["rotamer"]) == 0.0
    assert run["energy_trace"][0] > 9.0 and run["energy_trace"][-1] < 1.0
    assert o.brute_force()[1] == [8, 8]


def test_hand_lone():
    o = structure(PC.hand_lone("MET"))
    run = o.icm(8)
    e = o.self_[0]["E"]
    assert run["start"] == run["rotamer"] == [int(np.argmin(e))] and run["changed"] == [0] and run["sweeps_run"] == 1
    assert np.sort(e)[1] - np.sort(e)[0] > 1e-4             # no tie: "the smallest r attaining the minimum" is not put to the test
    pos, mask, chi = o.output(run["rotamer"])
    case = PC.hand_lone("MET")
    assert np.array_equal(pos[0, :4], case["pos"][0, 0, :4]) and mask[0, :8].all() and not mask[0, 8:].any()
    # with a table energy the minimum of (b) + energy moves where the energy says
    chi_t, count, energy = PO.rotamer_table()
    energy = energy.copy()
    energy[_tables()["res_index"]["MET"], 5] = -50.0
    assert structure(PC.hand_lone("MET"), rotamers=(chi_t, count, energy)).start() == [5]
