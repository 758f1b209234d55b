"""CPU checks of DSSP (pepflowww_amd.geometry.dssp and what is built on it): the numpy float64 oracle (dssp_oracle.py) on ideal
helices, prolines and strand pairs built here, its pattern stage on hand-made bond lists, the C ABI's bounds, and the wrapper's
argument checks and code helpers.  Every expected string is derived in the comments from the asserted bonds and the rules."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import dssp_build as DB  # noqa: E402
import dssp_oracle as DO  # noqa: E402
from pepflowww_amd import _capi, geometry, metrics  # noqa: E402


def bond_list(o):
    return sorted((int(d), int(a)) for d, a in zip(*np.nonzero(o["bonds"])))


def ss_str(ss):
    return DO.to_string(ss)


# ---- ideal helices ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [12, 20])
@pytest.mark.parametrize("angles,step,code", [(DB.ALPHA, 4, "H"), (DB.HELIX_310, 3, "G"), (DB.PI, 5, "I")])
def test_ideal_helix(angles, step, code, n):
    bb = DB.helix(n, angles)
    o = DO.dssp(bb, np.ones(n, bool))
    # the only bond of donor i + step is to acceptor i
    assert bond_list(o) == [(i + step, i) for i in range(n - step)]
    assert o["margin"] > 0.1
    # step-turns start at 0 .. n-1-step; consecutive starts at i-1, i (1 <= i <= n-1-step) cover i .. i+step-1, so 1 .. n-2
    assert ss_str(o["ss"]) == "-" + code * (n - 2) + "-"


def test_helix_energies_and_kappa():
    for angles, step, e in ((DB.ALPHA, 4, -2.286), (DB.HELIX_310, 3, -2.926), (DB.PI, 5, -5.13)):
        o = DO.dssp(DB.helix(16, angles), np.ones(16, bool))
        assert np.allclose(o["energy"][step:, 0], e, atol=1e-3)
    for angles, kappa in ((DB.ALPHA, 109.4), (DB.HELIX_310, 65.5), (DB.PI, 137.5)):
        ca = DB.helix(16, angles)[:, 1]
        u, w = ca[8] - ca[6], ca[10] - ca[8]
        assert abs(np.degrees(np.arccos(u @ w / np.linalg.norm(u) / np.linalg.norm(w))) - kappa) < 0.1


# ---- prolines --------------------------------------------------------------------------------------------------------------------

def test_one_proline_keeps_the_helix_whole():
    n, k = 20, 10
    bb = DB.helix(n, DB.ALPHA)
    pro = np.zeros(n, bool)
    pro[k] = True
    o = DO.dssp(bb, np.ones(n, bool), pro=pro)
    assert bond_list(o) == [(i + 4, i) for i in range(n - 4) if i + 4 != k]
    # 4-turns at 0..15 but 6; H from the pairs (i-1, i) with i in 1..5 (1..8) and 8..15 (8..18): overlapping at k-2 = 8
    assert ss_str(o["ss"]) == "-" + "H" * 18 + "-"


def test_four_prolines_split_the_helix_with_bends():
    n, k = 20, 10
    bb = DB.helix(n, DB.ALPHA)
    pro = np.zeros(n, bool)
    pro[k:k + 4] = True
    o = DO.dssp(bb, np.ones(n, bool), pro=pro)
    assert bond_list(o) == [(i + 4, i) for i in range(n - 4) if not k <= i + 4 < k + 4]
    # 4-turns at 0..5 and 10..15: H on 1..8 (i = 1..5) and 11..18 (i = 11..15).  9 and 10 lie strictly inside the turns at 6..8 /
    # 7..9 only, all gone: no T; kappa ~ 109 > 70: S
    ss = o["ss"]
    assert ss_str(ss) == "-" + "H" * 8 + "SS" + "H" * 8 + "-"
    simple = geometry.ss_simplify(torch.from_numpy(ss)).numpy()
    assert simple[9] == 2 and simple[10] == 2


# ---- strand pairs ----------------------------------------------------------------------------------------------------------------

def test_antiparallel_pair():
    bb, ch = DB.strand_pair("anti")
    o = DO.dssp(bb, np.ones(12, bool), ch)
    assert bond_list(o) == [(1, 10), (3, 8), (5, 6), (8, 3), (10, 1)]
    # antiparallel bridges: (1,10) and (3,8) by 1<->10, 3<->8; (2,9) by 3->8 and 10->1; (4,7) by 5->6 and 8->3.  One ladder of
    # four bridges: E on 1..4 and 7..10
    assert ss_str(o["ss"]) == "-EEEE--EEEE-"
    assert [(d["type"], d["ib"], d["ie"], d["jb"], d["je"], d["n"]) for d in o["ladders"]] == [("A", 1, 4, 7, 10, 4)]


def test_parallel_pair():
    bb, ch = DB.strand_pair("par")
    o = DO.dssp(bb, np.ones(12, bool), ch)
    assert bond_list(o) == [(2, 7), (4, 9), (7, 0), (9, 2), (11, 4)]
    # parallel bridges: (1,7) by 2->7, 7->0; (3,9) by 4->9, 9->2; (2,8) by 9->2, 2->7; (4,10) by 11->4, 4->9: E on 1..4, 7..10
    assert ss_str(o["ss"]) == "-EEEE--EEEE-"
    assert [(d["type"], d["ib"], d["ie"], d["jb"], d["je"], d["n"]) for d in o["ladders"]] == [("P", 1, 4, 7, 10, 4)]


def test_single_bridge_gives_b():
    bb, ch = DB.strand_pair("anti")
    keep = list(range(6)) + [9, 10, 11]                                  # the partner cut down to its residues 9..11
    o = DO.dssp(bb[keep], np.ones(9, bool), ch[keep])
    # 1 <-> 10 (now 7) stay; 3 -> 8 and 8 -> 3 lost their partner; (5, 6) is gone
    assert bond_list(o) == [(1, 7), (7, 1)]
    assert ss_str(o["ss"]) == "-B-----B-"


# ---- the pattern stage from hand-made bond lists ---------------------------------------------------------------------------------

def brk(n, at=()):
    b = np.zeros(n, bool)
    b[0] = True
    b[list(at)] = True
    return b


def test_h_beats_e():
    n = 20
    bonds = [(i + 4, i) for i in range(2, 7)]                            # 4-turns at 2..6: H on 3..9
    bonds += [(4, 16), (16, 4), (6, 14), (14, 6)]                        # antiparallel (4,16), (5,15) (6->14, 16->4), (6,14)
    ss, info = DO.assign(bonds, brk(n))
    assert [(d["type"], d["ib"], d["ie"], d["jb"], d["je"]) for d in info["ladders"]] == [("A", 4, 6, 14, 16)]
    assert ss_str(ss) == "---HHHHHHH----EEE---"


def test_g_only_on_a_free_span():
    n = 16
    bonds = [(4, 0), (5, 1)]                                             # 4-turns at 0, 1: H on 1..4
    bonds += [(6, 3), (7, 4)]                                            # 3-turns at 3, 4: span 4..6 holds H -> no G; T on 5, 6
    bonds += [(13, 10), (14, 11)]                                        # 3-turns at 10, 11: G on 11..13
    ss, _ = DO.assign(bonds, brk(n))
    # 4-turn at 1 puts 2, 3 strictly inside (H anyway); 3-turns at 3, 4: 4 (H), 5, 6 -> T; at 10, 11: 11..13 (G)
    assert ss_str(ss) == "-HHHHTT----GGG--"


def test_t_and_s():
    n = 10
    ca_bent = DB.helix(n, DB.ALPHA)[:, 1]                                # kappa ~ 109 on 2..7
    ca_flat = DB.helix(n, DB.HELIX_310)[:, 1]                            # kappa ~ 65.5
    ss, _ = DO.assign([(6, 2)], brk(n), ca_bent)                         # one 4-turn at 2: no H, T on 3..5
    assert ss_str(ss) == "--STTTSS--"
    ss, _ = DO.assign([(6, 2)], brk(n), ca_flat)
    assert ss_str(ss) == "---TTT----"


def _parallel_bridge(i, j):
    return [(i + 1, j), (j, i - 1)]


def _anti_bridge(i, j):
    return [(i, j), (j, i)]


@pytest.mark.parametrize("gi,gj,joined", [(2, 5, True), (5, 2, True), (2, 6, False), (6, 2, False)])
def test_parallel_bulge(gi, gj, joined):
    n = 34
    # ladder X: (4,20), (5,21); ladder Y: (5+gi, 21+gj), (6+gi, 22+gj)
    iy, jy = 5 + gi, 21 + gj
    bonds = []
    for i, j in ((4, 20), (5, 21), (iy, jy), (iy + 1, jy + 1)):
        bonds += _parallel_bridge(i, j)
    ss, info = DO.assign(bonds, brk(n))
    exp = np.full(n, "-")
    if joined:                                                           # one gap < 3, the other < 6: one E run per strand
        exp[4:iy + 2] = "E"
        exp[20:jy + 2] = "E"
        assert len(info["ladders"]) == 1
    else:
        for a, b in ((4, 6), (iy, iy + 2), (20, 22), (jy, jy + 2)):
            exp[a:b] = "E"
        assert len(info["ladders"]) == 2
    assert ss_str(ss) == "".join(exp)


@pytest.mark.parametrize("gi,gj,joined", [(2, 5, True), (5, 2, True), (2, 6, False), (6, 2, False)])
def test_antiparallel_bulge(gi, gj, joined):
    n = 34
    # ladder X: (4,27), (5,26); ladder Y: (5+gi, 26-gj), (6+gi, 25-gj)
    iy, jy = 5 + gi, 26 - gj
    bonds = []
    for i, j in ((4, 27), (5, 26), (iy, jy), (iy + 1, jy - 1)):
        bonds += _anti_bridge(i, j)
    ss, info = DO.assign(bonds, brk(n))
    exp = np.full(n, "-")
    if joined:
        exp[4:iy + 2] = "E"
        exp[jy - 1:28] = "E"
        assert len(info["ladders"]) == 1
    else:
        for a, b in ((4, 6), (iy, iy + 2), (26, 28), (jy - 1, jy + 1)):
            exp[a:b] = "E"
        assert len(info["ladders"]) == 2
    assert ss_str(ss) == "".join(exp)


def test_no_bridge_across_a_break():
    n = 32
    bonds = []
    for i, j in ((4, 27), (5, 26), (6, 25)):
        bonds += _anti_bridge(i, j)
    assert ss_str(DO.assign(bonds, brk(n))[0]) == "----EEE" + "-" * 18 + "EEE----"
    # a break between 4 and 5: (4,27) and (5,26) need 3..5 / 4..6 unbroken; (6,25) alone is left: B
    exp = np.full(n, "-")
    exp[[6, 25]] = "B"
    assert ss_str(DO.assign(bonds, brk(n, [5]))[0]) == "".join(exp)
    # the same from the mask: residue 5 masked cuts it off from both neighbours, (4,27), (5,26), (6,25) all need it
    mask = np.ones(n, bool)
    mask[5] = False
    exp = np.full(n, "-")
    exp[5] = "."
    assert ss_str(DO.assign(bonds, brk(n), mask=mask)[0]) == "".join(exp)


def _helix_with_break(kind):
    n, k = 20, 10
    bb = DB.helix(n, DB.ALPHA)
    mask, chain = np.ones(n, bool), np.zeros(n, np.int64)
    if kind == "chain":
        chain[k:] = 1
    elif kind == "mask":
        mask[k] = False
    else:                                                                # move residues k.. away along C(k-1) -> N(k): 3 A
        v = bb[k, 0] - bb[k - 1, 2]
        bb = bb.copy()
        bb[k:] += (3.0 / np.linalg.norm(v) - 1.0) * v
    return bb, mask, chain


@pytest.mark.parametrize("kind", ["chain", "mask", "gap"])
def test_no_helix_across_a_break(kind):
    bb, mask, chain = _helix_with_break(kind)
    o = DO.dssp(bb, mask, chain)
    assert list(np.nonzero(o["brk"])[0]) == ([0, 10, 11] if kind == "mask" else [0, 10])
    bl = bond_list(o)
    assert (10, 6) not in bl                                             # a segment's first residue is no donor
    assert all((i + 4, i) in bl for i in range(6))                       # the first segment keeps its helix bonds
    assert all((i + 4, i) in bl for i in range(11 if kind == "mask" else 10, 16))
    if kind == "mask":
        # turns at 0..5 and 11..15: H on 1..8 and 12..18; 9 and 11 are in no turn's inside and have no bend (breaks within 2)
        assert ss_str(o["ss"]) == "-" + "H" * 8 + "-.-" + "H" * 7 + "-"
    else:
        # turns at 0..5 and 10..15 (6..9 would cross the break): H on 1..8 and 11..18; 9, 10: no turn, no bend
        assert ss_str(o["ss"]) == "-" + "H" * 8 + "--" + "H" * 8 + "-"


# ---- the C ABI and the wrapper ---------------------------------------------------------------------------------------------------

def test_c_abi_bounds():
    lib = _capi.load()
    a = _capi.DsspArgs()
    a.pos = a.mask = a.ss = 16                                           # checks return before any device call
    a.B, a.N, a.n_atoms, a.pro = 2, geometry.DSSP_MAX_N + 1, 4, 12
    assert lib.pf_dssp_fwd(C.byref(a), None) == -2                       # PF_E_TOOLARGE
    a.N, a.n_atoms = 8, 3
    assert lib.pf_dssp_fwd(C.byref(a), None) == -1                       # fewer than N, CA, C, O
    a.n_atoms, a.hb_acc = 4, 16                                          # hb_acc without hb_energy
    assert lib.pf_dssp_fwd(C.byref(a), None) == -1
    a.hb_acc, a.B = None, 0
    assert lib.pf_dssp_fwd(C.byref(a), None) == 0                        # nothing to do
    assert C.sizeof(_capi.DsspArgs) == 7 * 8 + 4 * 4


def test_wrapper_rejects_bad_arguments_before_device_work():
    pos = torch.zeros(2, 10, 15, 3)
    m = torch.ones(2, 10, dtype=torch.bool)
    with pytest.raises(ValueError):
        geometry.dssp(torch.zeros(2, 10, 3), m)
    with pytest.raises(ValueError):
        geometry.dssp(torch.zeros(2, 10, 3, 3), m)                       # A < 4
    with pytest.raises(ValueError):
        geometry.dssp(pos, m[:, :9])
    with pytest.raises(ValueError):
        geometry.dssp(pos, m, chain=torch.zeros(2, 9, dtype=torch.long))
    with pytest.raises(ValueError):
        geometry.dssp(pos, m, aa=torch.zeros(3, 10, dtype=torch.long))
    with pytest.raises(ValueError, match="bound"):
        geometry.dssp(torch.zeros(1, geometry.DSSP_MAX_N + 1, 4, 3), torch.ones(1, geometry.DSSP_MAX_N + 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="backbone"):
        metrics.secondary_structure({}, {}, backbone="pdb")


def test_ss_simplify_and_strings():
    ss = torch.tensor([[0, 1, 2, 3, 4, 5, 6, 7, 255], [7, 0, 0, 255, 2, 2, 6, 5, 3]], dtype=torch.uint8)
    assert geometry.ss_simplify(ss).tolist() == [[0, 1, 1, 0, 0, 2, 2, 2, 255], [2, 0, 0, 255, 1, 1, 2, 2, 0]]
    assert geometry.ss_simplify(ss).dtype == torch.uint8
    assert geometry.ss_strings(ss) == ["HBEGITS-", "-HHEESTG"]
    assert geometry.ss_strings(ss, simplified=True) == ["HEEHHCCC", "CHHEECCH"]
    assert geometry.SS_SYMBOLS == "HBEGITS-" == DO.SYMBOLS
