"""CPU checks of TM-align (pepflowww_amd.geometry.tm_align and what is built on it): the numpy float64 oracle (tmalign_oracle.py)
against closed forms, the fixed-correspondence search and an enumeration of every alignment of short chains; the degenerate-fit
rule; the C ABI's bounds; and the argument checks that run before any device work."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import tm_oracle as TO  # noqa: E402
import tmalign_oracle as TA  # noqa: E402
from pepflowww_amd import _capi, geometry, metrics  # noqa: E402


def _chain(rng, n):
    """a CA-like random walk: steps of 3.8 A"""
    d = rng.standard_normal((n, 3))
    return np.cumsum(3.8 * d / np.linalg.norm(d, axis=1, keepdims=True), 0)


def _helix(n):
    """ideal alpha-helix CA trace: radius 2.3 A, rise 1.5 A, 100 degrees per residue"""
    k = np.arange(n)
    a = np.deg2rad(100.0) * k
    return np.stack([2.3 * np.cos(a), 2.3 * np.sin(a), 1.5 * k], 1)


def _strand(n):
    """extended-strand CA trace: 3.3 A along the axis, +-0.9 A zigzag"""
    k = np.arange(n)
    return np.stack([3.3 * k, 0.9 * (-1.0) ** k, np.zeros(n)], 1)


@pytest.mark.parametrize("L", [3, 4, 5, 8, 12, 25, 60])
def test_identical_and_rigidly_moved_chains(L):
    rng = np.random.default_rng(L)
    x = _chain(rng, L)
    for y in (x, x @ TO.rigid(rng).T + rng.uniform(-50, 50, 3)):
        r = TA.tm_align(x, y)
        assert r["tm"] == pytest.approx(1.0, abs=1e-12) and r["tm_x"] == pytest.approx(1.0, abs=1e-12)
        assert r["n_aligned"] == L and r["rmsd"] < 1e-9
        np.testing.assert_array_equal(r["y2x"], np.arange(L))
        assert r["kept"].all()


@pytest.mark.parametrize("Lx,k,m", [(40, 10, 20), (30, 3, 12), (60, 25, 30)])
def test_sub_fragment_is_found(Lx, k, m):
    rng = np.random.default_rng(Lx + k)
    x = _chain(rng, Lx)
    y = x[k:k + m] @ TO.rigid(rng).T + rng.uniform(-50, 50, 3)
    r = TA.tm_align(x, y)
    np.testing.assert_array_equal(r["y2x"], np.arange(k, k + m))
    assert r["tm"] == pytest.approx(1.0, abs=1e-9)
    assert r["tm_x"] == pytest.approx(m / Lx, abs=1e-9)
    fixed = TO.tm_score(x[:m], y)["tm"]                              # the same residues paired by position
    assert fixed < 0.6 and r["tm"] - fixed > 0.4


def test_insertion_is_skipped():
    rng = np.random.default_rng(7)
    x = _chain(rng, 24)
    loop = x[11] + np.array([0.0, 0.0, 30.0]) + _chain(rng, 6)        # a loop far from the chain
    y = np.concatenate([x[:12], loop, x[12:]]) @ TO.rigid(rng).T
    r = TA.tm_align(x, y)
    expect = np.full(len(y), -1)
    expect[:12], expect[18:] = np.arange(12), np.arange(12, 24)
    np.testing.assert_array_equal(r["y2x"], expect)
    assert r["tm_x"] == pytest.approx(1.0, abs=1e-9)
    assert r["tm"] == pytest.approx(24 / 30, abs=1e-9)


@pytest.mark.parametrize("L,noise", [(8, 0.3), (15, 0.5), (25, 0.4), (40, 0.5)])
def test_near_native_agrees_with_the_fixed_search(L, noise):
    rng = np.random.default_rng(L)
    x = _chain(rng, L)
    y = x @ TO.rigid(rng).T + noise * rng.standard_normal((L, 3)) / np.sqrt(3.0)
    r = TA.tm_align(x, y)
    np.testing.assert_array_equal(r["y2x"], np.arange(L))
    assert r["n_aligned"] == L
    assert r["tm"] == pytest.approx(TO.tm_score(x, y)["tm"], abs=1e-9)


def test_ca_secondary_structure_of_ideal_traces():
    ss, _ = TA.sec_str(_helix(12))
    assert "".join(TA.SS_CHARS[c] for c in ss) == "CC" + "H" * 8 + "CC"
    ss, _ = TA.sec_str(_strand(12))
    assert "".join(TA.SS_CHARS[c] for c in ss) == "CC" + "E" * 8 + "CC"
    ss, _ = TA.sec_str(_helix(4))
    assert (ss == TA.SS_C).all()


def test_degenerate_fit_rule():
    rng = np.random.default_rng(3)
    for _ in range(20):
        a, b = rng.standard_normal(3), rng.standard_normal(3)
        R = TA.two_point_rotation(a, b)
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)
        assert np.linalg.det(R) == pytest.approx(1.0, abs=1e-12)
        ua, ub = a / np.linalg.norm(a), b / np.linalg.norm(b)
        np.testing.assert_allclose(R @ ua, ub, atol=1e-12)
        # the smallest such rotation: its angle is the angle between a and b
        assert np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)) == pytest.approx(np.arccos(ua @ ub), abs=1e-7)
    R = TA.two_point_rotation(np.array([1.0, 0.0, 0.0]), np.array([-2.0, 0.0, 0.0]))       # antiparallel: a half turn
    np.testing.assert_allclose(R, np.diag([-1.0, -1.0, 1.0]), atol=1e-15)                  # about z = x x e_y
    np.testing.assert_array_equal(TA.two_point_rotation(np.zeros(3), np.ones(3)), np.eye(3))
    x = rng.standard_normal((1, 2, 3))
    y = rng.standard_normal((1, 2, 3))
    for w, rot in (([True, False], np.eye(3)), ([True, True], TA.two_point_rotation(x[0, 1] - x[0, 0], y[0, 1] - y[0, 0]))):
        R, t = TA.kabsch_b(x, y, np.array([w]))
        np.testing.assert_allclose(R[0], rot, atol=1e-15)
        k = np.nonzero(w)[0]
        np.testing.assert_allclose(R[0] @ x[0, k].mean(0) + t[0], y[0, k].mean(0), atol=1e-12)
    R, t = TA.kabsch_b(x, y, np.array([[False, False]]))
    np.testing.assert_array_equal(R[0], np.eye(3)) and np.testing.assert_array_equal(t[0], np.zeros(3))
    # peptides of 3 - 8 residues take the one- and two-point fragment fits of stage 3: the result is defined and reproducible
    for L in range(3, 9):
        x, y = _chain(rng, L), _chain(rng, L + 1)
        r1, r2 = TA.tm_align(x, y), TA.tm_align(x, y)
        assert np.isfinite(r1["tm"]) and 0.0 < r1["tm"] <= 1.0 + 1e-12 and r1["tm"] == r2["tm"]
        np.testing.assert_array_equal(r1["y2x"], r2["y2x"])


def _all_alignments(Lx, Ly):
    for k in range(3, min(Lx, Ly) + 1):
        for xi in itertools.combinations(range(Lx), k):
            for yj in itertools.combinations(range(Ly), k):
                m = np.full(Ly, -1)
                m[list(yj)] = xi
                yield m


def test_upper_bound_from_every_alignment_of_short_chains():
    """TM-align's tm is the final scoring of one sequential alignment, so it never exceeds the best of them all"""
    rng = np.random.default_rng(11)
    worst = 0.0
    for Lx, Ly in ((5, 5), (6, 5), (6, 6), (7, 6)):
        x = _chain(rng, Lx)
        y = _chain(rng, Ly) * 0.5 + x[:Ly] * 0.5 if Ly <= Lx else _chain(rng, Ly)
        r = TA.tm_align(x, y)
        best = max(TA.final_score(x, y, m, Ly) for m in _all_alignments(Lx, Ly))
        assert r["tm"] <= best + 1e-9
        worst = max(worst, best - r["tm"])
    assert worst < 0.3, worst                                           # a heuristic search: 0.253 here, bounded


def test_c_abi_bounds():
    lib = _capi.load()
    assert lib.pf_tm_align_lds_bytes(0) == 0 and lib.pf_tm_align_lds_bytes(geometry.TM_ALIGN_MAX_N + 1) == 0
    assert lib.pf_tm_align_lds_bytes(25) < 4096                         # a peptide's LDS does not grow with the slot count
    assert lib.pf_tm_align_lds_bytes(512) <= 160 * 1024
    a = _capi.TmAlignArgs()
    # argument checks return before any device call: any non-null address will do
    a.x = a.y = a.mx = a.my = a.pairs = a.tm = a.tm_x = a.rmsd = a.n_aligned = a.len_x = a.len_y = 16
    a.Bx, a.By, a.P = 2, 2, 1
    a.N = geometry.TM_ALIGN_MAX_N + 1
    assert lib.pf_tm_align_fwd(C.byref(a), None) == -2                  # PF_E_TOOLARGE
    a.N, a.P = geometry.TM_ALIGN_MAX_N, 0
    assert lib.pf_tm_align_fwd(C.byref(a), None) == 0                   # an empty work list launches nothing
    a.rot = 16                                                          # rot without trans
    assert lib.pf_tm_align_fwd(C.byref(a), None) == -1
    a.rot, a.y2x = None, 16                                             # y2x without kept
    assert lib.pf_tm_align_fwd(C.byref(a), None) == -1
    a.y2x, a.max_len = None, -1
    assert lib.pf_tm_align_fwd(C.byref(a), None) == -1
    assert C.sizeof(_capi.TmAlignArgs) == 16 * 8 + 5 * 4 + 4           # 16 pointers, 5 ints, padded to 8


def test_wrappers_reject_bad_arguments_before_device_work():
    x = torch.zeros(4, 10, 3)
    m = torch.ones(4, 10, dtype=torch.bool)
    pairs = torch.tensor([[0, 1]], dtype=torch.int32)
    with pytest.raises(ValueError):
        geometry.tm_align(x, torch.zeros(4, 9, 3), m, m, pairs)
    with pytest.raises(ValueError):
        geometry.tm_align(x, x, m[:, :9], m, pairs)
    with pytest.raises(ValueError):
        geometry.tm_align(x, x, m, m, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        geometry.tm_align(torch.zeros(4, 10), x, m, m, pairs)
    with pytest.raises(ValueError):
        geometry.tm_align(x, x, m, m, pairs, max_len=-1)
    big = torch.zeros(2, geometry.TM_ALIGN_MAX_N + 1, 3)
    bm = torch.ones(2, geometry.TM_ALIGN_MAX_N + 1, dtype=torch.bool)
    with pytest.raises(_capi.PepflowHipError, match="bound"):
        geometry.tm_align(big, big, bm, bm, pairs)
    with pytest.raises(_capi.PepflowHipError, match="bound"):
        geometry.pairwise_tm_align(big, bm)
    final = {"trans": torch.zeros(2, 6, 3), "trans_1": torch.zeros(2, 6, 3), "seqs": torch.zeros(2, 6, dtype=torch.long),
             "seqs_1": torch.zeros(2, 6, dtype=torch.long)}
    gen = torch.tensor([[1, 1, 1, 1, 0, 0], [1, 1, 1, 0, 0, 0]], dtype=torch.bool)
    with pytest.raises(ValueError, match="tm_mode"):
        metrics.structure_scores(final, {"generate_mask": gen}, tm_mode="align")
