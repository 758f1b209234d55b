"""CPU checks of TM-score (pepflowww_amd.geometry.tm_score and what is built on it): the numpy float64 oracle of the search
(tm_oracle.py) against closed forms and against an independent optimiser, the C ABI's bounds, and the argument checks that run
before any device work."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import tm_oracle as TO  # noqa: E402
from pepflowww_amd import _capi, geometry, metrics  # noqa: E402


@pytest.mark.parametrize("n,expected", [(128, [128, 64, 32, 16, 8, 4]), (15, [15, 7, 4]), (8, [8, 4]), (4, [4]), (3, [3])])
def test_seed_lengths(n, expected):
    assert TO.seed_lengths(n) == expected


def test_d0_from_the_formula():
    assert TO.d0_of(10) == 0.5 and TO.d0_of(21) == 0.5                  # 1.24 cbrt(6) - 1.8 = 0.453 < 0.5
    assert abs(TO.d0_of(22) - (1.24 * 7 ** (1 / 3) - 1.8)) < 1e-12 and TO.d0_of(22) > 0.5
    assert abs(TO.d0_of(100) - (1.24 * 85 ** (1 / 3) - 1.8)) < 1e-12


def test_identical_and_rigidly_moved_sets_score_one():
    rng = np.random.default_rng(1)
    for n in (3, 4, 9, 25, 60):
        x = rng.uniform(-10, 10, size=(n, 3))
        assert abs(TO.tm_score(x, x)["tm"] - 1.0) < 1e-12, n
        y = x @ TO.rigid(rng).T + rng.uniform(-50, 50, 3)
        o = TO.tm_score(x, y)
        assert abs(o["tm"] - 1.0) < 1e-12, n
        assert abs(np.linalg.det(o["rot"]) - 1.0) < 1e-12


@pytest.mark.parametrize("n", [8, 10, 24, 40])
def test_two_halves(n):
    rng = np.random.default_rng(n)
    x = rng.uniform(0, 10, size=(n, 3))
    y = x.copy()
    D = 100.0
    y[n // 2:] += D * np.array([0.6, 0.0, 0.8])
    o = TO.tm_score(x, y)
    d0 = TO.d0_of(n)
    assert abs(o["tm"] - (0.5 + 0.5 / (1 + (D / d0) ** 2))) < 1e-12, (n, o["tm"])


def test_rescoring_and_global_kabsch_bound():
    rng = np.random.default_rng(7)
    for case in range(8):
        n = int(rng.integers(5, 40))
        x = rng.uniform(-8, 8, size=(n, 3))
        y = x @ TO.rigid(rng).T + rng.uniform(-50, 50, 3) + rng.normal(scale=3.0, size=(n, 3))
        mx, my = rng.random(n) > 0.15, rng.random(n) > 0.15
        o = TO.tm_score(x, y, mx, my)
        if o["n_ali"] < 3:
            continue
        sel = mx & my
        assert o["lnorm"] == my.sum()
        assert TO.score(x[sel], y[sel], o["rot"], o["trans"], o["d0"], o["lnorm"]) == o["tm"]
        r, t = TO.kabsch(x[sel], y[sel])
        assert o["tm"] >= TO.score(x[sel], y[sel], r, t, o["d0"], o["lnorm"]), case


# Largest gaps observed between the best of 33 local optimisations and the oracle over these 20 cases: 0.106 overall, all of it at
# d0 = 0.5 (n <= 21) where the noise is 5 - 10 d0 and the search, which cuts at d0_search = 4.5 +- 1 A, does not resolve the
# sub-angstrom optimum (a property of the algorithm, shared by the TMscore program); 0.021 where d0 >= 1 A.  Bounds: those plus a
# margin.
SEARCH_GAP_BOUND = 0.12
SEARCH_GAP_BOUND_D0_1 = 0.03


def test_search_quality_against_an_independent_optimiser():
    from scipy.optimize import minimize
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(11)
    worst = worst_d0_1 = 0.0
    for case in range(20):
        n = int(rng.integers(10, 61))
        noise = float(rng.uniform(1.0, 6.0))
        x = rng.uniform(-10, 10, size=(n, 3))
        y = x @ TO.rigid(rng).T + rng.uniform(-50, 50, 3) + rng.normal(scale=noise, size=(n, 3))
        o = TO.tm_score(x, y)
        d0sq = o["d0"] ** 2

        def neg(p):
            e = x @ Rotation.from_rotvec(p[:3]).as_matrix().T + p[3:] - y
            return -float((d0sq / (d0sq + (e * e).sum(1))).sum() / n)

        starts = [np.r_[Rotation.from_matrix(o["rot"]).as_rotvec(), o["trans"]]]
        for _ in range(32):
            r = Rotation.random(random_state=int(rng.integers(1 << 31)))
            starts.append(np.r_[r.as_rotvec(), y.mean(0) - r.apply(x.mean(0))])
        found = max(-minimize(neg, s, method="Powell", options={"xtol": 1e-6, "ftol": 1e-10}).fun for s in starts)
        worst = max(worst, found - o["tm"])
        if o["d0"] >= 1.0:
            worst_d0_1 = max(worst_d0_1, found - o["tm"])
    print(f"largest gap over the oracle: {worst:.4g} ({worst_d0_1:.4g} where d0 >= 1)")
    assert worst <= SEARCH_GAP_BOUND and worst_d0_1 <= SEARCH_GAP_BOUND_D0_1, (worst, worst_d0_1)


def test_c_abi_bounds():
    lib = _capi.load()
    assert lib.pf_tm_score_work_slots(25) == 1                          # 57 seeds
    assert lib.pf_tm_score_work_slots(128) == 9                         # 522 seeds
    assert lib.pf_tm_score_work_slots(512) == 33                        # 2 082 seeds
    assert lib.pf_tm_score_work_slots(513) == -1 and lib.pf_tm_score_work_slots(0) == -1
    a = _capi.TmScoreArgs()
    # argument checks return before any device call: any non-null address will do
    a.x = a.y = a.mx = a.my = a.pairs = a.tm = a.count = a.lnorm = a.work = 16
    a.Bx, a.By, a.P = 2, 2, 1
    a.N = geometry.TM_MAX_N + 1
    assert lib.pf_tm_score_fwd(C.byref(a), None) == -2                  # PF_E_TOOLARGE
    a.N, a.P = geometry.TM_MAX_N, 0
    assert lib.pf_tm_score_fwd(C.byref(a), None) == 0                   # an empty work list launches nothing
    a.rot = 16                                                          # rot without trans
    assert lib.pf_tm_score_fwd(C.byref(a), None) == -1
    assert C.sizeof(_capi.TmScoreArgs) == 12 * 8 + 4 * 4


def test_wrappers_reject_bad_arguments_before_device_work():
    x = torch.zeros(4, 10, 3)
    m = torch.ones(4, 10, dtype=torch.bool)
    pairs = torch.tensor([[0, 1]], dtype=torch.int32)
    with pytest.raises(ValueError):
        geometry.tm_score(x, torch.zeros(4, 9, 3), m, m, pairs)
    with pytest.raises(ValueError):
        geometry.tm_score(x, x, m[:, :9], m, pairs)
    with pytest.raises(ValueError):
        geometry.tm_score(x, x, m, m, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        geometry.tm_score(torch.zeros(4, 10), x, m, m, pairs)
    big = torch.zeros(2, geometry.TM_MAX_N + 1, 3)
    bm = torch.ones(2, geometry.TM_MAX_N + 1, dtype=torch.bool)
    with pytest.raises(_capi.PepflowHipError, match="bound"):
        geometry.tm_score(big, big, bm, bm, pairs)
    with pytest.raises(_capi.PepflowHipError, match="bound"):
        geometry.pairwise_tm_score(big, bm)
    final = {"trans": torch.zeros(2, 6, 3), "trans_1": torch.zeros(2, 6, 3), "seqs": torch.zeros(2, 6, dtype=torch.long),
             "seqs_1": torch.zeros(2, 6, dtype=torch.long)}
    gen = torch.tensor([[1, 1, 1, 1, 0, 0], [1, 1, 1, 0, 0, 0]], dtype=torch.bool)
    with pytest.raises(ValueError, match="generate_mask"):
        metrics.structure_scores(final, {"generate_mask": gen})
    with pytest.raises(ValueError, match="labels"):
        metrics.structure_scores(final, {"generate_mask": gen}, groups=[0, 1, 2])
