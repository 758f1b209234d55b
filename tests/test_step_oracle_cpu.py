"""tests/step_oracle.py on the oracle alone (no GPU): the cases reach every region they list, the oracle's own fp32 step passes the
tight rule, and three planted faults of 5e-5 -- the size the whole-tensor bar of gpu_util.assert_close (1e-4) lets through -- are
reported in the region they were planted in while that bar passes them: the gap tests/test_gpu_step_forward.py closes, asserted."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import gpu_util as G  # noqa: E402
import block_oracle as K  # noqa: E402
import step_oracle as S  # noqa: E402

PLANT = 5e-5
PLANT_CASES = ["23", "64"]          # both have a 9-residue sample next to a longer one


def test_case_table():
    assert list(S.CASES) == ["23", "48-hole", "64", "68", "70", "128", "144", "272"]
    assert S.CASES["23"] == (3, 23, [17, 9, 23], None) and S.CASES["64"] == (3, 64, [64, 41, 9], 7)
    assert S.K_NOISE == 3 and K.REL == 1e-4 and K.FWD_REL == 2e-5
    assert all(v <= K.REL for v in S.REL_OF.values())


@pytest.mark.parametrize("name", list(S.CASES))
def test_truth_reaches_every_region_and_the_fp32_oracle_passes_the_tight_rule(seeded_sd, name):
    """Every region listed for the case holds a real, non-zero element of every float64 tensor; the rows and pairs the launch tail
    names are real where the case is there for them; the oracle's fp32 run passes compare at FWD_REL (and so at REL)."""
    tr = S.truth(seeded_sd, name)
    B, L, lengths, hole = S.CASES[name]
    assert sorted(tr["t64"]) == sorted(S.names()) and (tr["B"], tr["L"]) == (B, L)
    assert int(tr["mask"].sum()) == sum(lengths) - (hole is not None)
    for pair in (False, True):
        listed = [n for n, _ in K.regions(tr["mask"], pair)]
        assert "whole" in listed and all(f"sample {b}" in listed for b in range(B))
        assert all((f"rowband {b}" in listed and f"colband {b}" in listed) if pair else f"tail {b}" in listed for b in range(B))
    if name == "23":                     # 69 rows, 1587 pairs, the last sample full: both launch tails are real
        assert "launch-tail" in [n for n, _ in K.regions(tr["mask"], False)] and "launch-tail" in [n for n, _ in K.regions(tr["mask"], True)]
    for n, t in tr["t64"].items():
        for rname, sel in K.regions(tr["mask"], K.is_pair(t)):
            assert sel.any() and float(t[sel].abs().max()) > 0, (name, n, rname)
    got = {n: (tr["t64"][n] + tr["t32"][n]) if n == S.ANGLE else v for n, v in tr["t32"].items()}
    r = S.compare(tr, got, K.FWD_REL, strict=False)
    w = r["worst"]
    print(f"step oracle {name}: the oracle's fp32 step, worst err/tol {w[0]:.3f} at {w[1]} / {w[2]} (noise {w[4]:.2e}); "
          f"largest noise of any tensor and region {max(row[3] for row in r['rows']):.2e}")
    assert not r["bad"], r["bad"][:6]
    assert not S.compare(tr, got, K.REL, strict=False)["bad"]
    # a tensor the plan does not produce is left out by name; one that is merely forgotten is reported
    del got["z_4"]
    assert [b[:2] for b in S.compare(tr, got, K.FWD_REL, strict=False)["bad"]] == [("z_4", "-")]
    assert not S.compare(tr, got, K.FWD_REL, absent=("z_4",), strict=False)["bad"]


def _shortest(tr, name):
    lengths = S.CASES[name][2]
    b = lengths.index(min(lengths))
    last = int((tr["mask"][b] > 0.5).nonzero().max())
    return b, last


def _exact(tr):
    return {n: v.clone() for n, v in tr["t64"].items()}


def _assert_the_gap(tr, got, tensor, wanted):
    """The planted tensor is reported under the tight rule in every region of `wanted` (and nothing but that tensor is reported),
    and passes the whole-tensor bar every other forward test holds."""
    r = S.compare(tr, got, K.FWD_REL, strict=False)
    hit = {b[1] for b in r["bad"] if b[0] == tensor}
    assert {b[0] for b in r["bad"]} == {tensor} and set(wanted) <= hit, (wanted, r["bad"])
    G.assert_close(got[tensor].float(), tr["t64"][tensor].float(), 1e-4, f"planted {tensor}")
    return hit


@pytest.mark.parametrize("name", PLANT_CASES)
def test_planted_row_fault_in_the_shortest_sample(seeded_sd, name):
    """(a) 5e-5 max|s_3| added to one element of the last real residue of the shortest sample."""
    tr = S.truth(seeded_sd, name)
    b, i = _shortest(tr, name)
    assert tr["mask"][b, i] > 0.5
    got = _exact(tr)
    c = int(tr["t64"]["s_3"][b, i].abs().argmax())
    got["s_3"][b, i, c] += PLANT * tr["t64"]["s_3"].abs().max()
    hit = _assert_the_gap(tr, got, "s_3", [f"sample {b}", f"tail {b}"])
    print(f"planted (a) in {name}: s_3[{b}, {i}, {c}] reported in {sorted(hit)}")


@pytest.mark.parametrize("name", PLANT_CASES)
def test_planted_pair_fault_in_a_row_band(seeded_sd, name):
    """(b) the same added to one pair of z_2 in the last row band of sample 1."""
    tr = S.truth(seeded_sd, name)
    real = (tr["mask"][1] > 0.5).nonzero().reshape(-1)
    i, j = int(real[-1]), int(real[0])
    assert tr["mask"][1, i] > 0.5 and tr["mask"][1, j] > 0.5          # row = the last real residue, column = the first
    got = _exact(tr)
    c = int(tr["t64"]["z_2"][1, i, j].abs().argmax())
    got["z_2"][1, i, j, c] += PLANT * tr["t64"]["z_2"].abs().max()
    wanted = ["rowband 1", "sample 1"]
    hit = _assert_the_gap(tr, got, "z_2", wanted)
    if len(real) > K.TAIL:               # column j = the sample's first residue is outside its last 16: the column band is clean
        assert "colband 1" not in hit
    print(f"planted (b) in {name}: z_2[1, {i}, {j}, {c}] reported in {sorted(hit)}")


@pytest.mark.parametrize("name", PLANT_CASES)
def test_planted_scale_fault_in_the_shortest_sample(seeded_sd, name):
    """(c) x_4 of the shortest sample scaled by 1 + 5e-5."""
    tr = S.truth(seeded_sd, name)
    b, i = _shortest(tr, name)
    assert tr["mask"][b, i] > 0.5
    got = _exact(tr)
    got["x_4"][b] *= 1 + PLANT
    hit = _assert_the_gap(tr, got, "x_4", [f"sample {b}", f"tail {b}"])
    print(f"planted (c) in {name}: x_4[{b}] reported in {sorted(hit)}")


def test_angles_are_compared_across_the_wrap(seeded_sd):
    """An angle just below 2 pi against a truth just above 0 is a small error, half a turn is the largest one."""
    tr = S.truth(seeded_sd, "23")
    got = _exact(tr)
    got[S.ANGLE] = (got[S.ANGLE] - 1e-6) % (2 * torch.pi)
    assert not S.compare(tr, got, K.FWD_REL, strict=False)["bad"]
    got[S.ANGLE] = (tr["t64"][S.ANGLE] + torch.pi) % (2 * torch.pi)
    r = S.compare(tr, got, K.FWD_REL, strict=False)
    assert r["bad"] and abs(r["worst"][3] - 1.0) < 1e-9


def test_masked_rows_must_be_finite(seeded_sd):
    tr = S.truth(seeded_sd, "23")
    got = _exact(tr)
    got["s_0"][0, 20, 3] = float("nan")          # sample 0 has 17 residues
    got["bias_2"][1, 3, 15, 0] = float("inf")    # sample 1 has 9
    bad = S.compare(tr, got, K.FWD_REL, strict=False)["bad"]
    assert [b[:2] for b in bad] == [("s_0", "masked"), ("bias_2", "masked")]
