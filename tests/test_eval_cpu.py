"""CPU checks of the evaluation layer (pepflowww_amd.geometry / metrics): the test's numpy float64 oracle against the reference's recorded
`align` / `batch_align` (F13), the pair-list builder, and the argument checks that run before any device work."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import eval_oracle as EO  # noqa: E402
from pepflowww_amd import _capi, geometry, metrics, synth  # noqa: E402


@pytest.fixture(scope="module")
def f13(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "f13_align.npz")))


def _tol(x):
    return 1e-4 + 1e-5 * np.abs(x)


def test_oracle_reproduces_reference_align(f13):
    for case in ("align", "mirror"):
        out = EO.batch_align(f13[f"{case}_pos_1"][None], f13[f"{case}_pos_2"][None], f13[f"{case}_mask"][None])[0]
        ref = f13[f"{case}_out"]
        assert (np.abs(out - ref) <= _tol(ref)).all(), (case, np.abs(out - ref).max())
    out = EO.batch_align(f13["batch_pos_1"], f13["batch_pos_2"], f13["batch_mask"])
    assert (np.abs(out - f13["batch_out"]) <= _tol(f13["batch_out"])).all(), np.abs(out - f13["batch_out"]).max()
    # the fixture covers what it claims: masked atoms, equal per-sample counts, a reflection, +-50 A
    assert not f13["align_mask"].all() and len(set(f13["batch_mask"].reshape(5, -1).sum(1).tolist())) == 1
    assert f13["mirror_det"] < -0.99 and np.abs(f13["align_pos_1"]).max() > 45


def test_oracle_proper_and_reflected_residuals():
    rng = np.random.default_rng(3)
    x = rng.uniform(-20, 20, size=(30, 3))
    mirror = x * np.array([-1.0, 1.0, 1.0])
    k = EO.kabsch(x, mirror)
    assert k["rmsd_refl"] < 1e-9 < 1.0 < k["rmsd"] and np.linalg.det(k["r"]) > 0 > np.linalg.det(k["r_refl"])


def test_group_pairs():
    pairs, gidx, labels = geometry.group_pairs(torch.tensor([7, 3, 7, 7, 3, 9]))
    assert labels.tolist() == [3, 7, 9]
    assert pairs.dtype == torch.int32
    assert sorted(map(tuple, pairs.tolist())) == [(0, 2), (0, 3), (1, 4), (2, 3)]
    assert {tuple(p): int(g) for p, g in zip(pairs.tolist(), gidx)} == {(0, 2): 1, (0, 3): 1, (2, 3): 1, (1, 4): 0}
    pairs, gidx, labels = geometry.group_pairs(torch.zeros(64, dtype=torch.int64))
    assert pairs.shape == (2016, 2) and bool((pairs[:, 0] < pairs[:, 1]).all()) and labels.tolist() == [0]
    assert len(set(map(tuple, pairs.tolist()))) == 2016


def _final_and_batch(lengths, L=24, n_gen=6):
    B = len(lengths)
    batch = synth.make_pocket_batch(B, L, n_gen, seed=11, lengths=lengths)
    ca = batch["pos_heavyatom"][:, :, 1]
    final = {"rotmats": torch.eye(3).expand(B, L, 3, 3), "trans": ca, "seqs": batch["aa"], "rotmats_1": torch.eye(3).expand(B, L, 3, 3),
             "trans_1": ca, "seqs_1": batch["aa"]}
    return final, batch


def test_one_group_needs_equal_generate_masks():
    final, batch = _final_and_batch([24, 20, 24])          # padding moves the generated block of the second sample
    assert not bool((batch["generate_mask"] == batch["generate_mask"][0]).all())
    with pytest.raises(ValueError):
        metrics.evaluate_samples(final, batch)
    with pytest.raises(ValueError):                       # the same within a group
        metrics.evaluate_samples(final, batch, groups=torch.tensor([0, 0, 1]))
    with pytest.raises(ValueError):
        metrics.evaluate_samples(final, batch, groups=torch.tensor([0, 1]))


def test_superpose_rejects_bad_arguments_before_device_work():
    """the cases tm_score has in test_tm_cpu.py: superpose goes through the same pair-work-list checks"""
    x = torch.zeros(4, 10, 3)
    m = torch.ones(4, 10, dtype=torch.bool)
    aa = torch.zeros(4, 10, dtype=torch.long)
    pairs = torch.tensor([[0, 1]], dtype=torch.int32)
    with pytest.raises(ValueError):
        geometry.superpose(torch.zeros(4, 10), x, m, m, pairs)                         # a 2-D x
    with pytest.raises(ValueError):
        geometry.superpose(x, torch.zeros(4, 9, 3), m, m, pairs)                       # y of another N
    with pytest.raises(ValueError):
        geometry.superpose(x, torch.zeros(4, 10), m, m, pairs)                         # a 2-D y
    with pytest.raises(ValueError):
        geometry.superpose(x, x, m[:, :9], m, pairs)                                   # mx
    with pytest.raises(ValueError):
        geometry.superpose(x, x, m, m[:3], pairs)                                      # my
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)):
        with pytest.raises(ValueError):
            geometry.superpose(x, x, m, m, bad)                                        # pairs that is not [P,2]
    with pytest.raises(ValueError):
        geometry.superpose(x, x, m, m, pairs, aa_x=aa)                                 # exactly one of aa_x / aa_y
    with pytest.raises(ValueError):
        geometry.superpose(x, x, m, m, pairs, aa_y=aa)
    with pytest.raises(_capi.PepflowHipError):                                         # valid shapes on the CPU: no fallback
        geometry.superpose(x, x, m, m, pairs)
