"""The de novo design entry end to end on a real MI355X: design.find_cavities on a receptor-sized groove, design.make_design_batch
around the cavity it finds, and FlowModel.sample on that batch -- no native peptide anywhere.

The claim the entry rests on: the values in the placeholder peptide rows (coordinates, residue types, torsions) do not reach the
trajectory, because every generated row starts from noise and the embedders mask the generated rows' coordinates and types.  It is held
bit for bit (torch.equal) at every step for rotmats / trans / angles / seqs; only the `*_1` entries, which carry the batch's own
"native" rows, may differ.  The same comparison holds on the CPU oracle (oracle/pepflow_oracle.py): checked once when this test was
written, and again here in test_placeholder_values_do_not_reach_the_oracles_trajectory (no GPU needed for that one's arithmetic, but it
shares this module's batch)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import pepflowww_amd  # noqa: E402
from pepflowww_amd import design, io, synth  # noqa: E402
from oracle import pepflow_oracle as O  # noqa: E402
import cavity_cases as CC  # noqa: E402
import gpu_util as G  # noqa: E402

LENGTH, SAMPLES, NS = 8, 2, 4
STATE = ("rotmats", "trans", "angles", "seqs")


@pytest.fixture(scope="module")
def entry(tmp_path_factory):
    """the receptor goes through a PDB file: what follows starts from a bare receptor structure on disk"""
    built, free = CC.groove_receptor()
    path = str(tmp_path_factory.mktemp("design") / "receptor.pdb")
    io.write_pdb(built, path)
    rec = design.receptor_from_pdb(path)
    assert torch.equal(rec["pos_heavyatom"], built["pos_heavyatom"]) and torch.equal(rec["aa"], built["aa"])
    assert torch.equal(rec["mask_heavyatom"], built["mask_heavyatom"])
    cavities = design.find_cavities(rec)
    batch, info = design.make_design_batch(rec, LENGTH, SAMPLES, cavity=cavities[0])
    noise = synth.make_noise(SAMPLES, batch["aa"].shape[1], NS, seed=3)
    return rec, free, cavities, batch, info, noise


@pytest.fixture(scope="module")
def model(seeded_sd):
    m = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
    m.load_state_dict(seeded_sd)
    return m.to(G.dev()).eval()


def scrambled(batch):
    """the batch with random coordinates, residue types and torsions in the placeholder rows"""
    g = torch.Generator().manual_seed(1)
    out = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}
    gen = out["generate_mask"]
    n = int(gen.sum())
    out["pos_heavyatom"][gen] = torch.randn(n, 15, 3, generator=g) * 10.0
    out["aa"][gen] = torch.randint(0, 20, (n,), generator=g)
    out["torsion_angle"][gen] = torch.rand(n, 5, generator=g) * 6.28
    return out


def test_find_cavities_names_the_groove_first(entry):
    rec, (lo, hi), cavities, _, _, _ = entry
    assert len(cavities) >= 1 and [c["rank"] for c in cavities] == list(range(len(cavities)))
    first = cavities[0]
    c = first["center"].numpy()
    assert (c > lo).all() and (c < hi).all(), c                                         # inside the box
    pts = first["points"].numpy()
    assert pts.shape == (first["size"], 3) and (pts > lo).all() and (pts < hi).all()
    assert np.allclose(pts.mean(0), c, atol=1e-4) and first["volume"] == first["size"] * 1.0 and first["size"] >= 100
    assert 5.0 <= first["mean_buried"] <= 6.0                                           # open on one face: never 7
    assert all(first["size"] >= other["size"] for other in cavities[1:])
    lining = first["lining"]
    assert lining.numel() >= 10 and lining.dtype == torch.int64 and int(lining.max()) < rec["aa"].shape[0]
    atoms = rec["pos_heavyatom"][lining].reshape(-1, 1, 3)
    assert float(torch.cdist(atoms.reshape(-1, 3), first["points"]).min(1).values.reshape(lining.numel(), 15).min(1).values.max()) <= 4.5 + 1e-4


def test_design_batch_around_the_cavity(entry):
    rec, _, cavities, batch, info, _ = entry
    n_ctx = info["context_index"].numel()
    L = batch["aa"].shape[1]
    assert n_ctx >= 10 and L == -(-(n_ctx + LENGTH) // 8) * 8 and batch["aa"].shape == (SAMPLES, L)
    assert int(batch["generate_mask"][0].sum()) == LENGTH and int(batch["res_mask"][0].sum()) == n_ctx + LENGTH
    hot = info["hotspots"]
    assert hot.shape == (L,) and hot.any() and not hot[n_ctx:].any()
    assert set(info["context_index"][hot[:n_ctx]].tolist()) <= set(cavities[0]["lining"].tolist())
    back = design.to_receptor_frame(batch["pos_heavyatom"][0, :n_ctx], info)
    assert torch.allclose(back, rec["pos_heavyatom"][info["context_index"]], atol=1e-5)


def test_placeholder_values_do_not_reach_the_oracles_trajectory(entry, seeded_sd):
    _, _, _, batch, _, noise = entry
    tensors = {k: v for k, v in batch.items() if torch.is_tensor(v)}
    a, b = O.sample(seeded_sd, tensors, noise, NS), O.sample(seeded_sd, scrambled(tensors), noise, NS)
    for i in range(NS):
        for k in STATE:
            assert torch.equal(a[i][k], b[i][k]), (i, k)


def test_sample_runs_without_a_native_and_ignores_the_placeholder_values(entry, model):
    _, _, _, batch, info, noise = entry
    dev = G.dev()
    ctx = ~batch["generate_mask"] & batch["res_mask"]
    a = model.sample(design.batch_to(batch, dev), num_steps=NS, noise=noise)
    assert len(a) == NS
    for i in range(NS):
        for k in STATE:
            assert torch.isfinite(a[i][k].float()).all(), (i, k)
            assert torch.equal(a[i][k][ctx], a[0][k][ctx]), (i, k)                      # the context does not change
    gen = batch["generate_mask"]
    assert not torch.equal(a[-1]["trans"][gen], a[0]["trans"][gen])                    # the peptide does
    a = [{k: v.clone() for k, v in step.items()} for step in a]                         # (the trajectory may view staging buffers)
    b = model.sample(design.batch_to(scrambled(batch), dev), num_steps=NS, noise=noise)
    differs = False
    for i in range(NS):
        for k in STATE:
            assert torch.equal(a[i][k], b[i][k]), (i, k)
            differs |= not torch.equal(a[i][k + "_1"], b[i][k + "_1"])
    assert differs                                                                      # the scrambled values did go in


def test_guided_run_with_the_cavitys_lining_as_hot_spots(entry, model):
    _, _, _, batch, info, noise = entry
    guide = {"hotspots": info["hotspots"], "weights": {"hotspot": 1.0}}
    traj = model.sample(design.batch_to(batch, G.dev()), num_steps=NS, noise=noise, guide=guide)
    rep = model.last_guidance
    k = list(rep["terms"]).index("hotspot")
    assert len(traj) == NS and rep["energy"].shape[:2] == (NS, SAMPLES)
    assert (rep["energy"][0, :, k] > 0).all() and torch.isfinite(rep["energy"]).all()
    assert all(torch.isfinite(traj[-1][key].float()).all() for key in STATE)
