"""GPU checks of the evaluation layer: pf_superpose_fwd (align / batch_align against the reference's recorded outputs F13, Kabsch RMSD
and the pairwise matrix against a numpy float64 oracle) and pf_binding_site_fwd, then evaluate_samples on a short sample() run."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import eval_oracle as EO  # noqa: E402
import pepflowww_amd  # noqa: E402
from pepflowww_amd import geometry, metrics, synth  # noqa: E402


def cu(t):
    return torch.as_tensor(t).cuda()


def _rot(rng):
    q = rng.standard_normal(4)
    a, b, c, d = q / np.linalg.norm(q)
    return np.array([[a*a+b*b-c*c-d*d, 2*(b*c-a*d), 2*(b*d+a*c)], [2*(b*c+a*d), a*a-b*b+c*c-d*d, 2*(c*d-a*b)],
                     [2*(b*d-a*c), 2*(c*d+a*b), a*a-b*b-c*c+d*d]])


@pytest.fixture(scope="module")
def f13(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "f13_align.npz")))


def _close(out, ref, what):
    out, ref = out.detach().cpu().double().numpy(), np.asarray(ref, np.float64)
    err = np.abs(out - ref)
    assert (err <= 1e-4 + 1e-5 * np.abs(ref)).all(), (what, float(err.max()))


def test_align_and_batch_align_match_the_reference(f13):
    for case in ("align", "mirror"):
        p1, p2, m = cu(f13[f"{case}_pos_1"]), cu(f13[f"{case}_pos_2"]), cu(f13[f"{case}_mask"])
        out, same = geometry.align(p1, p2, m)
        assert same is p2 and out.shape == p1.shape
        _close(out, f13[f"{case}_out"], case)
    out, _ = geometry.batch_align(cu(f13["batch_pos_1"]), cu(f13["batch_pos_2"]), cu(f13["batch_mask"]))
    _close(out, f13["batch_out"], "batch")
    # the mirror case went through a reflection: the transform the kernel reports says so
    p1, p2, m = (cu(f13[f"mirror_{k}"]).reshape(1, -1, *f13[f"mirror_{k}"].shape[2:]) for k in ("pos_1", "pos_2", "mask"))
    o = geometry.superpose(p1, p2, m, m, cu(torch.zeros(1, 2, dtype=torch.int32)), allow_reflection=True, transform=True)
    assert float(torch.linalg.det(o["rot"][0].double().cpu())) < -0.999


def _sets(rng, B, N, scale=50.0, noise=1.0):
    x = rng.uniform(-scale, scale, size=(B, N, 3))
    y = np.stack([x[b] @ _rot(rng).T + rng.uniform(-20, 20, 3) + noise * rng.standard_normal((N, 3)) for b in range(B)])
    m = rng.random((B, N)) > 0.25
    return x.astype(np.float32), y.astype(np.float32), m


def test_superpose_rmsd_matches_numpy_kabsch():
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(5)
    x, y, m = _sets(rng, 24, 57)
    ids = torch.arange(24, dtype=torch.int32)
    out = geometry.superpose(cu(x), cu(y), cu(m), cu(m), torch.stack([ids, ids], 1), transform=True)
    rm = geometry.superpose_rmsd(cu(x), cu(y), cu(m))
    assert torch.equal(rm, out["rmsd"])
    for b in range(24):
        k = EO.kabsch(x[b][m[b]], y[b][m[b]])
        assert abs(out["rmsd"][b].item() - k["rmsd"]) < 2e-5, b
        assert abs(out["rmsd_plain"][b].item() - k["rmsd_plain"]) < 2e-5, b
        assert out["count"][b].item() == m[b].sum() and not out["degenerate"][b].item()
        assert np.abs(out["rot"][b].cpu().numpy() - k["r"]).max() < 1e-5
        assert np.abs(out["trans"][b].cpu().numpy() - k["t"]).max() < 1e-3
        # an independent Kabsch: scipy's align_vectors on the centred points
        xs, ys = x[b][m[b]].astype(np.float64), y[b][m[b]].astype(np.float64)
        r, _ = Rotation.align_vectors(ys - ys.mean(0), xs - xs.mean(0))
        rs = float(np.sqrt((((xs - xs.mean(0)) @ r.as_matrix().T - (ys - ys.mean(0))) ** 2).sum(1).mean()))
        assert abs(out["rmsd"][b].item() - rs) < 2e-5, b


def test_superpose_special_cases():
    rng = np.random.default_rng(9)
    x = rng.uniform(-50, 50, size=(1, 40, 3)).astype(np.float32)
    moved = (x[0].astype(np.float64) @ _rot(rng).T + np.array([7.0, -30.0, 12.0])).astype(np.float32)[None]
    mirror = (x[0] * np.array([-1.0, 1.0, 1.0], np.float32))[None]
    line = (np.linspace(-20, 20, 40)[:, None] * np.array([0.6, 0.0, 0.8])).astype(np.float32)[None]
    X = cu(np.concatenate([x, x, x, x, line]))
    Y = cu(np.concatenate([x, moved, mirror, x, line + np.float32(3.0)]))
    M = torch.ones(5, 40, dtype=torch.bool).cuda()
    M[3] = False                                                           # empty mask
    pairs = torch.arange(5, dtype=torch.int32)[:, None].expand(5, 2)
    o = geometry.superpose(X, Y, M, M, pairs, transform=True)
    refl = geometry.superpose(X, Y, M, M, pairs, allow_reflection=True, aligned=True)
    assert o["rmsd"][0].item() <= 1e-5
    assert o["rmsd"][1].item() <= 1e-4
    k = EO.kabsch(x[0], mirror[0])
    assert o["rmsd"][2].item() > 1.0 and abs(o["rmsd"][2].item() - k["rmsd"]) < 2e-5
    res = ((refl["aligned"][2] - Y[2]) ** 2).sum(-1).mean().sqrt().item()
    assert res < 1e-4, res                                                  # reflection allowed: the mirror image is reached
    assert float(torch.linalg.det(o["rot"][2].double().cpu())) > 0.999     # proper mode stays a rotation
    assert o["count"][3].item() == 0 and all(math.isnan(o[k][3].item()) for k in ("rmsd", "rmsd_plain"))
    assert bool(torch.isnan(refl["aligned"][3]).all())
    # collinear points: rank-1 S -> identity + flag, RMSD still exact (a translated copy: 0)
    assert o["degenerate"][4].item() and torch.equal(o["rot"][4].cpu(), torch.eye(3))
    assert o["rmsd"][4].item() < 1e-4 and abs(o["rmsd_plain"][4].item() - 3.0 * math.sqrt(3.0)) < 1e-5


def _peptides(B, seed=21):
    """B peptides of 3 - 25 residues (synthetic pockets), their CA packed at positions 0..len-1 of [B,25,3]"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(3, 26, size=B)
    lens[:2] = (3, 25)
    x = np.zeros((B, 25, 3), np.float32)
    aa = np.zeros((B, 25), np.int64)
    m = np.zeros((B, 25), bool)
    for b in range(B):
        batch = synth.make_pocket_batch(1, 12 + int(lens[b]), int(lens[b]), seed=seed * 100 + b)
        g = batch["generate_mask"][0]
        x[b, :lens[b]] = batch["pos_heavyatom"][0, g, 1].numpy()
        aa[b, :lens[b]] = batch["aa"][0, g].numpy()
        m[b, :lens[b]] = True
    return x, aa, m


def test_pairwise_matrix_properties_at_64_samples():
    B = 64
    x, aa, m = _peptides(B)
    rmsd, ident = geometry.pairwise_superpose_rmsd(cu(x), cu(m), aa=cu(aa))
    R, I = rmsd.cpu().double().numpy(), ident.cpu().double().numpy()
    assert np.array_equal(R, R.T) and np.array_equal(I, I.T)
    assert (np.diag(R) == 0).all() and (np.diag(I) == 1).all()
    for i in range(B):
        for j in range(i + 1, B):
            mm = m[i] & m[j]
            assert abs(R[i, j] - EO.kabsch(x[i][mm], x[j][mm])["rmsd"]) < 2e-5, (i, j)
            assert abs(I[i, j] - (aa[i][mm] == aa[j][mm]).mean()) < 1e-6, (i, j)
    perm = torch.from_numpy(np.random.default_rng(2).permutation(B))
    rp = geometry.pairwise_superpose_rmsd(cu(x[perm.numpy()]), cu(m[perm.numpy()])).cpu().double().numpy()
    assert np.abs(rp - R[np.ix_(perm.numpy(), perm.numpy())]).max() <= 1e-6
    # two groups of unequal size: same values inside a group, NaN across
    groups = torch.from_numpy(np.random.default_rng(4).permutation(np.r_[np.zeros(40), np.ones(24)]).astype(np.int64))
    rg = geometry.pairwise_superpose_rmsd(cu(x), cu(m), groups=groups).cpu().double().numpy()
    same = (groups[:, None] == groups[None, :]).numpy()
    assert np.isnan(rg[~same]).all() and not np.isnan(rg[same]).any()
    assert np.abs(rg[same] - R[same]).max() <= 1e-6 and np.array_equal(rg, rg.T, equal_nan=True) and (np.diag(rg) == 0).all()


def test_binding_site_ratio_matches_brute_force():
    B, L = 8, 128
    batch = synth.make_pocket_batch(B, L, 14, seed=31, lengths=[128, 128, 120, 100, 128, 90, 128, 64])
    rng = np.random.default_rng(8)
    native = batch["pos_heavyatom"][:, :, 1].clone()
    sample = native + torch.from_numpy(rng.normal(scale=3.0, size=native.shape).astype(np.float32))
    ca_mask = batch["mask_heavyatom"].clone()
    ca_mask[0, :20, 1] = False                                              # context residues without a CA
    s_site, n_site, bsr = metrics.binding_site(cu(batch["pos_heavyatom"]), cu(ca_mask), cu(batch["res_mask"]),
                                               cu(batch["generate_mask"]), cu(sample), cu(native))
    checked = sites = 0
    for b in range(B):
        args = (batch["pos_heavyatom"][b, :, 1].numpy(), ca_mask[b, :, 1].numpy(), batch["res_mask"][b].numpy(),
                batch["generate_mask"][b].numpy())
        ss, ms = EO.binding_sites(*args, sample[b].numpy())
        sn, mn = EO.binding_sites(*args, native[b].numpy())
        if min(ms, mn) < 1e-4:                                              # a tie at the cutoff: either answer is right
            continue
        checked += 1
        assert np.array_equal(s_site[b].cpu().numpy(), ss) and np.array_equal(n_site[b].cpu().numpy(), sn), b
        sites += int(sn.sum())
        assert abs(bsr[b].item() - (ss & sn).sum() / (sn.sum() + 1e-10)) < 1e-6, b
    assert checked >= 6 and sites > 0


@pytest.fixture(scope="module")
def model(seeded_sd):
    m = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
    m.load_state_dict(seeded_sd)
    return m.cuda().eval()


def test_evaluate_samples_after_sample(model):
    B, L, NS = 4, 24, 3
    batch = synth.make_pocket_batch(B, L, 6, seed=41)
    noise = synth.make_noise(B, L, NS, seed=42)
    dev_batch = {k: cu(v) for k, v in batch.items()}
    final = model.sample(dev_batch, num_steps=NS, noise=noise)[-1]
    gm = batch["generate_mask"]
    ev = metrics.evaluate_samples(final, dev_batch)
    # pooled: the three lines of the reference's sampling driver, restated on CPU in float32
    den = gm.sum() + 1e-8
    ca_ref = torch.sqrt(torch.sum((final["trans"] - final["trans_1"]) ** 2 * gm[..., None].long()) / den)
    rot_ref = torch.sqrt(torch.sum((final["rotmats"] - final["rotmats_1"]) ** 2 * gm[..., None, None].long()) / den)
    aar_ref = torch.sum((final["seqs"] == final["seqs_1"]) * gm.long()) / (gm.sum() + 1e-8)
    for k, ref in (("ca_rmsd_pooled", ca_ref), ("rot_rmsd_pooled", rot_ref), ("aar_pooled", aar_ref)):
        v = ev[k].item()
        assert abs(v - ref.item()) <= 1e-6 * abs(ref.item()) + 1e-12, (k, v, ref.item())
    # per sample: the numpy oracle
    for b in range(B):
        g = gm[b].numpy()
        x, y = final["trans"][b].numpy()[g], final["trans_1"][b].numpy()[g]
        k = EO.kabsch(x, y)
        assert abs(ev["ca_rmsd"][b].item() - k["rmsd_plain"]) < 2e-5
        assert abs(ev["ca_rmsd_aligned"][b].item() - k["rmsd"]) < 2e-5
        dr = (final["rotmats"][b].double() - final["rotmats_1"][b].double()).numpy()[g]
        assert abs(ev["rot_rmsd"][b].item() - math.sqrt((dr ** 2).sum() / g.sum())) < 2e-5
        assert abs(ev["aar"][b].item() - (final["seqs"][b].numpy()[g] == final["seqs_1"][b].numpy()[g]).mean()) < 1e-6
        args = (batch["pos_heavyatom"][b, :, 1].numpy(), batch["mask_heavyatom"][b, :, 1].numpy(), batch["res_mask"][b].numpy(), g)
        ss, _ = EO.binding_sites(*args, final["trans"][b].numpy())
        sn, _ = EO.binding_sites(*args, final["trans_1"][b].numpy())
        assert abs(ev["bsr"][b].item() - (ss & sn).sum() / (sn.sum() + 1e-10)) < 1e-6
    # diversity: one group, then two
    x = final["trans"].numpy()
    s = final["seqs"].numpy()
    g = gm[0].numpy()
    for groups, members in ((None, [list(range(B))]), (torch.tensor([5, 5, 2, 2]), [[2, 3], [0, 1]])):
        ev = metrics.evaluate_samples(final, dev_batch, groups=groups)
        assert ev["diversity_rmsd"].shape == (len(members),)
        for gi, mem in enumerate(members):
            pr = [(i, j) for i in mem for j in mem if i < j]
            dr = np.mean([EO.kabsch(x[i][g], x[j][g])["rmsd"] for i, j in pr])
            ds = 1.0 - np.mean([(s[i][g] == s[j][g]).mean() for i, j in pr])
            assert abs(ev["diversity_rmsd"][gi].item() - dr) < 2e-5 and abs(ev["diversity_seq"][gi].item() - ds) < 1e-6
