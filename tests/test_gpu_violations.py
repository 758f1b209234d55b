"""GPU checks of the structural violations: pf_violations_fwd (through geometry.structural_violations) against the fixture recorded
from the reference's OpenFold functions (golden F14) and against the numpy float64 oracle (violation_oracle.py) on seeded shapes
from 1 to 512 residues, with and without `query` / `group`; repeatability and independence of the batch; peak memory; constructed
cases with known answers; metrics.structural_violations after a short sample() run.

Bounds (derived, not tuned).  Floats: per value 8 * 2^-23 * max|coord| * (nonzero terms + 1) absolute plus 1e-6 relative -- the
kernel's clash pass is fp32: a distance carries a few ulp of the largest coordinate, and a sum of k such terms k times that; twice
that against the fixture, whose own values are fp32.  Flags: a flag whose float64 margin is below 8 * 2^-23 * max|coord| may differ,
at most 0.5 % of a case's flags, and none in the fixture (its margins are >= 1e-3)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import dssp_build as DB  # noqa: E402
import violation_oracle as VO  # noqa: E402
import pepflowww_amd  # noqa: E402
from pepflowww_amd import full_atom, geometry, metrics, synth  # noqa: E402
from pepflowww_amd.preprocess import residue_type  # noqa: E402

PRO = residue_type("PRO")
ULP8 = 8.0 * 2.0 ** -23
RADIUS = geometry.vdw_radius_table().numpy()

FLOATS = [("clash_atom_loss", "clash_atom_terms"), ("clash_mean_loss", "clash_mean_terms"), ("bond_c_n_loss_mean", "bond_c_n_terms"),
          ("angle_ca_c_n_loss_mean", "angle_ca_c_n_terms"), ("angle_c_n_ca_loss_mean", "angle_c_n_ca_terms"),
          ("connection_loss", "connection_terms"), ("clash_atom_loss_cross", "clash_atom_terms_cross")]
FLAGS = [("clash_atom", "clash_atom_margin"), ("connection_violation", "connection_margin"), ("ca_ca_break", "ca_ca_margin"),
         ("clash_atom_cross", "clash_atom_margin_cross")]


def cu(t):
    return None if t is None else torch.as_tensor(t).cuda()


def run(pos, mask, aa, index, query=None, group=None, **kw):
    out = geometry.structural_violations(cu(pos), cu(mask), cu(aa), cu(index), query=cu(query), group=cu(group), **kw)
    torch.cuda.synchronize()
    return out


def float_bound(max_coord, terms, value, factor=1.0):
    return factor * (ULP8 * max_coord * (np.asarray(terms) + 1) + 1e-6 * np.abs(value))


def make_batch(rng, B, N, scale):
    """B structures of N residues with coordinates within +-scale: NeRF backbone segments of up to 30 residues placed at random (so
    bonded neighbours, gaps and chain starts all occur), some samples with noisy atoms; side-chain atoms 1.5 - 4 A from CA; masks
    with holes; residue types 0..20; indices growing by 1 inside a segment, by 2 - 5 between segments, restarting in some samples;
    the last sample all masked.  -> pos [B,N,15,3] fp32, mask [B,N,15], aa [B,N], index [B,N] int32"""
    pos = np.zeros((B, N, 15, 3))
    index = np.zeros((B, N), np.int64)
    for b in range(B):
        k, cur = 0, int(rng.integers(-5, 50))
        while k < N:
            n = int(min(N - k, rng.integers(1, 31)))
            seg = DB.random_chain(rng, n) @ DB.rotation(rng.standard_normal(3) * 2.0).T
            room = max(scale - 4.0 - np.abs(seg - seg.mean((0, 1))).max(), 0.0)
            if room == 0.0:
                seg = seg * (scale - 4.0) / np.abs(seg - seg.mean((0, 1))).max()
            seg = seg - seg.mean((0, 1)) + rng.uniform(-room, room, 3)
            pos[b, k:k + n, :4] = seg
            index[b, k:k + n] = cur + np.arange(n)
            cur += n - 1 + int(rng.integers(2, 6))
            k += n
        if b % 4 == 1 and N > 3:
            index[b, N // 2:] -= index[b, N // 2] - index[b, 0]              # a second chain numbered like the first
        d = rng.standard_normal((N, 11, 3))
        pos[b, :, 4:] = pos[b, :, 1:2] + d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(1.5, 4.0, (N, 11, 1))
        if b % 3 == 2:
            pos[b] += rng.standard_normal(pos[b].shape) * (0.05 if b % 2 else 0.5)
    pos = np.clip(pos, -scale, scale).astype(np.float32)
    aa = rng.integers(0, 21, size=(B, N))
    aa[rng.random((B, N)) < 0.08] = PRO
    mask = (rng.random((B, N, 15)) > 0.1) & (rng.random((B, N, 1)) > 0.08)
    mask[B - 1] = False
    return pos, mask, aa.astype(np.int64), index.astype(np.int32)


def check_against_oracle(out, pos, mask, aa, index, query=None, group=None, budget=0.005):
    got = {k: v.cpu().numpy() for k, v in out.items()}
    B = pos.shape[0]
    n_flags = excused = 0
    for b in range(B):
        o = VO.violations(pos[b], mask[b], aa[b], index[b], RADIUS, PRO, None if query is None else query[b],
                          None if group is None else group[b])
        mc = float(np.abs(pos[b, :, :14]).max())
        assert np.array_equal(got["clash_atom_pairs"][b], o["clash_atom_pairs"]), b
        for key, terms in FLOATS:
            if key in o:
                err = np.abs(got[key][b].astype(np.float64) - o[key])
                assert (err <= float_bound(mc, o[terms], o[key])).all(), (b, key, float(np.max(err)))
        n_br = o["ca_ca_break"].sum()
        assert abs(float(got["ca_ca_extreme"][b]) - o["ca_ca_extreme"]) <= float_bound(mc, n_br, o["ca_ca_extreme"]), b
        for key, margin in FLAGS:
            if key in o:
                diff = got[key][b] != o[key]
                assert not (diff & (o[margin] >= ULP8 * mc)).any(), (b, key, np.argwhere(diff)[:4])
                excused += int(diff.sum())
                n_flags += diff.size
    assert excused <= budget * n_flags, (excused, n_flags)
    return excused


# ---- the fixture recorded from the reference ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "f14_violations.npz")))


REF = [("clash_atom_loss", "ref_clash_per_atom_loss_sum", "clash_atom_terms"), ("clash_mean_loss", "ref_clash_mean_loss", "clash_mean_terms"),
       ("bond_c_n_loss_mean", "ref_bond_c_n_loss_mean", "bond_c_n_terms"), ("angle_ca_c_n_loss_mean", "ref_bond_ca_c_n_loss_mean", "angle_ca_c_n_terms"),
       ("angle_c_n_ca_loss_mean", "ref_bond_c_n_ca_loss_mean", "angle_c_n_ca_terms"),
       ("connection_loss", "ref_bond_per_residue_loss_sum", "connection_terms")]


def test_kernel_matches_the_reference_fixture(gold):
    pos, mask, aa, index = gold["pos"], gold["atom_mask"], gold["aa"], gold["residue_index"]
    out = run(pos, mask, aa, index, violation_tolerance_factor=float(gold["violation_tolerance_factor"]),
              clash_overlap_tolerance=float(gold["clash_overlap_tolerance"]))
    assert out["clash_atom_loss"].dtype == torch.float32 and out["clash_atom"].dtype == torch.bool
    assert out["clash_atom_pairs"].dtype == torch.int32 and out["clash_atom"].shape == (7, 52, 14)
    assert "clash_atom_cross" not in out
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.array_equal(got["clash_atom"], gold["ref_clash_per_atom_clash_mask"] > 0)
    assert np.array_equal(got["connection_violation"], gold["ref_bond_per_residue_violation_mask"] > 0)
    assert np.array_equal(got["ca_ca_break"], gold["ca_ca_break"])
    for s in range(pos.shape[0]):
        o = VO.violations(pos[s], mask[s], aa[s], index[s], gold["radius"], int(gold["pro"]))
        mc = float(np.abs(pos[s]).max())
        for key, ref, terms in REF:
            err = np.abs(got[key][s].astype(np.float64) - gold[ref][s])
            assert (err <= float_bound(mc, o[terms], o[key], 2.0)).all(), (s, key, float(np.max(err)))
        assert abs(float(got["ca_ca_extreme"][s]) - float(gold["ref_extreme_ca_ca"][s])) <= float_bound(mc, o["ca_ca_break"].sum(), o["ca_ca_extreme"], 2.0)
    check_against_oracle(out, pos, mask, aa, index, budget=0.0)
    # 15-slot inputs (pos_heavyatom's layout) give the same bits
    pos15 = np.concatenate([pos, np.full((7, 52, 1, 3), 3.0, np.float32)], 2)
    mask15 = np.concatenate([mask, np.ones((7, 52, 1), bool)], 2)
    out15 = run(pos15, mask15, aa, index)
    for k in out:
        assert torch.equal(out[k], out15[k]), k


# ---- the float64 oracle on seeded shapes -------------------------------------------------------------------------------------------

SHAPES = {1: (64, 10.0), 2: (8, 5.0), 15: (8, 20.0), 16: (8, 30.0), 17: (8, 60.0), 52: (64, 25.0), 144: (8, 40.0), 256: (4, 60.0), 512: (4, 60.0)}


@pytest.mark.parametrize("N", sorted(SHAPES))
def test_kernel_matches_oracle(N):
    B, scale = SHAPES[N]
    rng = np.random.default_rng(3000 + N)
    pos, mask, aa, index = make_batch(rng, B, N, scale)
    assert np.abs(pos).max() <= scale
    query = rng.random((B, N)) < 0.25
    query[0] = False                                    # no query residue: nothing is evaluated
    if B > 2:
        query[1] = True
        query[2, :] = np.arange(N) >= N - 1             # a single query residue, in the last tile
    group = rng.random((B, N)) < 0.4
    modes = ((None, None), (query, group), (query, None), (None, group))
    for q, g in modes[:2] if N >= 256 else modes:          # (the oracle takes seconds per sample there)
        out = run(pos, mask, aa, index, q, g)
        check_against_oracle(out, pos, mask, aa, index, q, g)
        for k, v in out.items():                        # the all-masked sample (connection_loss is not masked, as the reference's)
            assert k == "connection_loss" or not v[-1].any(), k
        if q is not None:
            assert not out["clash_atom_pairs"][0].any() and out["clash_mean_loss"][0] == 0


def test_other_tolerances():
    rng = np.random.default_rng(31)
    pos, mask, aa, index = make_batch(rng, 6, 40, 20.0)
    out = run(pos, mask, aa, index, violation_tolerance_factor=4.0, clash_overlap_tolerance=0.5)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for b in range(6):
        o = VO.violations(pos[b], mask[b], aa[b], index[b], RADIUS, PRO, tol_factor=4.0, clash_tol=0.5)
        mc = float(np.abs(pos[b]).max())
        for key, margin in FLAGS[:3]:
            assert not ((got[key][b] != o[key]) & (o[margin] >= ULP8 * mc)).any(), (b, key)
        for key, terms in FLOATS[:6]:
            assert (np.abs(got[key][b] - o[key]) <= float_bound(mc, o[terms], o[key])).all(), (b, key)


# ---- repeatability -----------------------------------------------------------------------------------------------------------------

def _bits(out):
    return {k: (v.view(torch.int32) if v.dtype == torch.float32 else v).cpu() for k, v in out.items()}


def test_deterministic_and_independent_of_the_batch():
    rng = np.random.default_rng(41)
    B, N = 12, 100
    pos, mask, aa, index = make_batch(rng, B, N, 30.0)
    query, group = rng.random((B, N)) < 0.3, rng.random((B, N)) < 0.4
    for q, g in ((None, None), (query, group)):
        sub = lambda rows: _bits(run(pos[rows], mask[rows], aa[rows], index[rows], None if q is None else q[rows],  # noqa: E731
                                     None if g is None else g[rows]))
        full = np.arange(B)
        a = sub(full)
        for _ in range(3):
            b = sub(full)
            for k in a:
                assert torch.equal(a[k], b[k]), k
        for rows in (full[4:5], full[:5], full[5:], np.array([7, 2, 9])):
            part = sub(rows)
            for k in a:
                assert torch.equal(part[k], a[k][torch.from_numpy(rows)]), k


def test_peak_memory_is_not_pair_sized():
    """B = 64, L = 144: 2.6e8 atom pairs; the dense form's [B,L,L,14,14] tensors are 1 GB each.  The call may hold 32 MB beyond its
    inputs and outputs."""
    rng = np.random.default_rng(43)
    B, N = 64, 144
    pos, mask, aa, index = make_batch(rng, 4, N, 40.0)
    rep = lambda x: cu(np.concatenate([x] * (B // 4)))  # noqa: E731
    P, M, A, I = rep(pos), rep(mask).to(torch.uint8), rep(aa), rep(index)
    Q, G = rep(rng.random((4, N)) < 0.1), rep(rng.random((4, N)) < 0.1)
    for q, g in ((None, None), (Q, G)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = geometry.structural_violations(P, M, A, I, query=q, group=g)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        out_bytes = sum(v.numel() * v.element_size() for v in out.values())
        assert peak - base - out_bytes <= 32 * 2 ** 20, (peak - base, out_bytes)
        del out


# ---- constructed answers -----------------------------------------------------------------------------------------------------------

def backbone_only(bb):
    n = len(bb)
    pos = np.zeros((1, n, 14, 3), np.float32)
    pos[0, :, :4] = bb
    mask = np.zeros((1, n, 14), bool)
    mask[0, :, :4] = True
    return pos, mask, np.zeros((1, n), np.int64), np.arange(n, dtype=np.int32)[None]


def test_ideal_chain_has_no_bond_violation():
    # dssp_build's chain: C-N 1.329 A, CA-C-N 116.2 (cos -0.4415 against -0.4473 +- 0.168), C-N-CA 121.7 (cos -0.5255 against -0.5203
    # +- 0.4236), CA-CA 3.80 in trans: every term is inside its tolerance, so every loss is 0
    for angles in (DB.ALPHA, DB.STRAND):
        out = run(*backbone_only(DB.helix(24, angles)))
        assert not out["connection_violation"].any() and not out["ca_ca_break"].any()
        assert float(out["connection_loss"].abs().max()) == 0.0 and float(out["ca_ca_extreme"]) == 0.0
        assert float(out["bond_c_n_loss_mean"]) == 0.0 and float(out["angle_ca_c_n_loss_mean"]) == 0.0


def test_one_shifted_residue_flags_its_two_connections():
    # residue k moved by 1 A at right angles to both of its peptide bonds: each C-N length becomes sqrt(1.329^2 + 1) = 1.663 A, 0.334
    # off, beyond 12 x 0.014 = 0.168; the connections (k-1, k) and (k, k+1) mark residues k-1, k, k+1 and no other.  No CA moves by
    # more than 1 A, so no CA-CA distance passes 3.80 + 1.5.
    bb = DB.helix(24, DB.STRAND)
    k = 11
    b1, b2 = bb[k, 0] - bb[k - 1, 2], bb[k + 1, 0] - bb[k, 2]
    v = np.cross(b1, b2)
    bb[k] += v / np.linalg.norm(v)
    pos, mask, aa, index = backbone_only(bb)
    out = run(pos, mask, aa, index)
    assert out["connection_violation"][0].nonzero().flatten().tolist() == [k - 1, k, k + 1]
    assert not out["ca_ca_break"].any()
    loss = out["connection_loss"][0].cpu()
    assert (loss[[k - 1, k, k + 1]] > 0).all() and loss[k] > loss[k - 1] and float(loss[:k - 1].abs().max()) == 0.0
    # a gap in the numbering at k: the connection (k-1, k) is no longer tested
    index[0, k:] += 1
    out = run(pos, mask, aa, index)
    assert out["connection_violation"][0].nonzero().flatten().tolist() == [k, k + 1]
    # 2 A along CA(k) -> CA(k+1) from there on: that CA-CA distance is 5.8 > 5.3
    bb2 = DB.helix(24, DB.STRAND)
    d = bb2[k + 1, 1] - bb2[k, 1]
    bb2[k + 1:] += 2.0 * d / np.linalg.norm(d)
    out = run(*backbone_only(bb2))
    assert out["ca_ca_break"][0].nonzero().flatten().tolist() == [k]
    assert abs(float(out["ca_ca_extreme"]) - 1.0 / (1e-4 + 23)) < 1e-7


def test_two_atoms_one_angstrom_apart_flag_each_other():
    # two CA (carbon, 1.7 A) of residues 0 and 5, 1 A apart, nothing else: bound 1.7 + 1.7 - 1.5 = 1.9, overlap 0.9
    pos = np.zeros((1, 8, 14, 3), np.float32)
    mask = np.zeros((1, 8, 14), bool)
    pos[0, 0, 1] = [3.0, 4.0, 5.0]
    pos[0, 5, 1] = [3.0, 4.0, 6.0]
    mask[0, [0, 5], 1] = True
    aa, index = np.zeros((1, 8), np.int64), np.arange(8, dtype=np.int32)[None] * 3
    out = run(pos, mask, aa, index)
    assert out["clash_atom"][0].nonzero().tolist() == [[0, 1], [5, 1]]
    assert out["clash_atom_pairs"][0].sum() == 2
    assert torch.allclose(out["clash_atom_loss"][0, [0, 5], 1].cpu(), torch.tensor([0.9, 0.9]), atol=1e-6)
    assert abs(float(out["clash_mean_loss"]) - 0.9 / (1.0 + 1e-6)) < 1e-6
    # the same index on both residues: never compared;  slot 5 against slot 5: never compared
    same = index.copy()
    same[0, 5] = same[0, 0]
    assert not run(pos, mask, aa, same)["clash_atom"].any()
    pos5, mask5 = np.roll(pos, 4, axis=2), np.roll(mask, 4, axis=2)
    aa5 = np.full((1, 8), residue_type("LEU"), np.int64)
    assert mask5[0, 0, 5] and not run(pos5, mask5, aa5, index)["clash_atom"].any()
    # C of index r against N of index r + 1: the peptide bond, not a clash; against N of index r + 2 it is one
    posb, maskb = np.zeros_like(pos), np.zeros_like(mask)
    posb[0, 0, 2], posb[0, 1, 0] = [0.0, 0.0, 0.0], [1.329, 0.0, 0.0]
    maskb[0, 0, 2] = maskb[0, 1, 0] = True
    near = np.arange(8, dtype=np.int32)[None]
    assert not run(posb, maskb, aa, near)["clash_atom"].any()
    assert run(posb, maskb, aa, near * 2)["clash_atom"][0].nonzero().tolist() == [[0, 2], [1, 0]]


def test_peptide_pushed_into_the_receptor(gold):
    # the clean complex of the fixture (row 0), its peptide (residues 40..51) translated twice: 150 A away, where no receptor atom is
    # within reach, so no peptide atom has a receptor partner; and so that CA of peptide residue 45 sits 1 A from CA of receptor
    # residue 20 (two carbons: bound 1.7 + 1.7 - 1.5 = 1.9 A), so at least that atom has one.  A translation changes no distance
    # inside the peptide, so the peptide evaluated on its own (what metrics reports as clash_internal) keeps its flags.
    pos, mask, aa, index = (np.stack([gold[k][0]] * 2) for k in ("pos", "atom_mask", "aa", "residue_index"))
    assert mask[0, 45, 1] and mask[0, 20, 1]
    pos[0, 40:] += np.array([150.0, 0.0, 0.0], np.float32)
    pos[1, 40:] += pos[1, 20, 1] + np.array([1.0, 0.0, 0.0], np.float32) - pos[1, 45, 1]
    pep = np.zeros((2, 52), bool)
    pep[:, 40:] = True
    out = run(pos, mask, aa, index, query=pep, group=pep)
    receptor = out["clash_atom_cross"][:, 40:].any(-1).sum(1)                # peptide residues with a receptor partner
    assert receptor[0] == 0 and receptor[1] >= 1 and out["clash_atom_cross"][1, 45, 1] and out["clash_atom_cross"][1, 20, 1]
    assert float(out["clash_atom_loss_cross"][0].abs().max()) == 0.0 and float(out["clash_atom_loss_cross"][1, 45, 1]) >= 0.9 - 1e-4
    alone = run(pos, mask & pep[:, :, None], aa, index)
    assert torch.equal(alone["clash_atom"][0], alone["clash_atom"][1])
    assert torch.allclose(alone["clash_atom_loss"][0], alone["clash_atom_loss"][1], atol=1e-4)
    assert not alone["clash_atom"][:, :40].any()


# ---- metrics.structural_violations -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(seeded_sd):
    m = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
    m.load_state_dict(seeded_sd)
    return m.cuda().eval()


PER_SAMPLE = ("bond_violation", "ca_ca_break", "clash", "clash_receptor", "clash_internal", "violation", "valid", "n_clashing_atoms")


def test_structural_violations_after_sample(model):
    B, L, NS = 4, 40, 3
    batch = synth.make_pocket_batch(B, L, 12, seed=61)
    noise = synth.make_noise(B, L, NS, seed=62)
    dev_batch = {k: cu(v) for k, v in batch.items()}
    final = model.sample(dev_batch, num_steps=NS, noise=noise)[-1]
    gen = (dev_batch["generate_mask"].bool() & dev_batch["res_mask"].bool())
    n = gen.sum(1).double()
    index = metrics.residue_index(dev_batch["chain_nb"], dev_batch["res_nb"], dev_batch["res_mask"])
    mask_n = dev_batch["mask_heavyatom"].bool() & dev_batch["res_mask"].bool()[:, :, None]
    for scope in ("generated", "all"):
        q = gen if scope == "generated" else None
        nat = geometry.structural_violations(dev_batch["pos_heavyatom"], mask_n, cu(final["seqs_1"]), index, query=q, group=gen)
        for backbone in ("full_atom", "frames"):
            out = metrics.structural_violations(final, dev_batch, backbone=backbone, scope=scope)
            for tag in ("", "_native"):
                for k in PER_SAMPLE:
                    assert out[k + tag].shape == (B,), k + tag
                assert out["valid" + tag].dtype == torch.bool and out["valid_fraction" + tag].dtype == torch.float64
                assert out["atom_clash" + tag].shape == (B, L, 14) and out["residue_clash" + tag].shape == (B, L)
                for k in ("bond_violation", "ca_ca_break", "clash", "clash_receptor", "clash_internal", "violation"):
                    v = out[k + tag]
                    assert ((v >= 0) & (v <= 1)).all(), k + tag
                assert (out["violation" + tag] >= torch.maximum(out["bond_violation" + tag], out["clash" + tag])).all()
                assert (out["clash" + tag] >= torch.maximum(out["clash_receptor" + tag], out["clash_internal" + tag])).all()
                assert abs(float(out["valid_fraction" + tag]) - float(out["valid" + tag].double().mean())) <= 1e-12
            assert torch.equal(out["residue_index"], index)
            # the native's values are those of a direct call on the native
            assert torch.equal(out["atom_clash_native"], nat["clash_atom"]) and torch.equal(out["atom_clash_loss_native"], nat["clash_atom_loss"])
            assert torch.equal(out["residue_bond_violation_native"], nat["connection_violation"])
            assert torch.equal(out["atom_clash_receptor_native"], nat["clash_atom_cross"])
            assert torch.equal(out["bond_violation_native"], (nat["connection_violation"] & gen).sum(1).double() / n)
            assert torch.equal(out["clash_native"], (nat["clash_atom"].any(-1) & gen).sum(1).double() / n)
            assert torch.equal(out["n_clashing_atoms_native"], (nat["clash_atom"] & gen[:, :, None]).sum((1, 2)))
            # the sample's: a direct call on the rebuilt complex
            if backbone == "full_atom":
                pos_s, mask_s = full_atom.reconstruct_sample(cu(final["rotmats"]), cu(final["trans"]), cu(final["angles"]), cu(final["seqs"]),
                                                             gen, dev_batch["pos_heavyatom"])
                mask_s = torch.where(gen[:, :, None], mask_s, dev_batch["mask_heavyatom"].bool())
            else:
                pos_s, mask_s = full_atom.reconstruct_sample_bb(cu(final["rotmats"]), cu(final["trans"]), cu(final["seqs"]),
                                                                dev_batch["chain_nb"], dev_batch["res_nb"], dev_batch["res_mask"], gen,
                                                                dev_batch["pos_heavyatom"], dev_batch["mask_heavyatom"])
                assert not out["atom_clash"][gen][:, 4:].any()
            aa_s = torch.where(gen, cu(final["seqs"]), cu(final["seqs_1"]))
            direct = geometry.structural_violations(pos_s, mask_s & dev_batch["res_mask"].bool()[:, :, None], aa_s, index, query=q, group=gen)
            assert torch.equal(out["atom_clash"], direct["clash_atom"]) and torch.equal(out["residue_bond_violation"], direct["connection_violation"])
            o = VO.violations(pos_s[0].cpu().numpy(), (mask_s & dev_batch["res_mask"].bool()[:, :, None])[0].cpu().numpy(), aa_s[0].cpu().numpy(),
                              index[0].cpu().numpy(), RADIUS, PRO, None if q is None else q[0].cpu().numpy(), gen[0].cpu().numpy())
            ok = o["connection_margin"] >= 1e-4
            assert np.array_equal(out["residue_bond_violation"][0].cpu().numpy()[ok], o["connection_violation"][ok])
    # a sample without generated residues: NaN, and it does not count in valid_fraction
    none = dict(dev_batch)
    none["generate_mask"] = dev_batch["generate_mask"].clone()
    none["generate_mask"][1] = False
    out = metrics.structural_violations(final, none)
    assert torch.isnan(out["clash"][1]) and torch.isnan(out["bond_violation_native"][1]) and not torch.isnan(out["clash"][0])
    keep = torch.tensor([0, 2, 3])
    assert abs(float(out["valid_fraction"]) - float(out["valid"][keep].double().mean())) <= 1e-12
