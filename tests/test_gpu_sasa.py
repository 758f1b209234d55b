"""GPU checks of the solvent-accessible surface: pf_sasa_fwd (through geometry.sasa) against the numpy float64 oracle (sasa_oracle.py)
on seeded shapes from 1 to 512 residues and 1 to 1024 points, plain, with `group` and with `query` + `group`; translation;
crowded structures that overflow the per-wave neighbour list and fill the stage; constructed cases with known answers;
repeatability, independence of the batch and peak memory; metrics.interface_area after a short sample() run.

Bounds (derived, not tuned).  Counts: the kernel's fp32 test and the oracle's float64 test can only disagree on a point whose
decisive margin is below eps = 32 * 2^-23 * 2 * (1.8 + probe) (about ten fp32 roundings of lengths no larger than the reach; d = x_a -
x_b is exact to its last bit in both), so per atom |count - oracle| <= the oracle's number of such points, and per case those
differences total at most 1e-4 of the points evaluated (the marginal share itself is a few 1e-6, so the cap cannot hide a wrong
neighbour list: a single missed partner buries tens of points).  Areas, given the kernel's own count: sasa_atom is one fp32 rounding
of the float64 formula (bound 4 * 2^-23 relative), sasa_residue adds 14 fp32 additions (16 * 2^-23), the totals are fp64 sums of the
fp32 atom areas rounded once (4 * 2^-23)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import dssp_build as DB  # noqa: E402
import sasa_oracle as SO  # noqa: E402
import pepflowww_amd  # noqa: E402
from pepflowww_amd import geometry, metrics, synth  # noqa: E402
from pepflowww_amd.preprocess import residue_type  # noqa: E402

ULP = 2.0 ** -23
RADIUS = geometry.sasa_radius_table().numpy()
GLY = residue_type("GLY")
PROBE = 1.4


def cu(t):
    return None if t is None else torch.as_tensor(t).cuda()


def run(pos, mask, aa, query=None, group=None, **kw):
    out = geometry.sasa(cu(pos), cu(mask), cu(aa), query=cu(query), group=cu(group), **kw)
    torch.cuda.synchronize()
    return out


def make_batch(rng, B, N, scale, A=15):
    """B structures of N residues with coordinates within +-scale: NeRF backbone segments of up to 30 residues placed at random (so
    bonded neighbours, gaps and separate pieces all occur), some samples with noisy atoms; side-chain atoms 1.5 - 4 A from CA; masks
    with holes; residue types 0..20; the last sample all masked.  -> pos [B,N,A,3] fp32, mask [B,N,A], aa [B,N]"""
    pos = np.zeros((B, N, A, 3))
    for b in range(B):
        k = 0
        while k < N:
            n = int(min(N - k, rng.integers(1, 31)))
            seg = DB.random_chain(rng, n) @ DB.rotation(rng.standard_normal(3) * 2.0).T
            room = max(scale - 4.0 - np.abs(seg - seg.mean((0, 1))).max(), 0.0)
            if room == 0.0:
                seg = seg * (scale - 4.0) / np.abs(seg - seg.mean((0, 1))).max()
            seg = seg - seg.mean((0, 1)) + rng.uniform(-room, room, 3)
            pos[b, k:k + n, :4] = seg
            k += n
        d = rng.standard_normal((N, A - 4, 3))
        pos[b, :, 4:] = pos[b, :, 1:2] + d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(1.5, 4.0, (N, A - 4, 1))
        if b % 3 == 2:
            pos[b] += rng.standard_normal(pos[b].shape) * (0.05 if b % 2 else 0.5)
    pos = np.clip(pos, -scale, scale).astype(np.float32)
    aa = rng.integers(0, 21, size=(B, N))
    mask = (rng.random((B, N, A)) > 0.1) & (rng.random((B, N, 1)) > 0.08)
    mask[B - 1] = False
    return pos, mask, aa.astype(np.int64)


def check_sample(got, o, P, query=None, own=True):
    """one sample of the kernel's outputs (numpy) against its oracle `o` (computed with `group`, without `query`) -> (excused
    differences, points evaluated)"""
    exists = o["exists"]
    evaluated = exists if query is None else exists & (np.asarray(query) != 0)[:, None]
    excused = 0
    for tag in ("", "_own") if own else ("",):
        cnt = got["count" + tag]
        assert (cnt[~exists] == 0).all() and (cnt[exists & ~evaluated] == -1).all(), tag
        diff = np.abs(cnt - o["count" + tag])[evaluated]
        assert (diff <= o["marginal" + tag][evaluated]).all(), (tag, np.argwhere(np.abs(cnt - o["count" + tag]) * evaluated > o["marginal" + tag])[:4])
        excused += int(diff.sum())
        # the areas, given the kernel's own count
        c = np.maximum(cnt, 0).astype(np.float64)
        want = o["sphere"] * c
        assert (np.abs(got["sasa_atom" + tag] - want) <= 4 * ULP * want).all(), tag
        assert (np.abs(got["sasa_residue" + tag] - want.sum(1)) <= 16 * ULP * want.sum(1)).all(), tag
        assert abs(float(got["sasa_total" + tag]) - want.sum()) <= 4 * ULP * want.sum(), tag
    if own:
        assert (got["count_own"] >= got["count"]).all()
    return excused, int(evaluated.sum()) * P * (2 if own else 1)


def check_modes(pos, mask, aa, P, rng, samples=None, probe=PROBE, masked_last=True):
    """plain, with group, with query + group, against one oracle evaluation per sample"""
    B, N = aa.shape
    group = rng.random((B, N)) < 0.4
    query = rng.random((B, N)) < 0.3
    query[0, N - 1] = True
    if B > 2:
        query[1] = np.arange(N) == N - 1                    # a single query residue, in the last tile
    u = geometry.sphere_points(P).numpy()
    samples = range(B) if samples is None else samples
    oracle = {b: SO.sasa(pos[b], mask[b], aa[b], RADIUS, u, probe, group=group[b]) for b in samples}
    for q, g in ((None, None), (None, group), (query, group)):
        out = run(pos, mask, aa, q, g, n_points=P, probe_radius=probe)
        assert set(out) == {"count", "sasa_atom", "sasa_residue", "sasa_total"} | (
            set() if g is None else {"count_own", "sasa_atom_own", "sasa_residue_own", "sasa_total_own"})
        assert out["count"].dtype == torch.int32 and out["count"].shape == (B, N, 15) and out["sasa_residue"].shape == (B, N)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        excused = points = 0
        for b in samples:
            e, n = check_sample({k: v[b] for k, v in got.items()}, oracle[b], P, None if q is None else q[b], own=g is not None)
            excused, points = excused + e, points + n
        print(f"B {B} N {N} P {P} query {q is not None} group {g is not None}: excused {excused} of {points} points")
        assert excused <= 1e-4 * points, (excused, points)
        for k, v in got.items():                            # the all-masked sample
            assert not masked_last or not v[-1].any(), k


# ---- the float64 oracle on seeded shapes -------------------------------------------------------------------------------------------

SHAPES = [(3, 1, 960, 10.0), (3, 2, 960, 5.0), (3, 15, 64, 20.0), (3, 16, 92, 30.0), (3, 17, 1, 60.0), (3, 33, 960, 25.0),
          (2, 48, 1024, 25.0), (2, 144, 92, 40.0), (2, 512, 92, 60.0)]


@pytest.mark.parametrize("B,N,P,scale", SHAPES)
def test_kernel_matches_oracle(B, N, P, scale):
    rng = np.random.default_rng(5000 + N)
    pos, mask, aa = make_batch(rng, B, N, scale)
    check_modes(pos, mask, aa, P, rng, samples=[0] if N == 512 else None)


def test_fourteen_slots_and_another_probe():
    """pos with 14 slots (no OXT) gives slot 14 count 0; a probe of 0 is the van der Waals surface"""
    rng = np.random.default_rng(5100)
    pos, mask, aa = make_batch(rng, 3, 20, 20.0, A=14)
    check_modes(pos, mask, aa, 92, rng)
    check_modes(pos, mask, aa, 64, rng, probe=0.0)
    out = run(pos, mask, aa, n_points=92)
    assert not out["count"][:, :, 14].any()
    pos15, mask15 = np.concatenate([pos, pos[:, :, :1]], 2), np.concatenate([mask, np.zeros_like(mask[:, :, :1])], 2)
    out15 = run(pos15, mask15, aa, n_points=92)
    for k in out:
        assert torch.equal(out[k], out15[k]), k


def test_translation_changes_no_count():
    """coordinates that are multiples of 2^-10 A, within +-64 A: d = x_a - x_b is exact there and after a shift by (1024, -2048, 512),
    so every count is the same"""
    rng = np.random.default_rng(5200)
    pos, mask, aa = make_batch(rng, 3, 70, 40.0)
    pos = (np.round(pos * 1024.0) / 1024.0).astype(np.float32)
    shifted = pos + np.array([1024.0, -2048.0, 512.0], np.float32)
    assert np.array_equal((shifted.astype(np.float64) - np.array([1024.0, -2048.0, 512.0])), pos.astype(np.float64))
    group = rng.random((3, 70)) < 0.4
    a, b = run(pos, mask, aa, group=group), run(shifted, mask, aa, group=group)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert a["count"].sum() > 0


# ---- crowded structures ------------------------------------------------------------------------------------------------------------

def ball(rng, N, radius):
    d = rng.standard_normal((N, 15, 3))
    pos = (d / np.linalg.norm(d, axis=-1, keepdims=True) * radius * rng.random((N, 15, 1)) ** (1 / 3)).astype(np.float32)
    return pos[None], rng.random((1, N, 15)) > 0.05, rng.integers(0, 21, size=(1, N)).astype(np.int64)


def test_collapsed_structure_overflows_the_neighbour_list():
    """40 residues with every atom inside a 3 A ball: every atom has all the others (about 450) as neighbours, several times the
    per-wave list; only the outermost atoms keep accessible points"""
    rng = np.random.default_rng(5300)
    pos, mask, aa = ball(rng, 40, 3.0)
    check_modes(pos, mask, aa, 92, rng, masked_last=False)
    out = run(pos, mask, aa, n_points=92)
    assert 0 < int(out["count"].sum()) < 0.1 * 92 * int((out["count"] >= 0).sum())


def test_compact_cloud_fills_the_stage():
    """512 residues inside a 24 A ball: no residue is culled for any row tile, so every tile stages all 6 000 atoms"""
    rng = np.random.default_rng(5400)
    pos, mask, aa = ball(rng, 512, 24.0)
    check_modes(pos, mask, aa, 92, rng, masked_last=False)


# ---- constructed answers -----------------------------------------------------------------------------------------------------------

def atoms(*specs, n_res=None):
    n = 1 + max(r for r, _, _ in specs) if n_res is None else n_res
    pos, mask = np.zeros((1, n, 15, 3), np.float32), np.zeros((1, n, 15), bool)
    for r, s, x in specs:
        pos[0, r, s] = x
        mask[0, r, s] = True
    return pos, mask, np.full((1, n), GLY, np.int64)


@pytest.mark.parametrize("P", [1, 92, 960])
def test_exact_answers(P):
    sphere = lambda r: 4 * np.pi * float(np.float32(r) + np.float32(PROBE)) ** 2  # noqa: E731
    out = run(*atoms((0, 1, [3.0, -2.0, 7.0])), n_points=P)                     # an isolated atom
    assert out["count"][0, 0].tolist() == [0, P] + [0] * 13
    for k in ("sasa_atom", "sasa_residue", "sasa_total"):
        assert abs(float(out[k].sum()) - sphere(1.7)) <= 4 * ULP * sphere(1.7), k
    out = run(*atoms((0, 1, [1.0, 1.0, 1.0]), (1, 3, [1.0, 1.0, 1.0])), n_points=P)       # an oxygen inside a coincident carbon
    assert out["count"][0, 0, 1] == P and out["count"][0, 1, 3] == 0 and out["count"].sum() == P
    for spec in (((0, 1, [0.0, 0.0, 0.0]), (0, 3, [6.03, 0.0, 0.0])), ((0, 1, [0.0, 0.0, 0.0]), (17, 3, [0.0, 6.03, 0.0]))):
        assert run(*atoms(*spec), n_points=P)["count"].sum() == 2 * P           # beyond R_a + R_b = 6.02
    for spec in (((0, 1, [0.0, 0.0, 0.0]), (0, 3, [3.0, 0.0, 0.0])), ((0, 1, [0.0, 0.0, 0.0]), (17, 3, [3.0, 0.0, 0.0]))):
        pos, mask, aa = atoms(*spec)
        assert run(pos, mask, aa, n_points=P)["count"][0, 0, 1] < P             # the same residue counts, and another tile
        mask[0, spec[1][0], 3] = False
        assert run(pos, mask, aa, n_points=P)["count"].sum() == P               # a masked partner buries nothing
    # an atom alone in its group next to the other group
    pos, mask, aa = atoms((0, 1, [0.0, 0.0, 0.0]), (1, 1, [3.0, 0.0, 0.0]))
    out = run(pos, mask, aa, group=np.array([[0, 1]]), n_points=P)
    assert out["count_own"][0, :, 1].tolist() == [P, P] and out["count"][0, 0, 1] < P
    assert (out["count_own"] >= out["count"]).all()
    # query: not evaluated, still a partner
    out = run(pos, mask, aa, query=np.array([[1, 0]]), n_points=P)
    assert out["count"][0, 1, 1] == -1 and out["count"][0, 0, 1] < P and float(out["sasa_residue"][0, 1]) == 0.0
    assert float(out["sasa_total"]) == float(out["sasa_residue"][0, 0])


def test_two_residues_that_touch():
    """two glycine backbones 4 A apart as a two-group complex: both bury area, each group on its own is that residue alone"""
    bb = DB.helix(2, DB.STRAND)
    pos = np.zeros((1, 2, 15, 3), np.float32)
    pos[0, 0, :4] = bb[0]
    pos[0, 1, :4] = bb[0] + np.array([0.0, 0.0, 4.0])
    mask = np.zeros((1, 2, 15), bool)
    mask[:, :, :4] = True
    aa = np.full((1, 2), GLY, np.int64)
    out = run(pos, mask, aa, group=np.array([[1, 0]]))
    buried = out["sasa_residue_own"] - out["sasa_residue"]
    assert (buried > 1.0).all() and (out["count_own"] - out["count"] >= 0).all()
    alone = run(pos[:, :1], mask[:, :1], aa[:, :1])
    assert torch.equal(alone["count"][0, 0], out["count_own"][0, 0])


# ---- repeatability and memory ------------------------------------------------------------------------------------------------------

def _bits(out):
    return {k: (v.view(torch.int32) if v.dtype == torch.float32 else v).cpu() for k, v in out.items()}


def test_deterministic_and_independent_of_the_batch():
    rng = np.random.default_rng(5500)
    B, N = 10, 100
    pos, mask, aa = make_batch(rng, B, N, 30.0)
    query, group = rng.random((B, N)) < 0.3, rng.random((B, N)) < 0.4
    for q, g in ((None, None), (query, group)):
        sub = lambda rows: _bits(run(pos[rows], mask[rows], aa[rows], None if q is None else q[rows],  # noqa: E731
                                     None if g is None else g[rows], n_points=92))
        full = np.arange(B)
        a = sub(full)
        for _ in range(2):
            b = sub(full)
            for k in a:
                assert torch.equal(a[k], b[k]), k
        for rows in (full[4:5], full[:5], np.array([7, 2, 9])):
            part = sub(rows)
            for k in a:
                assert torch.equal(part[k], a[k][torch.from_numpy(rows)]), k


def test_peak_memory_is_residue_sized():
    """B = 64, L = 144, P = 960: about 4e9 point tests; the call may hold its workspace [B,L,4] fp32 beyond its inputs and outputs
    (plus the allocator's rounding of each tensor to 512 bytes)"""
    rng = np.random.default_rng(5600)
    B, N = 64, 144
    pos, mask, aa = make_batch(rng, 4, N, 40.0)
    mask[3] = mask[0]
    rep = lambda x: cu(np.concatenate([x] * (B // 4)))  # noqa: E731
    X, M, T = rep(pos), rep(mask).to(torch.uint8), rep(aa)
    G = rep(rng.random((4, N)) < 0.1).to(torch.uint8)
    geometry.sasa(X[:1], M[:1], T[:1])                                  # the cached tables are not the call's
    for g in (None, G):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = geometry.sasa(X, M, T, group=g)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        out_bytes = sum(v.numel() * v.element_size() for v in out.values())
        assert peak - base - out_bytes <= B * N * 16 + 512 * (len(out) + 1), (peak - base, out_bytes)
        assert float(out["sasa_total"].min()) > 1000.0
        del out


# ---- metrics.interface_area --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(seeded_sd):
    m = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
    m.load_state_dict(seeded_sd)
    return m.cuda().eval()


PER_SAMPLE = ("sasa_peptide_free", "sasa_peptide_bound", "buried_peptide", "buried_receptor", "bsa", "buried_fraction",
              "buried_apolar_fraction", "n_interface_peptide", "n_interface_receptor", "interface_recovery")


def test_interface_area_after_sample(model):
    B, L, NS = 2, 64, 2
    batch = synth.make_pocket_batch(B, L, 8, seed=71)
    noise = synth.make_noise(B, L, NS, seed=72)
    dev_batch = {k: cu(v) for k, v in batch.items()}
    final = model.sample(dev_batch, num_steps=NS, noise=noise)[-1]
    res_mask = dev_batch["res_mask"].bool()
    gen = dev_batch["generate_mask"].bool() & res_mask
    rec = res_mask & ~gen
    nat = geometry.sasa(dev_batch["pos_heavyatom"], dev_batch["mask_heavyatom"].bool() & res_mask[:, :, None], cu(final["seqs_1"]),
                        group=gen)
    for backbone in ("full_atom", "frames"):
        out = metrics.interface_area(final, dev_batch, backbone=backbone)
        assert len(out) == 2 * (len(PER_SAMPLE) + 2)
        for tag in ("", "_native"):
            for k in PER_SAMPLE:
                assert out[k + tag].shape == (B,), k + tag
            assert out["residue_buried" + tag].shape == (B, L) and out["interface_residue" + tag].dtype == torch.bool
            assert torch.equal(out["bsa" + tag], out["buried_peptide" + tag] + out["buried_receptor" + tag])
            assert ((out["buried_fraction" + tag] >= 0) & (out["buried_fraction" + tag] <= 1)).all()
            assert (out["sasa_peptide_bound" + tag] <= out["sasa_peptide_free" + tag]).all() and (out["sasa_peptide_free" + tag] > 0).all()
            assert (out["residue_buried" + tag] >= 0).all()
            assert torch.equal(out["interface_residue" + tag], out["residue_buried" + tag] > 1.0)
            assert torch.equal(out["n_interface_peptide" + tag], (out["interface_residue" + tag] & gen).sum(1))
            assert torch.equal(out["n_interface_receptor" + tag], (out["interface_residue" + tag] & rec).sum(1))
            fr = out["buried_apolar_fraction" + tag]
            assert (torch.isnan(fr) | ((fr >= 0) & (fr <= 1))).all()
        # the native's values are those of a direct call on the native
        buried = (nat["sasa_atom_own"].double() - nat["sasa_atom"].double()).sum(-1)
        assert torch.equal(out["residue_buried_native"], buried)
        assert torch.equal(out["sasa_peptide_free_native"], (nat["sasa_atom_own"].double().sum(-1) * gen).sum(1))
        assert torch.equal(out["sasa_peptide_bound_native"], (nat["sasa_atom"].double().sum(-1) * gen).sum(1))
        assert torch.equal(out["buried_receptor_native"], (buried * rec).sum(1))
        has = out["n_interface_receptor_native"] > 0
        assert torch.equal(out["interface_recovery_native"] > 1 - 1e-9, has) and (out["interface_recovery_native"][~has] == 0).all()
        assert ((out["interface_recovery"] >= 0) & (out["interface_recovery"] <= 1)).all()
        if backbone == "frames":                            # generated residues as N, CA, C, O only
            s = metrics.interface_area(final, dev_batch, backbone="frames", n_points=92)
            assert (s["sasa_peptide_free"] > 0).all() and s["residue_buried"].shape == (B, L)
    # a sample without generated residues: NaN
    none = dict(dev_batch)
    none["generate_mask"] = dev_batch["generate_mask"].clone()
    none["generate_mask"][1] = False
    out = metrics.interface_area(final, none, n_points=92)
    assert torch.isnan(out["buried_fraction"][1]) and not torch.isnan(out["buried_fraction"][0])
    assert float(out["bsa"][1]) == 0.0 and float(out["interface_recovery_native"][1]) == 0.0
