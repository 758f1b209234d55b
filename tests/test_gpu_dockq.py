"""GPU checks of the interface contacts and DockQ: pf_contacts_fwd (through geometry.interface_contacts) against the numpy float64
oracle (lddt_oracle.py) on seeded shapes from 1 to 512 residues; geometry.dockq against the oracle's Kabsch restatement; bitwise
repeatability and independence of the batch and of the order of the work list; peak memory; constructed cases with known answers;
metrics.docking_quality after a short sample() run.  The comparison rule and its cap are stated in lddt_cases.py.  DockQ is written
from the publication (Basu & Wallner 2016) and is not checked against the DockQ program."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import lddt_cases as LC  # noqa: E402
import lddt_oracle as LO  # noqa: E402
import pepflowww_amd  # noqa: E402
from pepflowww_amd import full_atom, geometry, metrics, synth  # noqa: E402
from pepflowww_amd.geometry import dockq as _dockq_is_there  # noqa: E402,F401

RMSD_TOL = 1e-5             # what test_gpu_eval.py's superpose tests allow for identical inputs


def cu(t):
    return None if t is None else torch.as_tensor(t).cuda()


def dev(d):
    return {k: cu(v) for k, v in d.items()}


def run(x, y, pairs, group, **kw):
    out = geometry.interface_contacts(dev(x), dev(x) if y is x else dev(y), cu(pairs), cu(group), **kw)
    torch.cuda.synchronize()
    return out


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "f15_lddt.npz")))


# ---- the float64 oracle on seeded shapes -------------------------------------------------------------------------------------------

SHAPES = {1: (6, 10.0), 2: (6, 8.0), 15: (6, 20.0), 16: (6, 20.0), 17: (6, 20.0), 33: (6, 25.0), 52: (6, 25.0), 144: (4, 40.0),
          256: (2, 50.0), 512: (2, 60.0)}


@pytest.mark.parametrize("N", sorted(SHAPES))
def test_kernel_matches_oracle(N):
    B, scale = SHAPES[N]
    rng = np.random.default_rng(1600 + N)
    x, y = LC.make_pair_batch(rng, B, N, scale)
    pairs = LC.work_list(B)
    group = rng.random((B, N)) < 0.4
    group[0] = np.arange(N) >= N - min(N, 12)               # a peptide at the end: most column tiles are skipped
    if B > 2:
        group[2] = False                                    # one group only: nothing counts
    runs = [dict()] if N >= 256 else [dict(), dict(slots="backbone", contact_cutoff=4.0, interface_cutoff=8.0), dict(slots=0x7FFF)]
    contacts = 0
    for kw in runs:
        out = run(x, y, pairs, group, **kw)
        assert out["contacts_x"].dtype == torch.int32 and out["interface_y"].dtype == torch.bool and out["min_dist_x"].dtype == torch.float32
        assert out["contacts_shared"].shape == (len(pairs), N)
        got = host(out)
        slots = kw.get("slots", "all")
        contacts += LC.check_contacts(got, x, y, pairs, group, slots if isinstance(slots, int) else geometry.SLOT_MASKS[slots],
                                      kw.get("contact_cutoff", 5.0), kw.get("interface_cutoff", 10.0))[0]
        assert not got["contacts_x"][B - 1].any() and np.isinf(got["min_dist_y"][B - 1]).all()      # x[B-1] is all masked
        for k in got:
            assert np.array_equal(got[k][B + 1], got[k][0]), k                          # the repeated pair
        if B > 2:
            assert not got["contacts_y"][pairs[:, 1] == 2].any() and not got["interface_y"][pairs[:, 1] == 2].any()
    assert contacts > 0 or N == 1


def test_dockq_matches_oracle():
    rng = np.random.default_rng(1631)
    B, N = 4, 52
    x, y = LC.make_pair_batch(rng, B, N, 14.0, mask_last_x=False)
    group = np.tile(np.arange(N) >= 40, (B, 1))
    pairs = np.array([[0, 0], [1, 1], [2, 2], [3, 3], [1, 2], [4, 0]], np.int32)
    out = geometry.dockq(dev(x), dev(y), cu(pairs), cu(group))
    for k in ("fnat", "fnonnat", "irmsd", "lrmsd", "dockq"):
        assert out[k].shape == (len(pairs),) and out[k].dtype == torch.float64, k
    got = host(out)
    bound = LC.bound_of(x, y)
    for p, (i, j) in enumerate(pairs[:5].tolist()):
        o = LO.dockq(x["pos"][i], x["atom_mask"][i], y["pos"][j], y["atom_mask"][j], group[j])
        c = LO.contacts(x["pos"][i], x["atom_mask"][i], y["pos"][j], y["atom_mask"][j], group[j], bound=bound)
        assert not c["near_contact_x"].any() and not c["near_contact_y"].any() and not c["near_interface_y"].any()      # the case's condition
        assert got["n_native_contacts"][p] == o["n_native_contacts"] > 0 and got["n_sample_contacts"][p] == o["n_sample_contacts"]
        assert abs(got["fnat"][p] - o["fnat"]) <= 1e-12 and abs(got["fnonnat"][p] - o["fnonnat"]) <= 1e-12
        # the superposition tolerance of test_gpu_eval.py's comparison with Kabsch in float64
        assert abs(got["irmsd"][p] - o["irmsd"]) <= 1e-4 + 1e-5 * o["irmsd"], (p, got["irmsd"][p], o["irmsd"])
        assert abs(got["lrmsd"][p] - o["lrmsd"]) <= 1e-4 + 1e-5 * o["lrmsd"], (p, got["lrmsd"][p], o["lrmsd"])
        assert abs(got["dockq"][p] - o["dockq"]) <= 1e-4
        cls = int(o["dockq"] >= 0.23) + int(o["dockq"] >= 0.49) + int(o["dockq"] >= 0.80)
        assert got["dockq_class"][p] == cls or min(abs(o["dockq"] - t) for t in (0.23, 0.49, 0.80)) < 1e-4
    assert all(np.isnan(got[k][5]) for k in ("fnat", "fnonnat", "irmsd", "lrmsd", "dockq")) and got["dockq_class"][5] == 0


# ---- repeatability -----------------------------------------------------------------------------------------------------------------

def _bits(out):
    return {k: (v.view(torch.int32) if v.dtype == torch.float32 else v) for k, v in out.items()}


def test_bitwise_repeatable_and_independent_of_batch_and_order():
    rng = np.random.default_rng(1641)
    B, N = 8, 100
    x, y = LC.make_pair_batch(rng, B, N, 30.0)
    group = rng.random((B, N)) < 0.4
    pairs = LC.work_list(B)
    a = _bits(run(x, y, pairs, group))
    b = _bits(run(x, y, pairs, group))
    rev = _bits(run(x, y, pairs[::-1].copy(), group))
    one = _bits(run({k: v[3:4] for k, v in x.items()}, {k: v[4:5] for k, v in y.items()}, np.array([[0, 0]], np.int32), group[4:5]))
    assert int(a["contacts_x"].sum()) > 0
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k], rev[k].flip(0)), k
        assert torch.equal(a[k][3], one[k][0]), k


def test_peak_memory_is_not_pair_sized():
    """B = 8, N = 144, all atoms: one [2160, 2160] fp32 distance matrix is 18.7 MB per pair; the call may hold 1 MB beyond its inputs
    and outputs."""
    rng = np.random.default_rng(1643)
    B, N = 8, 144
    x, y = LC.make_pair_batch(rng, B, N, 40.0, mask_last_x=False)
    X = dict(pos=cu(x["pos"]), atom_mask=cu(x["atom_mask"]).to(torch.uint8), aa=cu(x["aa"]))
    Y = dict(pos=cu(y["pos"]), atom_mask=cu(y["atom_mask"]).to(torch.uint8), aa=cu(y["aa"]))
    ids = torch.arange(B, dtype=torch.int32, device="cuda")
    pairs, G = torch.stack([ids, ids], 1), cu(rng.random((B, N)) < 0.2).to(torch.uint8)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = geometry.interface_contacts(X, Y, pairs, G)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    out_bytes = sum(v.numel() * v.element_size() for v in out.values())
    assert peak - base - out_bytes <= 2 ** 20, (peak - base, out_bytes)
    assert int(out["contacts_x"].sum()) > 0


# ---- constructed answers -----------------------------------------------------------------------------------------------------------

def rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q))


def test_two_atoms_around_the_contact_cutoff():
    pos = np.zeros((2, 2, 14, 3), np.float32)
    pos[0, 1, 1, 0], pos[1, 1, 1, 0] = 4.9, 5.1
    mask = np.zeros((2, 2, 14), bool)
    mask[:, :, 1] = True
    s = dict(pos=pos, atom_mask=mask, aa=np.zeros((2, 2), np.int64))
    group = np.array([[0, 1], [0, 1]], bool)
    got = host(run(s, s, np.array([[0, 1], [1, 0]], np.int32), group))
    assert got["contacts_x"].tolist() == [[1, 1], [0, 0]] and got["contacts_y"].tolist() == [[0, 0], [1, 1]]
    assert not got["contacts_shared"].any() and got["interface_x"].all() and got["interface_y"].all()
    assert np.allclose(got["min_dist_x"], [[4.9, 4.9], [5.1, 5.1]], atol=1e-6)
    assert not host(run(s, s, np.array([[0, 1]], np.int32), np.ones((2, 2), bool)))["contacts_x"].any()


def test_known_answers(gold):
    pos, mask, aa, group = gold["pos"][:1], gold["atom_mask"][:1], gold["aa"][:1], gold["group"][None]
    y = dict(pos=pos, atom_mask=mask, aa=aa)
    pairs = np.array([[0, 0]], np.int32)
    G = cu(group)
    same = host(geometry.dockq(dev(y), dev(y), cu(pairs), G))
    o = LO.contacts(pos[0], mask[0], pos[0], mask[0], group[0])
    assert np.array_equal(same["contacts_y"][0], o["contacts_y"]) and np.array_equal(same["contacts_x"], same["contacts_shared"])
    assert same["n_native_contacts"][0] == o["contacts_y"][group[0]].sum() > 0
    assert same["fnat"][0] == 1.0 and same["fnonnat"][0] == 0.0
    assert same["irmsd"][0] <= RMSD_TOL and same["lrmsd"][0] <= RMSD_TOL and abs(same["dockq"][0] - 1.0) <= RMSD_TOL
    assert same["dockq_class"][0] == 3
    # the whole model rigidly rotated and moved: the same contacts (a min distance away from the cutoff by more than the rounding)
    rng = np.random.default_rng(1651)
    c = LO.contacts(pos[0], mask[0], pos[0], mask[0], group[0], bound=1e-3)
    assert not c["near_contact_x"].any() and not c["near_interface_x"].any()
    moved = dict(y, pos=(pos @ rotation(rng).T.astype(np.float32) + np.array([30.0, -20.0, 10.0], np.float32)).astype(np.float32))
    rigid = host(geometry.dockq(dev(moved), dev(y), cu(pairs), G))
    for k in ("contacts_x", "contacts_y", "contacts_shared", "interface_x", "interface_y"):
        assert np.array_equal(rigid[k], same[k]), k
    assert rigid["fnat"][0] == 1.0 and rigid["irmsd"][0] <= 1e-4 and rigid["lrmsd"][0] <= 1e-4       # test_gpu_eval.py's for a moved copy
    # the ligand moved 100 A: no contact in the model
    away = pos.copy()
    away[0, 40:] += np.array([100.0, 0.0, 0.0], np.float32)
    far = host(geometry.dockq(dev(dict(y, pos=away)), dev(y), cu(pairs), G))
    assert not far["contacts_x"].any() and not far["interface_x"].any() and far["fnat"][0] == 0.0 and np.isnan(far["fnonnat"][0])
    assert np.array_equal(far["contacts_y"], same["contacts_y"]) and abs(far["lrmsd"][0] - 100.0) <= 1e-3
    assert far["dockq_class"][0] == 0
    # the ligand moved by a vector of length 3 A, the receptor fixed: LRMSD 3
    shifted = pos.copy()
    shifted[0, 40:] += np.array([1.0, 2.0, 2.0], np.float32)
    three = host(geometry.dockq(dev(dict(y, pos=shifted)), dev(y), cu(pairs), G))
    assert abs(three["lrmsd"][0] - 3.0) <= RMSD_TOL, three["lrmsd"][0]


# ---- metrics.docking_quality -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(seeded_sd):
    m = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
    m.load_state_dict(seeded_sd)
    return m.cuda().eval()


FLOATS = ("fnat", "fnonnat", "irmsd", "lrmsd", "dockq")


def test_docking_quality_after_sample(model):
    B, L, NS = 4, 40, 3
    batch = synth.make_pocket_batch(B, L, 12, seed=61)
    noise = synth.make_noise(B, L, NS, seed=62)
    dev_batch = {k: cu(v) for k, v in batch.items()}
    final = model.sample(dev_batch, num_steps=NS, noise=noise)[-1]
    for backbone in ("full_atom", "frames"):
        out = metrics.docking_quality(final, dev_batch, backbone=backbone)
        for k in FLOATS:
            assert out[k].shape == (B,) and out[k].dtype == torch.float64, k
        for k in ("dockq_class", "n_native_contacts", "n_sample_contacts"):
            assert out[k].shape == (B,) and out[k].dtype == torch.int64, k
        for k in ("fnat", "fnonnat", "dockq"):
            assert (torch.isnan(out[k]) | ((out[k] >= 0) & (out[k] <= 1))).all(), k
        assert (torch.isnan(out["irmsd"]) | (out["irmsd"] >= 0)).all() and (torch.isnan(out["lrmsd"]) | (out["lrmsd"] >= 0)).all()
        assert ((out["dockq_class"] >= 0) & (out["dockq_class"] <= 3)).all()
        for k in ("dockq_pooled", "success_rate"):
            assert out[k].dim() == 0 and out[k].dtype == torch.float64, k
        has = ~torch.isnan(out["dockq"])
        if has.any():
            assert abs(float(out["dockq_pooled"]) - float(out["dockq"][has].mean())) <= 1e-12
            assert abs(float(out["success_rate"]) - float((out["dockq"][has] >= 0.23).double().mean())) <= 1e-12
    # other cut-offs run (CAPRI-peptide)
    metrics.docking_quality(final, dev_batch, contact_cutoff=4.0, interface_cutoff=8.0)
    # the native passed as its own sample: the rebuilt complex as pos_heavyatom, its types as seqs_1
    gen = dev_batch["generate_mask"].bool() & dev_batch["res_mask"].bool()
    f = {k: cu(v) for k, v in final.items()}
    pos_s, mask_s = full_atom.reconstruct_sample(f["rotmats"], f["trans"], f["angles"], f["seqs"], gen, dev_batch["pos_heavyatom"])
    mask_s = torch.where(gen[:, :, None], mask_s, dev_batch["mask_heavyatom"].bool()[:, :, :15])
    f["seqs_1"] = torch.where(gen, f["seqs"], f["seqs_1"])
    own = metrics.docking_quality(f, dict(dev_batch, pos_heavyatom=pos_s, mask_heavyatom=mask_s))
    has = own["n_native_contacts"] > 0
    assert (own["fnat"][has] == 1.0).all() and (own["fnonnat"][has] == 0.0).all() and torch.isnan(own["dockq"][~has]).all()
    assert (own["irmsd"][has] <= RMSD_TOL).all() and (own["lrmsd"][has] <= RMSD_TOL).all()
    assert ((own["dockq"][has] - 1.0).abs() <= RMSD_TOL).all() and (own["dockq_class"][has] == 3).all()
