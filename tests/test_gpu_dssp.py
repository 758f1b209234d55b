"""GPU checks of DSSP: pf_dssp_fwd against the numpy float64 oracle (dssp_oracle.py) from 3 to 512 residues on NeRF chains, the
constructs of the CPU tests and backbones made by the package's reconstruction kernels; determinism and independence of the batch;
metrics.secondary_structure after a short sample() run."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import dssp_build as DB  # noqa: E402
import dssp_oracle as DO  # noqa: E402
import pepflowww_amd  # noqa: E402
from pepflowww_amd import full_atom, geometry, metrics, synth  # noqa: E402
from pepflowww_amd.preprocess import residue_type  # noqa: E402

PRO = residue_type("PRO")


def cu(t):
    return torch.as_tensor(t).cuda()


_PAIRS = {}


def strand_pair(kind):
    if kind not in _PAIRS:
        _PAIRS[kind] = DB.strand_pair(kind)
    return _PAIRS[kind]


def make_rows(rng, N, B, A=5):
    """B rows of N residues: random chains (second chain id from a random point), masks with holes, prolines; the constructs
    where they fit; the last row all masked.  -> pos [B,N,A,3] fp32 (atoms 4.. random), mask, chain, aa"""
    pos = rng.uniform(-30, 30, size=(B, N, A, 3))
    mask = np.ones((B, N), bool)
    chain = np.zeros((B, N), np.int64)
    aa = rng.integers(0, 20, size=(B, N))
    aa[aa == PRO] = 0
    constructs = [DB.helix(min(N, 20), DB.ALPHA), DB.helix(min(N, 16), DB.HELIX_310), DB.helix(min(N, 16), DB.PI)]
    if N >= 12:
        constructs += [strand_pair("anti")[0], strand_pair("par")[0]]
    for b in range(B):
        c = b if b < len(constructs) else None
        if c is not None and b < B - 1:
            bb = constructs[c]
            if len(bb) == 12 and c >= 3:                                 # strand pair: two chain ids
                chain[b, 6:12] = 1
                chain[b, 12:] = 2
            else:
                chain[b, len(bb):] = 1
            bb = bb + (0.15 * rng.standard_normal(bb.shape) if b % 2 else 0.0)
            pos[b, :len(bb), :4] = bb
            if len(bb) < N:
                pos[b, len(bb):, :4] = DB.random_chain(rng, N - len(bb)) + 40.0
        else:
            pos[b, :, :4] = DB.random_chain(rng, N)
            if N > 4:
                chain[b, int(rng.integers(N // 2, N)):] = 1
            mask[b] = rng.random(N) > 0.08
            aa[b, rng.random(N) < 0.08] = PRO
    mask[B - 1] = False
    return pos.astype(np.float32), mask, chain, aa


def check_against_oracle(pos, mask, chain, aa, ss, acc, en, max_excused=0.01):
    ss, acc, en = ss.cpu().numpy(), acc.cpu().numpy(), en.cpu().double().numpy()
    excused = 0
    for b in range(pos.shape[0]):
        o = DO.dssp(pos[b, :, :4].astype(np.float64), mask[b], chain[b], aa[b] == PRO)
        if o["margin"] < 1e-6:
            excused += 1
            continue
        assert np.array_equal(ss[b], o["ss"]), (b, DO.to_string(ss[b]), DO.to_string(o["ss"]))
        assert np.array_equal(acc[b], o["acc"]), (b, np.nonzero((acc[b] != o["acc"]).any(1))[0])
        assert np.abs(en[b] - o["energy"]).max() <= 1e-5
    assert excused <= max_excused * pos.shape[0] + 1e-9, excused
    return excused


ROWS_AT = {3: 6, 5: 8, 8: 8, 25: 24, 64: 12, 65: 12, 128: 8, 256: 6, 512: 6}


@pytest.mark.parametrize("N", sorted(ROWS_AT))
def test_kernel_matches_oracle(N):
    rng = np.random.default_rng(2000 + N)
    pos, mask, chain, aa = make_rows(rng, N, ROWS_AT[N])
    ss, acc, en = geometry.dssp(cu(pos), cu(mask), cu(chain), cu(aa), hbonds=True)
    assert ss.dtype == torch.uint8 and acc.dtype == torch.int32 and en.dtype == torch.float32
    check_against_oracle(pos, mask, chain, aa, ss, acc, en)
    assert (ss[-1] == 255).all()


def test_pooled_oracle_margin_budget():
    """over many 25-residue rows at once (the evaluation's shape), at most 1 % of the chains may sit within 1e-6 of a threshold"""
    rng = np.random.default_rng(5)
    pos, mask, chain, aa = make_rows(rng, 25, 200)
    ss, acc, en = geometry.dssp(cu(pos), cu(mask), cu(chain), cu(aa), hbonds=True)
    check_against_oracle(pos, mask, chain, aa, ss, acc, en)


def test_constructs_give_their_codes():
    bb = np.stack([DB.helix(20, DB.ALPHA), DB.helix(20, DB.HELIX_310), DB.helix(20, DB.PI)]).astype(np.float32)
    ss = geometry.dssp(cu(bb), cu(np.ones((3, 20), bool)))
    assert geometry.ss_strings(ss) == ["-" + c * 18 + "-" for c in "HGI"]
    aa = np.zeros((1, 20), np.int64)
    aa[0, 10:14] = PRO
    ss = geometry.dssp(cu(bb[:1]), cu(np.ones((1, 20), bool)), aa=cu(aa))
    assert geometry.ss_strings(ss) == ["-" + "H" * 8 + "SS" + "H" * 8 + "-"]
    pair, ch = strand_pair("anti")
    ss = geometry.dssp(cu(pair[None].astype(np.float32)), cu(np.ones((1, 12), bool)), chain=cu(ch[None]))
    assert geometry.ss_strings(ss) == ["-EEEE--EEEE-"]


def test_backbones_from_the_package():
    rng = np.random.default_rng(9)
    B, L = 6, 40
    # native frames: the frames of NeRF chains (N, CA, C) as rotations about CA; random frames: random rotations, CA walk
    natives = np.stack([DB.random_chain(rng, L) for _ in range(B // 2)])
    R = np.zeros((B, L, 3, 3))
    t = np.zeros((B, L, 3))
    for b in range(B // 2):
        nb, ca, c = natives[b, :, 0], natives[b, :, 1], natives[b, :, 2]
        e1 = (c - ca) / np.linalg.norm(c - ca, axis=-1, keepdims=True)
        u = nb - ca
        e2 = u - (u * e1).sum(-1, keepdims=True) * e1
        e2 /= np.linalg.norm(e2, axis=-1, keepdims=True)
        R[b] = np.stack([e1, e2, np.cross(e1, e2)], -1)
        t[b] = ca
    for b in range(B // 2, B):
        q = rng.standard_normal((L, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        w, x, y, z = q.T
        R[b] = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                         np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                         np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)
        d = rng.standard_normal((L, 3))
        t[b] = np.cumsum(3.8 * d / np.linalg.norm(d, axis=1, keepdims=True), 0)
    aa = rng.integers(0, 20, size=(B, L))
    mask = np.ones((B, L), bool)
    mask[1, 17] = False
    chain = np.zeros((B, L), np.int64)
    chain[2, 30:] = 1
    res_nb = np.tile(np.arange(1, L + 1), (B, 1))
    Rd, td, aad = cu(R).float(), cu(t).float(), cu(aa)
    bb_frames = full_atom.reconstruct_backbone(Rd, td, aad, cu(chain), cu(res_nb), cu(mask))
    angles = cu(rng.uniform(0, 2 * np.pi, size=(B, L, 5))).float()
    bb_full = full_atom.full_atom_reconstruction(Rd, td, angles, aad)[0]
    for bb in (bb_frames, bb_full):
        ss, acc, en = geometry.dssp(bb, cu(mask), cu(chain), aad, hbonds=True)
        check_against_oracle(bb.cpu().numpy(), mask, chain, aa, ss, acc, en, max_excused=0.0)


def _bits(out):
    return [v.cpu().view(torch.int32) if v.dtype == torch.float32 else v.cpu() for v in out]


def test_deterministic_and_independent_of_the_batch():
    rng = np.random.default_rng(12)
    pos, mask, chain, aa = make_rows(rng, 64, 24)
    P, M, CH, AA = cu(pos), cu(mask), cu(chain), cu(aa)
    run = lambda idx: _bits(geometry.dssp(P[idx], M[idx], CH[idx], AA[idx], hbonds=True))  # noqa: E731
    full = torch.arange(24)
    a, b = run(full), run(full)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    perm = torch.from_numpy(np.random.default_rng(13).permutation(24))
    for x, y in zip(run(perm), a):
        assert torch.equal(x, y[perm])
    for part in (full[:7], full[7:], full[5:6]):
        for x, y in zip(run(part), a):
            assert torch.equal(x, y[part])
    # in other company: a row of 64 residues among 100 random others
    other, om, oc, oa = make_rows(np.random.default_rng(14), 64, 100)
    mix = [torch.cat([cu(other)[:50], P[3:4], cu(other)[50:]]), torch.cat([cu(om)[:50], M[3:4], cu(om)[50:]]),
           torch.cat([cu(oc)[:50], CH[3:4], cu(oc)[50:]]), torch.cat([cu(oa)[:50], AA[3:4], cu(oa)[50:]])]
    for x, y in zip(_bits(geometry.dssp(*mix, hbonds=True)), a):
        assert torch.equal(x[50], y[3])


def test_bound_raises():
    big = torch.zeros(1, geometry.DSSP_MAX_N + 1, 4, 3, device="cuda")
    with pytest.raises(ValueError):
        geometry.dssp(big, torch.ones(1, geometry.DSSP_MAX_N + 1, dtype=torch.bool, device="cuda"))


@pytest.fixture(scope="module")
def model(seeded_sd):
    m = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
    m.load_state_dict(seeded_sd)
    return m.cuda().eval()


def test_secondary_structure_after_sample(model):
    B, L, NS = 4, 40, 3
    batch = synth.make_pocket_batch(B, L, 12, seed=51)
    noise = synth.make_noise(B, L, NS, seed=52)
    dev_batch = {k: cu(v) for k, v in batch.items()}
    final = model.sample(dev_batch, num_steps=NS, noise=noise)[-1]
    gen = (batch["generate_mask"].bool() & batch["res_mask"].bool()).numpy()
    chain = batch["chain_nb"].numpy()
    seqs, seqs1 = final["seqs"].numpy(), final["seqs_1"].numpy()
    native_ok = gen & batch["mask_heavyatom"][:, :, :4].bool().all(-1).numpy()
    pos = batch["pos_heavyatom"].float().numpy()
    nat = geometry.dssp(dev_batch["pos_heavyatom"], cu(native_ok), dev_batch["chain_nb"], cu(final["seqs_1"]))
    for backbone in ("full_atom", "frames"):
        out = metrics.secondary_structure(final, dev_batch, backbone=backbone)
        if backbone == "full_atom":
            bb = full_atom.full_atom_reconstruction(cu(final["rotmats"]), cu(final["trans"]), cu(final["angles"]), cu(final["seqs"]))[0]
        else:
            bb = full_atom.reconstruct_backbone(cu(final["rotmats"]), cu(final["trans"]), cu(final["seqs"]), dev_batch["chain_nb"],
                                                dev_batch["res_nb"], dev_batch["res_mask"])
        bb = bb.cpu().numpy()
        ss_s, ss_n = out["ss_sample"].cpu().numpy(), out["ss_native"].cpu().numpy()
        assert torch.equal(out["ss_native"], nat)
        for b in range(B):
            o = DO.dssp(bb[b, :, :4].astype(np.float64), gen[b], chain[b], seqs[b] == PRO)
            assert o["margin"] >= 1e-6 and np.array_equal(ss_s[b], o["ss"]), (backbone, b)
            o = DO.dssp(pos[b, :, :4].astype(np.float64), native_ok[b], chain[b], seqs1[b] == PRO)
            assert o["margin"] >= 1e-6 and np.array_equal(ss_n[b], o["ss"]), (backbone, b)
        simp = {0: "H", 1: "E", 2: "C", 255: "."}
        ssr = out["ssr"].cpu().numpy()
        for b in range(B):
            a = [simp[int(c)] for c in geometry.ss_simplify(out["ss_sample"][b]).cpu()[gen[b]]]
            n = [simp[int(c)] for c in geometry.ss_simplify(out["ss_native"][b]).cpu()[gen[b]]]
            agree = np.mean([x == y and y != "." for x, y in zip(a, n)])
            assert 0.0 <= ssr[b] <= 1.0 and abs(ssr[b] - agree) <= 1e-12
            for key, c in (("helix", "H"), ("strand", "E"), ("coil", "C")):
                assert abs(out[key][b].item() - np.mean([x == c for x in a])) <= 1e-12
        assert abs(out["ssr_pooled"].item() - ssr.mean()) <= 1e-12
