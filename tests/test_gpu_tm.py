"""GPU checks of TM-score: pf_tm_score_fwd against the numpy float64 oracle (tm_oracle.py) from 3 to 512 points, its special cases and
determinism, the pairwise matrix, and metrics.structure_scores after a short sample() run."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import tm_oracle as TO  # noqa: E402
import pepflowww_amd  # noqa: E402
from pepflowww_amd import _capi, geometry, metrics, synth  # noqa: E402


def cu(t):
    return torch.as_tensor(t).cuda()


def _chain(rng, n):
    """a CA-like random walk: steps of 3.8 A"""
    d = rng.standard_normal((n, 3))
    return np.cumsum(3.8 * d / np.linalg.norm(d, axis=1, keepdims=True), 0)


def _cases(rng, N, B):
    """B model / target pairs of N points: target = rotated model + offset (+-50 A) + noise (0.3 - 8 A); masks with holes"""
    x = np.stack([_chain(rng, N) for _ in range(B)])
    y = np.stack([x[b] @ TO.rigid(rng).T + rng.uniform(-50, 50, 3) + rng.uniform(0.3, 8.0) * rng.standard_normal((N, 3))
                  for b in range(B)])
    mx, my = rng.random((B, N)) > 0.15, rng.random((B, N)) > 0.15
    if N <= 5:
        mx[0], my[0] = True, True                                          # keep n_ali = N in one pair
    return x.astype(np.float32), y.astype(np.float32), mx, my


PAIRS_AT = {3: 6, 4: 6, 5: 6, 8: 8, 15: 8, 25: 8, 64: 4, 65: 4, 128: 3, 256: 1, 512: 1}


@pytest.mark.parametrize("N", sorted(PAIRS_AT))
def test_kernel_matches_oracle(N):
    rng = np.random.default_rng(1000 + N)
    B = PAIRS_AT[N]
    x, y, mx, my = _cases(rng, N, B)
    ids = torch.arange(B, dtype=torch.int32)
    out = geometry.tm_score(cu(x), cu(y), cu(mx), cu(my), torch.stack([ids, ids], 1), transform=True, aligned=True)
    tm, cnt, ln = out["tm"].cpu().double().numpy(), out["count"].cpu().numpy(), out["lnorm"].cpu().numpy()
    rot, trans = out["rot"].cpu().double().numpy(), out["trans"].cpu().double().numpy()
    for b in range(B):
        o = TO.tm_score(x[b], y[b], mx[b], my[b])                           # the same fp32-rounded inputs, in float64
        assert cnt[b] == o["n_ali"] and ln[b] == o["lnorm"], b
        if o["n_ali"] < 3:
            assert math.isnan(tm[b])
            continue
        assert abs(tm[b] - o["tm"]) <= 1e-6, (N, b, tm[b], o["tm"])
        sel = mx[b] & my[b]
        rescored = TO.score(x[b][sel].astype(np.float64), y[b][sel].astype(np.float64), rot[b], trans[b], o["d0"], o["lnorm"])
        assert abs(rescored - tm[b]) <= 1e-5, (N, b, rescored, tm[b])
        assert abs(np.linalg.det(rot[b]) - 1.0) <= 1e-5
        ali = x[b].astype(np.float64) @ rot[b].T + trans[b]
        assert np.abs(out["aligned"][b].cpu().double().numpy() - ali).max() <= 1e-3


def test_identity_and_two_halves():
    rng = np.random.default_rng(3)
    n, D = 24, 100.0
    x = rng.uniform(0, 10, size=(2, n, 3)).astype(np.float32)
    y = x.copy()
    y[1, n // 2:] += np.float32(D) * np.array([0.6, 0.0, 0.8], np.float32)
    m = np.ones((2, n), bool)
    ids = torch.arange(2, dtype=torch.int32)
    out = geometry.tm_score(cu(x), cu(y), cu(m), cu(m), torch.stack([ids, ids], 1), transform=True)
    assert abs(out["tm"][0].item() - 1.0) <= 1e-6
    assert np.abs(out["rot"][0].cpu().numpy() - np.eye(3)).max() <= 1e-6
    d0 = TO.d0_of(n)
    assert abs(out["tm"][1].item() - (0.5 + 0.5 / (1 + (D / d0) ** 2))) <= 1e-6
    assert abs(out["tm"][1].item() - TO.tm_score(x[1], y[1])["tm"]) <= 1e-6


def test_small_and_out_of_range_pairs():
    rng = np.random.default_rng(4)
    x = rng.uniform(-20, 20, size=(4, 10, 3)).astype(np.float32)
    m = np.zeros((4, 10), bool)
    m[1, :1] = True
    m[2, :2] = True
    m[3, :] = True
    pairs = torch.tensor([[0, 3], [1, 3], [2, 3], [3, 3], [4, 3], [3, -1], [0, 7]], dtype=torch.int32)
    out = geometry.tm_score(cu(x), cu(x), cu(m), cu(m), pairs, transform=True, aligned=True)
    tm, cnt, ln = out["tm"].cpu(), out["count"].cpu(), out["lnorm"].cpu()
    assert cnt.tolist() == [0, 1, 2, 10, 0, 0, 0] and ln.tolist() == [10, 10, 10, 10, 0, 0, 0]
    assert all(math.isnan(tm[k].item()) for k in (0, 1, 2, 4, 5, 6)) and abs(tm[3].item() - 1.0) <= 1e-6
    assert bool(torch.isnan(out["trans"][:3]).all()) and bool(torch.isnan(out["aligned"][:3]).all())
    assert torch.equal(out["rot"][0].cpu(), torch.eye(3))


def test_bound_on_points_raises():
    big = torch.zeros(2, geometry.TM_MAX_N + 1, 3, device="cuda")
    bm = torch.ones(2, geometry.TM_MAX_N + 1, dtype=torch.bool, device="cuda")
    with pytest.raises(_capi.PepflowHipError):
        geometry.tm_score(big, big, bm, bm, torch.tensor([[0, 1]], dtype=torch.int32))


def _bits(out):
    return {k: v.cpu().view(torch.int32) if v.dtype == torch.float32 else v.cpu() for k, v in out.items()}


def test_deterministic_and_independent_of_the_work_list():
    rng = np.random.default_rng(6)
    B, N = 24, 40
    x, _, m, _ = _cases(rng, N, B)
    X, M = cu(x), cu(m)
    pairs, _, _ = geometry.group_pairs(torch.zeros(B, dtype=torch.int64))
    pairs = pairs[:150]
    run = lambda p: _bits(geometry.tm_score(X, X, M, M, p, transform=True, aligned=True))  # noqa: E731
    a, b = run(pairs), run(pairs)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    perm = torch.from_numpy(np.random.default_rng(7).permutation(len(pairs)))
    c = run(pairs[perm])
    for k in a:
        assert torch.equal(c[k], a[k][perm]), k
    h1, h2 = run(pairs[:61]), run(pairs[61:])
    for k in a:
        assert torch.equal(torch.cat([h1[k], h2[k]]), a[k]), k


def test_pairwise_matrix_two_groups():
    rng = np.random.default_rng(8)
    B, N = 64, 15
    base = _chain(rng, N)
    x = np.stack([base @ TO.rigid(rng).T + rng.uniform(0.5, 3.0) * rng.standard_normal((N, 3)) for _ in range(B)]).astype(np.float32)
    m = np.ones((B, N), bool)
    m[:, 13:] = rng.random((1, 2)) > 0.5
    groups = torch.from_numpy(np.random.default_rng(9).permutation(np.r_[np.zeros(40), np.ones(24)]).astype(np.int64))
    X, M = cu(x), cu(m)
    tm = geometry.pairwise_tm_score(X, M, groups=groups).cpu().double().numpy()
    same = (groups[:, None] == groups[None, :]).numpy()
    assert np.array_equal(tm, tm.T, equal_nan=True) and (np.diag(tm) == 1).all()
    assert np.isnan(tm[~same]).all() and not np.isnan(tm[same]).any()
    iu, ju = np.nonzero(np.triu(same, 1))
    fwd = geometry.tm_score(X, X, M, M, torch.from_numpy(np.stack([iu, ju], 1)).int())["tm"].cpu().double().numpy()
    bwd = geometry.tm_score(X, X, M, M, torch.from_numpy(np.stack([ju, iu], 1)).int())["tm"].cpu().double().numpy()
    assert np.array_equal(tm[iu, ju], fwd)
    assert np.abs(bwd - fwd).max() <= 1e-4, np.abs(bwd - fwd).max()


@pytest.fixture(scope="module")
def model(seeded_sd):
    m = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
    m.load_state_dict(seeded_sd)
    return m.cuda().eval()


def test_structure_scores_after_sample(model):
    B, L, NS = 4, 24, 3
    batch = synth.make_pocket_batch(B, L, 6, seed=41)
    noise = synth.make_noise(B, L, NS, seed=42)
    dev_batch = {k: cu(v) for k, v in batch.items()}
    final = model.sample(dev_batch, num_steps=NS, noise=noise)[-1]
    g = batch["generate_mask"][0].numpy()
    x, x1 = final["trans"].numpy(), final["trans_1"].numpy()
    s, s1 = final["seqs"].numpy(), final["seqs_1"].numpy()
    tm_ref = np.array([TO.tm_score(x[b][g], x1[b][g])["tm"] for b in range(B)])
    aar = np.array([(s[b][g] == s1[b][g]).mean() for b in range(B)])
    for groups, members in ((None, [list(range(B))]), (torch.tensor([5, 5, 2, 2]), [[2, 3], [0, 1]])):
        sc = metrics.structure_scores(final, dev_batch, groups=groups, novelty_tm=0.3, novelty_ident=0.6)
        tm = sc["tm"].cpu().double().numpy()
        assert np.abs(tm - tm_ref).max() <= 1e-6, (tm, tm_ref)
        assert abs(sc["tm_pooled"].item() - tm.mean()) <= 1e-12
        novel = (tm < 0.3) & (aar < 0.6)
        assert np.array_equal(sc["novel"].cpu().numpy(), novel)
        assert sc["novelty"].shape == (len(members),) and sc["diversity_tm"].shape == (len(members),)
        for gi, mem in enumerate(members):
            assert abs(sc["novelty"][gi].item() - novel[mem].mean()) <= 1e-12
            pr = [(i, j) for i in mem for j in mem if i < j]
            div = 1.0 - np.mean([TO.tm_score(x[i][g], x[j][g])["tm"] for i, j in pr])
            assert abs(sc["diversity_tm"][gi].item() - div) <= 1e-6
    native = dict(final, trans=final["trans_1"])
    sc = metrics.structure_scores(native, dev_batch)
    assert (sc["tm"] - 1.0).abs().max().item() <= 1e-6
