"""pf_cluster_fwd on the device against the numpy oracle (cluster_oracle.py), which runs on the SAME float32 matrix: every integer
output is compared with array_equal, without a tolerance.  The average linkage's float64 heights are formed in the written order
without contraction on both sides; tests/test_cluster_cpu.py asserts that no height of the inputs used here lies within 1e-6 of a
cutoff, so even a last-bit difference could not move a cut.  The linkages are checked against scipy (as partitions) on the CPU, through
the oracle; gromos follows the publication and is not checked against GROMACS."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import cluster_cases as CC  # noqa: E402
import cluster_oracle as CO  # noqa: E402
import pepflowww_amd  # noqa: E402
from pepflowww_amd import _capi, geometry, metrics, synth  # noqa: E402
from pepflowww_amd.geometry import cluster as _is_there  # noqa: E402,F401

KEYS = ("label", "cluster_size", "representative", "n_neighbours", "n_clusters")


def cu(t):
    return torch.as_tensor(t).cuda()


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def check(out, dist, groups, cutoff, method, score=None):
    """the device outputs against the oracle on the same matrix"""
    got = host(out)
    index, offsets, labels = CO.index_offsets(np.zeros(dist.shape[0], dtype=np.int64) if groups is None else groups)
    assert np.array_equal(got["index"], index) and np.array_equal(got["offsets"], offsets)
    assert np.array_equal(got["group_labels"], labels) and np.array_equal(labels[got["group_of"]], np.zeros(len(index)) if groups is None else groups)
    ref = CO.cluster(dist, index, offsets, cutoff, method, score)
    for k in KEYS + (("best",) if score is not None else ()):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (method, cutoff, k)
    assert ("best" in got) == (score is not None)
    return got


@pytest.fixture(scope="module")
def mixed():
    dist, groups, own = CC.mixed_batch()
    return dist, groups, own, cu(dist)


@pytest.mark.parametrize("cutoff", CC.CUTOFFS)
@pytest.mark.parametrize("method", geometry.CLUSTER_METHODS)
def test_seeded_shapes_match_oracle(mixed, method, cutoff):
    dist, groups, _, dev = mixed
    got = check(geometry.cluster(dev, cutoff, groups=groups, method=method), dist, groups, cutoff, method)
    assert sorted(np.bincount(got["group_of"]).tolist()) == sorted(CC.SIZES)
    print(method, cutoff, "clusters per group", got["n_clusters"].tolist())


@pytest.mark.parametrize("name,dist,cutoff,method,expected", CC.constructed(), ids=[c[0] for c in CC.constructed()])
def test_constructed_cases(name, dist, cutoff, method, expected):
    got = check(geometry.cluster(cu(dist), cutoff, method=method), dist, None, cutoff, method)
    for k, v in expected.items():
        assert np.array_equal(got[k].reshape(-1), np.asarray(v).reshape(-1)), (k, got[k], v)
    dirty = host(geometry.cluster(cu(CC.with_garbage_below(dist)), cutoff, method=method))     # the lower triangle is never read
    for k in KEYS:
        assert np.array_equal(dirty[k], got[k]), k


@pytest.mark.parametrize("method", geometry.CLUSTER_METHODS)
def test_garbage_below_the_diagonal_changes_nothing(mixed, method):
    dist, groups, _, dev = mixed
    clean = host(geometry.cluster(dev, 2.0, groups=groups, method=method))
    dirty = host(geometry.cluster(cu(CC.with_garbage_below(dist)), 2.0, groups=groups, method=method))
    for k in KEYS:
        assert np.array_equal(clean[k], dirty[k]), k


@pytest.mark.parametrize("method", geometry.CLUSTER_METHODS)
def test_best_by_score(mixed, method):
    dist, groups, _, dev = mixed
    score = CC.seeded_scores(len(groups))
    assert np.isnan(score).any() and len(np.unique(score[~np.isnan(score)])) < len(score) // 4      # NaN and equal scores
    got = check(geometry.cluster(dev, 2.0, groups=groups, method=method, score=cu(score)), dist, groups, 2.0, method, score)
    own = got["group_of"][got["best"]] == got["group_of"]
    assert own.all() and np.array_equal(got["label"][got["best"]], got["label"])
    assert "best" not in geometry.cluster(dev, 2.0, groups=groups, method=method)
    # a cluster whose scores are all NaN still names a member: its first
    allnan = np.full(len(groups), np.nan, dtype=np.float32)
    check(geometry.cluster(dev, 2.0, groups=groups, method=method, score=cu(allnan)), dist, groups, 2.0, method, allnan)


@pytest.mark.parametrize("method", ["gromos", "complete"])
def test_the_bound(method):
    n = geometry.CLUSTER_MAX_N
    dist = CC.distance_matrix(CC.seeded_points(n, 4242, centres=24))
    check(geometry.cluster(cu(dist), 2.0, method=method), dist, None, 2.0, method)


@pytest.mark.parametrize("method", geometry.CLUSTER_METHODS)
def test_repeatable_and_independent_of_the_batch(mixed, method):
    dist, groups, own, dev = mixed
    score = CC.seeded_scores(len(groups))
    a = host(geometry.cluster(dev, 2.0, groups=groups, method=method, score=cu(score)))
    b = host(geometry.cluster(dev, 2.0, groups=groups, method=method, score=cu(score)))
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for lab, d in own.items():                      # the same group on its own
        idx = np.flatnonzero(groups == lab)
        alone = host(geometry.cluster(cu(d), 2.0, method=method, score=cu(score[idx])))
        for k in ("label", "cluster_size", "n_neighbours"):
            assert np.array_equal(alone[k], a[k][idx]), (lab, k)
        for k in ("representative", "best"):
            assert np.array_equal(idx[alone[k]], a[k][idx]), (lab, k)
        assert alone["n_clusters"][0] == a["n_clusters"][list(a["group_labels"]).index(lab)]


def round512(n):
    return (n + 511) // 512 * 512


@pytest.mark.parametrize("method", geometry.CLUSTER_METHODS)
def test_chain_with_pairwise_rmsd_and_memory(method):
    """pairwise_superpose_rmsd -> cluster, nothing in between; the call allocates its outputs and the scratch, nothing matrix-sized
    beyond that (the allocator hands out multiples of 512 bytes)"""
    rng = np.random.default_rng(5)
    sizes, N = (40, 25), 12
    base = [rng.normal(0.0, 4.0, size=(3, N, 3)) for _ in sizes]
    x = np.concatenate([b[rng.integers(0, 3, size=n)] + rng.normal(0.0, 0.5, size=(n, N, 3)) for b, n in zip(base, sizes)])
    groups = np.repeat([4, 1], sizes)
    perm = rng.permutation(len(groups))
    x, groups = x[perm].astype(np.float32), groups[perm]
    mask = torch.ones(len(groups), N, dtype=torch.bool).cuda()
    dist = geometry.pairwise_superpose_rmsd(cu(x), mask, groups=groups)
    geometry.cluster(dist, 1.5, groups=groups, method=method)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = geometry.cluster(dist, 1.5, groups=groups, method=method)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    work = len(sizes) * _capi.load().pf_cluster_work_bytes(max(sizes), geometry.CLUSTER_METHODS.index(method))
    allowed = sum(round512(v.numel() * v.element_size()) for v in out.values()) + round512(work)
    assert peak - before <= allowed, (peak - before, allowed)
    got = check(out, dist.cpu().numpy(), groups, 1.5, method)
    assert (got["n_clusters"] >= 1).all() and got["n_clusters"].sum() < len(groups)
    print(method, "clusters", got["n_clusters"].tolist(), "allocated", peak - before, "allowed", allowed)


def test_empty_batch_launches_nothing():
    calls = _capi.CALLS
    out = geometry.cluster(torch.zeros(0, 0).cuda(), 1.0, score=torch.zeros(0).cuda())
    assert _capi.CALLS == calls
    assert all(out[k].shape == (0,) for k in ("label", "cluster_size", "representative", "best", "n_neighbours", "n_clusters", "index"))
    assert out["offsets"].tolist() == [0]


# ---- metrics.cluster_samples -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sampled(seeded_sd):
    model = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
    model.load_state_dict(seeded_sd)
    model = model.cuda().eval()
    B, L, NS = 6, 40, 3
    batch = synth.make_pocket_batch(B, L, 12, seed=81)
    noise = synth.make_noise(B, L, NS, seed=82)
    dev_batch = {k: cu(v) for k, v in batch.items()}
    return model.sample(dev_batch, num_steps=NS, noise=noise)[-1], dev_batch


@pytest.mark.parametrize("metric", metrics.CLUSTER_METRICS)
def test_cluster_samples_after_sample(sampled, metric):
    final, batch = sampled
    groups = np.array([7, 2, 7, 2, 7, 7])
    score = torch.tensor([0.5, float("nan"), -1.0, 2.0, -1.0, 3.0])
    first = metrics.cluster_samples(final, batch, groups=groups, metric=metric)
    d = first["dist"].cpu().numpy()
    same = groups[:, None] == groups[None, :]
    assert np.isfinite(d[same]).all() and np.isnan(d[~same]).all() and np.array_equal(d, d.T, equal_nan=True) and not d.diagonal().any()
    spread = float(np.median(d[same & ~np.eye(6, dtype=bool)]))         # a cutoff that splits these samples
    for cutoff in (None, spread):
        for method in geometry.CLUSTER_METHODS:
            out = metrics.cluster_samples(final, batch, groups=groups, metric=metric, cutoff=cutoff, method=method, score=score.cuda())
            assert torch.equal(out["dist"].view(torch.int32), first["dist"].view(torch.int32))      # bitwise: NaN across groups
            used = metrics.CLUSTER_CUTOFFS[metric] if cutoff is None else cutoff
            again = geometry.cluster(out["dist"], used, groups=groups, method=method, score=score.cuda())
            for k in KEYS + ("best",):
                assert torch.equal(out[k], again[k]), k
            got = check(again, d, groups, used, method, score.numpy())
            lab, rep, best, gof = got["label"], got["representative"], got["best"], got["group_of"]
            sizes = np.bincount(gof)
            assert out["cluster_diversity"].dtype == torch.float64
            assert np.array_equal(out["cluster_diversity"].cpu().numpy(), got["n_clusters"] / sizes)
            for g in range(len(sizes)):                                 # a partition of each group, numbered without gaps
                assert sorted(set(lab[gof == g].tolist())) == list(range(got["n_clusters"][g]))
            assert np.array_equal(gof[rep], gof) and np.array_equal(lab[rep], lab)
            assert np.array_equal(gof[best], gof) and np.array_equal(lab[best], lab)
            s = score.numpy()
            for i in range(6):                                          # the minimum score of the own cluster
                mem = s[(gof == gof[i]) & (lab == lab[i])]
                assert np.isnan(mem).all() or s[best[i]] == np.nanmin(mem)
            print(metric, method, used, "labels", lab.tolist(), "clusters", got["n_clusters"].tolist())
