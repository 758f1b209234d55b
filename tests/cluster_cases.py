"""Inputs of the clustering tests: seeded point clouds around a few centres with their float32 Euclidean distance matrices, the mixed
batch whose groups are interleaved, and small constructed matrices whose answers are written out by hand."""
import numpy as np

SIZES = (1, 2, 3, 63, 64, 65, 130)          # the edges of a 64-bit word and of a wave, and more than one word per row
SCIPY_SIZES = (2, 3, 17, 64, 65, 130)
CUTOFFS = (1.0, 2.0, 3.5)
NAN = float("nan")


def seeded_points(n, seed, centres=4, spread=3.0, noise=0.6):
    rng = np.random.default_rng(seed)
    c = rng.normal(0.0, spread, size=(centres, 3))
    return (c[rng.integers(0, centres, size=n)] + rng.normal(0.0, noise, size=(n, 3))).astype(np.float32)


def distance_matrix(p):
    """float32 Euclidean distances; (a - b)^2 == (b - a)^2 exactly, so the matrix is exactly symmetric"""
    p = np.asarray(p, dtype=np.float32)
    diff = p[:, None, :] - p[None, :, :]
    return np.sqrt((diff * diff).sum(-1, dtype=np.float32), dtype=np.float32)


def seeded_matrix(n, seed=None):
    return distance_matrix(seeded_points(n, 1000 + n if seed is None else seed))


def mixed_batch(sizes=SIZES, seed=7):
    """-> (dist [B,B] float32 with NaN across groups, groups [B], {group label: its own [n,n] matrix}); the groups' members are
    scattered through the batch by a seeded permutation and keep their order inside a group"""
    groups = np.concatenate([np.full(n, 10 * g + 3) for g, n in enumerate(sizes)])
    groups = groups[np.random.default_rng(seed).permutation(len(groups))]
    B = len(groups)
    dist = np.full((B, B), np.nan, dtype=np.float32)
    own = {}
    for g, n in enumerate(sizes):
        lab = 10 * g + 3
        idx = np.flatnonzero(groups == lab)
        own[lab] = seeded_matrix(n)
        dist[np.ix_(idx, idx)] = own[lab]
    return dist, groups, own


def seeded_scores(B, seed=11):
    """scores with exact ties and NaN among them"""
    rng = np.random.default_rng(seed)
    s = np.round(rng.normal(0.0, 2.0, size=B), 0).astype(np.float32)         # whole numbers: many equal scores
    s[rng.random(B) < 0.15] = np.nan
    return s


def matrix(n, entries, fill):
    d = np.full((n, n), fill, dtype=np.float32)
    np.fill_diagonal(d, 0.0)
    for (i, j), v in entries.items():
        d[i, j] = d[j, i] = v
    return d


def line(n):
    x = np.arange(n, dtype=np.float32)
    return np.abs(x[:, None] - x[None, :])


def constructed():
    """-> list of (name, dist [n,n], cutoff, method, expected): expected maps output names to lists over positions (representative as
    a position) and n_clusters to an int; only the keys given are checked"""
    zero, far, ln = np.zeros((5, 5), dtype=np.float32), matrix(5, {}, 9.0), line(7)
    cases = []
    for m in ("gromos", "single", "complete", "average"):
        cases.append(("zero-" + m, zero, 0.0, m, dict(label=[0] * 5, cluster_size=[5] * 5, representative=[0] * 5, n_clusters=1,
                                                      n_neighbours=[5] * 5)))
        cases.append(("far-" + m, far, 2.0, m, dict(label=[0, 1, 2, 3, 4], cluster_size=[1] * 5, representative=[0, 1, 2, 3, 4],
                                                    n_clusters=5, n_neighbours=[1] * 5)))
    # points on a line at spacing 1, cutoff exactly 1.0: the comparison is <=
    cases.append(("line-single", ln, 1.0, "single", dict(label=[0] * 7, cluster_size=[7] * 7, representative=[3] * 7, n_clusters=1)))
    cases.append(("line-complete", ln, 1.0, "complete", dict(label=[0, 0, 1, 1, 2, 2, 3], cluster_size=[2, 2, 2, 2, 2, 2, 1],
                                                             representative=[0, 0, 2, 2, 4, 4, 6], n_clusters=4)))
    # gromos: counts 2 3 3 3 3 3 2 -> centre 1 takes {0,1,2}; then 3:2 4:3 5:3 6:2 -> centre 4 takes {3,4,5}; 6 is left
    cases.append(("line-gromos", ln, 1.0, "gromos", dict(label=[0, 0, 0, 1, 1, 1, 2], cluster_size=[3, 3, 3, 3, 3, 3, 1],
                                                         representative=[1, 1, 1, 4, 4, 4, 6], n_clusters=3,
                                                         n_neighbours=[2, 3, 3, 3, 3, 3, 2])))
    # exact ties: d(0,1) = d(1,2) = 1, d(0,2) = 5.  complete merges the smaller pair (0,1) first, after which 2 is 5 away
    tie3 = matrix(3, {(0, 1): 1.0, (1, 2): 1.0, (0, 2): 5.0}, 5.0)
    cases.append(("tie3-complete", tie3, 1.0, "complete", dict(label=[0, 0, 1], cluster_size=[2, 2, 1], representative=[0, 0, 2],
                                                               n_clusters=2)))
    cases.append(("tie3-average", tie3, 1.0, "average", dict(label=[0, 0, 1], cluster_size=[2, 2, 1], representative=[0, 0, 2],
                                                             n_clusters=2)))
    # single joins all three; the medoid is 1 (sums 6, 2, 6)
    cases.append(("tie3-single", tie3, 1.0, "single", dict(label=[0, 0, 0], cluster_size=[3] * 3, representative=[1] * 3, n_clusters=1)))
    # gromos on a chain of four: counts 2 3 3 2, the tie of 1 and 2 goes to the smaller position
    chain4 = matrix(4, {(0, 1): 1.0, (1, 2): 1.0, (2, 3): 1.0}, 5.0)
    cases.append(("chain4-gromos", chain4, 1.0, "gromos", dict(label=[0, 0, 0, 1], cluster_size=[3, 3, 3, 1],
                                                               representative=[1, 1, 1, 3], n_clusters=2)))
    # two clusters of equal size: the label order falls back to the smallest position
    cases.append(("chain4-complete", chain4, 1.0, "complete", dict(label=[0, 0, 1, 1], cluster_size=[2] * 4,
                                                                   representative=[0, 0, 2, 2], n_clusters=2)))
    # a NaN inside a group is +inf: 0 and 1 are never joined directly
    nan3 = matrix(3, {(0, 1): NAN, (0, 2): 0.5, (1, 2): 0.5}, 0.0)
    cases.append(("nan3-gromos", nan3, 1.0, "gromos", dict(label=[0, 0, 0], cluster_size=[3] * 3, representative=[2] * 3, n_clusters=1,
                                                           n_neighbours=[2, 2, 3])))
    cases.append(("nan3-single", nan3, 1.0, "single", dict(label=[0, 0, 0], cluster_size=[3] * 3, representative=[2] * 3, n_clusters=1)))
    for m in ("complete", "average"):
        cases.append(("nan3-" + m, nan3, 1.0, m, dict(label=[0, 1, 0], cluster_size=[2, 1, 2], representative=[0, 1, 0], n_clusters=2)))
    nan2 = matrix(2, {(0, 1): NAN}, 0.0)
    for m in ("gromos", "single", "complete", "average"):
        cases.append(("nan2-" + m, nan2, float("inf"), m, dict(label=[0, 1], cluster_size=[1, 1], representative=[0, 1], n_clusters=2)))
    return cases


def with_garbage_below(dist, seed=3):
    """the same matrix with the lower triangle (which is never read) overwritten: noise, NaN, negative values and infinities"""
    rng = np.random.default_rng(seed)
    n = dist.shape[0]
    junk = rng.choice(np.array([np.nan, -1.0, 0.0, np.inf, 0.25, 1e30], dtype=np.float32), size=(n, n))
    return np.where(np.tril(np.ones((n, n), dtype=bool), -1), junk, dist).astype(np.float32)
