"""numpy restatement of pf_cluster_fwd (csrc/clustering.hip): gromos clustering (Daura et al. 1999) and single / complete / average
linkage cut at a height, with the kernel's exact rules, so that every integer output can be compared with array_equal.

Rules (positions are ranks inside a group; d(a, b) for a < b is dist[index[a], index[b]], the entry right of the diagonal only):
  NaN is +inf; the cutoff is cast to float32 (+inf: the largest float32), so neither is ever within it;
  gromos    neighbours d <= cutoff in float32, self included; the active sample with the most active neighbours, of equal counts the
            smallest position, leaves with them; labels in extraction order; representative = that centre;
  linkage   the pair of clusters (i < j, named by their smallest positions) with the smallest linkage distance, of equal distances the
            lexicographically smallest, merges while that distance is <= cutoff; single min, complete max (float32), average
            (n_i d_ik + n_j d_jk) / (n_i + n_j) in float64; labels by size descending, then smallest position; representative = the
            medoid, sums in float64 in ascending position, of equal sums the smallest position;
  best      lowest score of the cluster, NaN last, of equal scores the smallest position.
Each method has a plain loop form (`vectorised=False`) and a vectorised form; tests/test_cluster_cpu.py holds them against each other
and the linkages against scipy."""
import numpy as np

METHODS = ("gromos", "single", "complete", "average")
F32_MAX = np.finfo(np.float32).max


def cutoff32(cutoff):
    return np.float32(min(float(cutoff), float(F32_MAX)))


def group_matrix(dist, index):
    """the group's symmetric float32 matrix from the entries right of the diagonal only, NaN -> +inf, diagonal 0"""
    index = np.asarray(index, dtype=np.int64)
    sub = np.asarray(dist, dtype=np.float32)[np.ix_(index, index)]
    n = len(index)
    d = np.full((n, n), np.float32(0))
    iu = np.triu_indices(n, 1)
    d[iu] = sub[iu]
    d.T[iu] = sub[iu]
    d[np.isnan(d)] = np.inf
    return d


def neighbours(d, cutoff):
    nb = d <= cutoff32(cutoff)
    np.fill_diagonal(nb, True)
    return nb


def gromos_loop(d, cutoff):
    n = d.shape[0]
    c32 = cutoff32(cutoff)
    active = [True] * n
    label, size, rep = [-1] * n, [0] * n, [-1] * n
    k = 0
    while any(active):
        best_c, best_p = -1, -1
        for i in range(n):
            if not active[i]:
                continue
            c = 0
            for j in range(n):
                if active[j] and (i == j or d[i, j] <= c32):
                    c += 1
            if c > best_c:
                best_c, best_p = c, i
        for j in range(n):
            if active[j] and (j == best_p or d[best_p, j] <= c32):
                active[j] = False
                label[j], size[j], rep[j] = k, best_c, best_p
        k += 1
    return np.array(label), np.array(size), np.array(rep), k


def gromos_vec(d, cutoff):
    n = d.shape[0]
    nb = neighbours(d, cutoff)
    active = np.ones(n, dtype=bool)
    label, size, rep = np.full(n, -1), np.zeros(n, dtype=np.int64), np.full(n, -1)
    k = 0
    while active.any():
        counts = np.where(active, (nb & active[None, :]).sum(1), -1)
        p = int(np.argmax(counts))                  # the first of the largest: the smallest position
        mem = nb[p] & active
        label[mem], size[mem], rep[mem] = k, counts[p], p
        active &= ~mem
        k += 1
    return label, size, rep, k


def _update(method, di, dj, ni, nj):
    if method == "single":
        return np.minimum(di, dj)
    if method == "complete":
        return np.maximum(di, dj)
    return (ni * di + nj * dj) / np.float64(ni + nj)


def linkage_loop(d, cutoff, method):
    """-> (root [n]: the smallest position of each sample's cluster, heights of the merges made, the first height refused or +inf)"""
    n = d.shape[0]
    c = np.float64(cutoff32(cutoff))
    D = d.astype(np.float64 if method == "average" else np.float32).copy()
    alive = [True] * n
    cnt = [1] * n
    root = list(range(n))
    heights = []
    while True:
        best, bi, bj = None, -1, -1
        for i in range(n):
            if not alive[i]:
                continue
            for j in range(i + 1, n):
                if alive[j] and (best is None or D[i, j] < best):
                    best, bi, bj = D[i, j], i, j
        if best is None:
            return np.array(root), heights, np.inf
        if not np.float64(best) <= c:
            return np.array(root), heights, float(best)
        heights.append(float(best))
        for k in range(n):
            if alive[k] and k != bi and k != bj:
                D[bi, k] = D[k, bi] = _update(method, D[bi, k], D[bj, k], cnt[bi], cnt[bj])
        alive[bj] = False
        cnt[bi] += cnt[bj]
        root = [bi if r == bj else r for r in root]


def linkage_vec(d, cutoff, method):
    n = d.shape[0]
    c = np.float64(cutoff32(cutoff))
    W = d.astype(np.float64 if method == "average" else np.float32).copy()
    inf = W.dtype.type(np.inf)
    U = np.where(np.triu(np.ones((n, n), dtype=bool), 1), W, inf)      # the candidates: i < j, both alive
    cnt = np.ones(n, dtype=np.int64)
    root = np.arange(n)
    heights = []
    for _ in range(n - 1):
        flat = int(np.argmin(U))                    # the first of the smallest in row-major order: the smallest (i, j)
        i, j = divmod(flat, n)
        h = U[i, j]
        if not np.float64(h) <= c:
            return root, heights, float(h)
        heights.append(float(h))
        new = _update(method, W[i], W[j], int(cnt[i]), int(cnt[j])).astype(W.dtype)
        W[i, :] = W[:, i] = new
        W[j, :] = W[:, j] = inf
        U[i, i + 1:] = new[i + 1:]
        U[:i, i] = new[:i]
        U[i, j] = U[j, :] = U[:, j] = inf
        cnt[i] += cnt[j]
        root[root == j] = i
    return root, heights, np.inf


def linkage_labels(d, root, vectorised=True):
    """-> (label, size, representative) from the clusters' roots: by size descending then root; medoids"""
    n = d.shape[0]
    roots = sorted(set(int(r) for r in root))
    members = {r: [p for p in range(n) if root[p] == r] for r in roots}
    order = sorted(roots, key=lambda r: (-len(members[r]), r))
    label, size, rep = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for k, r in enumerate(order):
        mem = members[r]
        if vectorised:
            m = np.array(mem)
            sums = np.zeros(len(mem), dtype=np.float64)
            for q in mem:                           # serially in ascending position; adding 0.0 for q == p changes nothing
                sums = sums + np.where(m == q, 0.0, d[m, q].astype(np.float64))
        else:
            sums = []
            for p in mem:
                s = np.float64(0.0)
                for q in mem:
                    if q != p:
                        s = s + np.float64(d[p, q])
                sums.append(s)
            sums = np.array(sums)
        medoid = mem[int(np.argmin(sums))]          # the first of the smallest: the smallest position
        label[mem], size[mem], rep[mem] = k, len(mem), medoid
    return label, size, rep


def best_by_score(label, score, n_clusters):
    """-> per sample the position of its cluster's lowest score: NaN last, of equal scores the smallest position"""
    best = np.zeros(len(label), dtype=np.int64)
    for k in range(n_clusters):
        mem = np.flatnonzero(label == k)
        bq, bs = -1, np.float32(0)
        for q in mem:
            s = np.float32(score[q])
            if bq < 0 or (not np.isnan(s) and (np.isnan(bs) or s < bs)):
                bq, bs = q, s
        best[mem] = bq
    return best


def cluster_group(d, cutoff, method, score=None, vectorised=True):
    """one group from its prepared matrix d (group_matrix) -> dict with positions for representative / best"""
    if method == "gromos":
        label, size, rep, k = (gromos_vec if vectorised else gromos_loop)(d, cutoff)
        heights, refused = [], np.inf
    else:
        root, heights, refused = (linkage_vec if vectorised else linkage_loop)(d, cutoff, method)
        label, size, rep = linkage_labels(d, root, vectorised)
        k = int(label.max()) + 1
    out = {"label": label, "cluster_size": size, "representative": rep, "n_neighbours": neighbours(d, cutoff).sum(1),
           "n_clusters": k, "heights": heights, "refused": refused}
    if score is not None:
        out["best"] = best_by_score(label, np.asarray(score, dtype=np.float32), k)
    return out


def cluster(dist, index, offsets, cutoff, method, score=None, vectorised=True):
    """the whole batch, as pf_cluster_fwd writes it: outputs at the batch indices, representative / best as batch indices"""
    dist = np.asarray(dist, dtype=np.float32)
    index, offsets = np.asarray(index, dtype=np.int64), np.asarray(offsets, dtype=np.int64)
    B, G = dist.shape[0], len(offsets) - 1
    out = {k: np.zeros(B, dtype=np.int32) for k in ("label", "cluster_size", "representative", "n_neighbours")}
    if score is not None:
        out["best"] = np.zeros(B, dtype=np.int32)
    out["n_clusters"] = np.zeros(G, dtype=np.int32)
    out["heights"], out["refused"] = [], []
    for g in range(G):
        idx = index[offsets[g]:offsets[g + 1]]
        o = cluster_group(group_matrix(dist, idx), cutoff, method, None if score is None else np.asarray(score)[idx], vectorised)
        for k in ("label", "cluster_size", "n_neighbours"):
            out[k][idx] = o[k]
        out["representative"][idx] = idx[o["representative"]]
        if score is not None:
            out["best"][idx] = idx[o["best"]]
        out["n_clusters"][g] = o["n_clusters"]
        out["heights"] += o["heights"]
        out["refused"].append(o["refused"])
    return out


def index_offsets(groups):
    """groups [B] (None-free integer labels) -> (index, offsets, sorted labels), as geometry.cluster builds them"""
    groups = np.asarray(groups).reshape(-1)
    labels, inv, counts = np.unique(groups, return_inverse=True, return_counts=True)
    return np.argsort(inv, kind="stable"), np.concatenate([[0], np.cumsum(counts)]), labels
