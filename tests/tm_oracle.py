"""numpy float64 restatement of TM-score with a fixed residue correspondence (the TMscore program's search, Zhang & Skolnick 2004),
the specification pf_tm_score_fwd follows: test infrastructure for test_tm_cpu.py / test_gpu_tm.py."""
import numpy as np

N_ITER = 20                 # refinements per seed


def seed_lengths(n):
    """n, n >> 1, ... : a value <= min(4, n) is replaced by min(4, n) and ends the list; after five values min(4, n) is appended"""
    lmin = min(4, n)
    out = []
    for m in range(5):
        v = n >> m
        if v <= lmin:
            out.append(lmin)
            return out
        out.append(v)
    out.append(lmin)
    return out


def d0_of(lnorm):
    return max(0.5, 1.24 * float(np.cbrt(lnorm - 15.0)) - 1.8)


def kabsch(x, y):
    """proper rotation and translation of the least-squares fit y ~ R x + t (unit weights)"""
    xm, ym = x.mean(0), y.mean(0)
    u, _, vt = np.linalg.svd((x - xm).T @ (y - ym))
    d = 1.0 if np.linalg.det(vt.T @ u.T) >= 0 else -1.0
    r = vt.T @ np.diag([1.0, 1.0, d]) @ u.T
    return r, ym - r @ xm


def dist2(x, y, r, t):
    e = x @ r.T + t - y
    return (e * e).sum(1)


def score(x, y, r, t, d0, lnorm):
    """sum 1 / (1 + (d / d0)^2) / lnorm, written d0^2 / (d0^2 + d^2) as the kernel does"""
    d0sq = d0 * d0
    return float((d0sq / (d0sq + dist2(x, y, r, t))).sum() / lnorm)


def cut(d2, d, n):
    """indices with distance < d (compared as d^2 < d * d); d raised by 0.5 while fewer than 3 and n > 3"""
    while True:
        sel = np.nonzero(d2 < d * d)[0]
        if len(sel) >= 3 or n <= 3:
            return sel
        d += 0.5


def tm_score(x, y, mx=None, my=None):
    """x (model), y (target) [N,3]; masks [N] (default all).  -> dict(tm, n_ali, lnorm, d0, rot, trans, seeds (the seed lengths),
    n_cand (superpositions scored)).  tm is NaN (rot / trans None) when fewer than 3 points are aligned."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    mx = np.ones(len(x), bool) if mx is None else np.asarray(mx, bool)
    my = np.ones(len(y), bool) if my is None else np.asarray(my, bool)
    idx = np.nonzero(mx & my)[0]
    n, lnorm = len(idx), int(my.sum())
    out = dict(n_ali=n, lnorm=lnorm, tm=float("nan"), rot=None, trans=None, seeds=seed_lengths(n), n_cand=0)
    if n < 3:
        return out
    X, Y = x[idx], y[idx]
    d0 = d0_of(lnorm)
    d0s = min(max(d0, 4.5), 8.0)
    out["d0"] = d0
    best = -1.0
    for ls in out["seeds"]:
        for s in range(n - ls + 1):
            sel = np.arange(s, s + ls)
            for it in range(N_ITER + 1):
                r, t = kabsch(X[sel], Y[sel])
                d2 = dist2(X, Y, r, t)
                d0sq = d0 * d0
                sc = float((d0sq / (d0sq + d2)).sum() / lnorm)
                out["n_cand"] += 1
                if sc > best:
                    best, out["rot"], out["trans"] = sc, r, t
                if it == N_ITER:
                    break
                new = cut(d2, d0s - 1.0 if it == 0 else d0s + 1.0, n)
                if it > 0 and np.array_equal(new, sel):
                    break
                sel = new
                if len(sel) < 3:
                    break
    out["tm"] = best
    return out


def rigid(rng):
    """a random proper rotation"""
    q = rng.standard_normal(4)
    a, b, c, d = q / np.linalg.norm(q)
    return np.array([[a*a+b*b-c*c-d*d, 2*(b*c-a*d), 2*(b*d+a*c)], [2*(b*c+a*d), a*a-b*b+c*c-d*d, 2*(c*d-a*b)],
                     [2*(b*d-a*c), 2*(c*d+a*b), a*a-b*b-c*c+d*d]])
