"""numpy float64 restatement of TM-align (Zhang & Skolnick, Nucleic Acids Res. 2005) on CA coordinates: the specification
pf_tm_align_fwd follows (csrc/tm_align.hip lists the conventions), test infrastructure for test_tmalign_cpu.py / test_gpu_tmalign.py.

X (chain 1, the model) is superposed onto Y (chain 2, the target); an alignment is y2x[j] (-1: unaligned).  The pipeline is
TMalign_main without options: gapless threading, secondary structure, local superposition, secondary structure plus superposition,
fragment gapless threading, each followed by a detailed TM search (step 40) and, under the program's conditions, DP_iter; then the
final search (step 1) and the two final TM-scores.  The DP is vectorised along anti-diagonals and over candidates, the TM searches
over seeds, the quick scores over candidates.

`margin` is the smallest gap |a - b| (a != b) over the real-valued decisions taken: DP comparisons, cuts and thresholds, arg-maxima
(the winner against every other candidate), the stage tests and the 1e-6 convergence test.  A result whose margin is below ~1e-9
may differ from another correct fp64 implementation."""
import numpy as np

N_ITER = 20                 # refinements per TM-search seed
GAPS = (-0.6, 0.0)          # DP_iter gap values
STEP_SEARCH = 40            # seed start step of the detailed searches and of DP_iter

SS_C, SS_H, SS_E, SS_T = 0, 1, 2, 3
SS_CHARS = "CHET"


def seed_lengths(n):
    """n, n >> 1, ... : a value <= min(4, n) is replaced by min(4, n) and ends the list; after five values min(4, n) is appended
    (TMscore8_search's L_ini; the same list as tm_oracle.seed_lengths)"""
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


def seed_starts(n, ls, step):
    """0, step, 2 step, ... below n - ls, and n - ls itself"""
    last = n - ls
    out, i = [], 0
    while True:
        out.append(i)
        if i < last:
            i = min(i + step, last)
        else:
            return out


def params_search(lx, ly):
    """parameter_set4search: (d0 (= D0_MIN), d0_search, score_d8, ddcc, lmin)"""
    lmin = min(lx, ly)
    d0 = 0.168 if lmin <= 19 else 1.24 * float(np.cbrt(lmin - 15.0)) - 1.8
    d0 += 0.8
    d0s = min(max(d0, 4.5), 8.0)
    d8 = 1.5 * float(lmin) ** 0.3 + 3.5
    ddcc = 0.1 if lmin <= 40 else 0.4
    return d0, d0s, d8, ddcc, lmin


def params_final(L):
    """parameter_set4final: (d0, d0_search) for normalising by L"""
    d0 = 0.5 if L <= 21 else max(0.5, 1.24 * float(np.cbrt(L - 15.0)) - 1.8)
    return d0, min(max(d0, 4.5), 8.0)


def two_point_rotation(a, b):
    """the canonical rotation of a two-point fit: the smallest rotation taking unit(a) onto unit(b); the identity when either
    vector is zero; a half turn about unit(a x e_k) (k the axis of the smallest |a_k|, the first on ties) when 1 + cos <= 1e-12"""
    na, nb = np.sqrt(a @ a), np.sqrt(b @ b)
    if not (na > 0.0 and nb > 0.0):
        return np.eye(3)
    ua, ub = a / na, b / nb
    c = float(ua @ ub)
    if 1.0 + c <= 1e-12:
        k = int(np.argmin(np.abs(ua)))
        e = np.zeros(3)
        e[k] = 1.0
        n = np.cross(ua, e)
        n = n / np.sqrt(n @ n)
        return 2.0 * np.outer(n, n) - np.eye(3)
    v = np.cross(ua, ub)
    K = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    return np.eye(3) + K + K @ K / (1.0 + c)


def kabsch_b(X, Y, W):
    """proper least-squares fits y ~ R x + t of the rows of W.  X, Y [B,n,3], W [B,n] bool -> R [B,3,3], t [B,3].
    0 points: identity, t = 0; 1 point: identity, t = y - x; 2 points: two_point_rotation of the segment (first -> second);
    >= 3 points with s2 <= 1e-6 s1 (rank < 2, superpose_dev.h's rule): identity; t = mean(y) - R mean(x)."""
    X, Y, W = np.broadcast_arrays(X, Y, W[..., None])
    W = W[..., 0]
    w = W.astype(np.float64)
    c = w.sum(1)
    cs = np.maximum(c, 1.0)[:, None]
    mx = (w[..., None] * X).sum(1) / cs
    my = (w[..., None] * Y).sum(1) / cs
    Cm = np.einsum("bn,bni,bnj->bij", w, X - mx[:, None], Y - my[:, None])
    u, s, vt = np.linalg.svd(Cm)
    d = np.sign(np.linalg.det(np.transpose(vt, (0, 2, 1)) @ np.transpose(u, (0, 2, 1))))
    d[d == 0] = 1.0
    D = np.zeros((len(c), 3, 3))
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = d
    R = np.transpose(vt, (0, 2, 1)) @ D @ np.transpose(u, (0, 2, 1))
    degen = ~(s[:, 0] > 0.0) | (s[:, 1] <= 1e-6 * s[:, 0]) | (c < 3)
    R[degen] = np.eye(3)
    for b in np.nonzero(c == 2)[0]:
        k = np.nonzero(W[b])[0]
        R[b] = two_point_rotation(X[b, k[1]] - X[b, k[0]], Y[b, k[1]] - Y[b, k[0]])
    t = my - np.einsum("bij,bj->bi", R, mx)
    t[c == 0] = 0.0
    return R, t


def apply(R, t, X):
    """R x + t, written as the program's transform(): t + u[r][0] x0 + u[r][1] x1 + u[r][2] x2"""
    return t[..., None, :] + X @ np.swapaxes(R, -1, -2)


def dist2_b(R, t, X, Y):
    e = apply(R, t, X) - Y
    return (e * e).sum(-1)


def sec_str(X):
    """make_sec / sec_str (the unsmoothed form of TM-align 2019+): codes SS_C, SS_H, SS_E, SS_T; margin of the thresholds"""
    L = len(X)
    ss = np.full(L, SS_C, np.int64)
    marg = np.inf
    if L < 5:
        return ss, marg
    i = np.arange(2, L - 2)
    dd = lambda a, b: np.sqrt(((X[i + a] - X[i + b]) ** 2).sum(1))
    d13, d14, d15, d24, d25, d35 = dd(-2, 0), dd(-2, 1), dd(-2, 2), dd(-1, 1), dd(-1, 2), dd(0, 2)
    ds = (d15, d14, d25, d13, d24, d35)
    res = np.full(len(i), SS_C, np.int64)
    for code, ref, delta in ((SS_E, (13.0, 10.4, 10.4, 6.1, 6.1, 6.1), 1.42), (SS_H, (6.37, 5.18, 5.18, 5.45, 5.45, 5.45), 2.1)):
        ok = np.ones(len(i), bool)
        for dv, r in zip(ds, ref):
            g = np.abs(dv - r)
            ok &= g < delta
            e = np.abs(g - delta)
            marg = min(marg, float(e[e > 0].min(initial=np.inf)))
        res[ok] = code                                          # H written last: H wins over E
    turn = (res == SS_C) & (d15 < 8.0)
    e = np.abs(d15 - 8.0)
    marg = min(marg, float(e[e > 0].min(initial=np.inf)))
    res[turn] = SS_T
    ss[2:L - 2] = res
    return ss, marg


class _Run:
    def __init__(self, X, Y):
        self.X, self.Y = X, Y
        self.Lx, self.Ly = len(X), len(Y)
        self.d0, self.d0s, self.d8, self.ddcc, self.lmin = params_search(self.Lx, self.Ly)
        self.margin = np.inf
        self.R, self.t = np.eye(3), np.zeros(3)
        self.stats = dict(dp=0, search=0)

    # ---- margin bookkeeping ----
    def m(self, a, b, where=None):
        e = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
        if where is not None:
            e = e[np.asarray(where, bool)]
        e = e[e > 0]
        if e.size:
            self.margin = min(self.margin, float(e.min()))

    def m_argmax(self, sc, best):
        self.m(sc, best)

    # ---- the threshold raise of score_fun8 / get_score_fast ----
    def cut_d(self, d2, d, n):
        """score_fun8's cut: d2 < (d + 0.5 m)^2 for the least m >= 0 giving >= 3 rows when n > 3 (d2 [B,n], rows may be padded
        with +inf)"""
        thr = np.full(len(d2), d, np.float64)
        cnt = (d2 < thr[:, None] ** 2).sum(1)
        need = (cnt < 3) & (n > 3)
        if need.any():
            third = np.sort(d2[need], 1)[:, 2]
            mm = np.floor((np.sqrt(third) - d) * 2.0) - 1.0
            mm = np.maximum(mm, 0.0)
            for q in range(len(mm)):
                while not (third[q] < (d + 0.5 * mm[q]) ** 2):
                    mm[q] += 1.0
            thr[need] = d + 0.5 * mm
        self.m(d2, (thr ** 2)[:, None], np.isfinite(d2))
        return d2 < thr[:, None] ** 2

    def cut_sq(self, d2, t2, n):
        """get_score_fast's cut: d2 <= t2 + 0.5 m for the least m >= 0 giving >= 3 rows when n > 3 (t2 + 0.5 m evaluated in closed
        form; the program adds 0.5 m times)"""
        thr = np.full(len(d2), t2, np.float64)
        cnt = (d2 <= thr[:, None]).sum(1)
        need = (cnt < 3) & (n > 3)
        if need.any():
            third = np.sort(d2[need], 1)[:, 2]
            mm = np.maximum(np.ceil((third - t2) * 2.0) - 1.0, 0.0)
            for q in range(len(mm)):
                while not (third[q] <= t2 + 0.5 * mm[q]):
                    mm[q] += 1.0
                while mm[q] > 0 and third[q] <= t2 + 0.5 * (mm[q] - 1.0):
                    mm[q] -= 1.0
            thr[need] = t2 + 0.5 * mm
        self.m(d2, thr[:, None], np.isfinite(d2))
        return d2 <= thr[:, None]

    # ---- TMscore8_search ----
    def tm_search(self, xa, ya, step, d8, d0, d0s, lnorm):
        """xa, ya [n,3] the aligned pairs -> (score, R, t); R, t None when n == 0 (score 0).  d8: squared score_d8 cut of
        score_sum_method 8, None for all pairs"""
        self.stats["search"] += 1
        n = len(xa)
        if n == 0:
            return 0.0, None, None
        seeds = [(ls, s) for ls in seed_lengths(n) for s in seed_starts(n, ls, step)]
        B = len(seeds)
        S = np.zeros((B, n), bool)
        for b, (ls, s) in enumerate(seeds):
            S[b, s:s + ls] = True
        act = np.ones(B, bool)
        d02 = d0 * d0
        cand_sc, cand_id, cand_rt = [], [], []
        for it in range(N_ITER + 1):
            ia = np.nonzero(act)[0]
            if ia.size == 0:
                break
            R, t = kabsch_b(xa[None], ya[None], S[ia])
            d2 = dist2_b(R, t, xa[None], ya[None])
            term = 1.0 / (1.0 + d2 / d02)
            if d8 is not None:
                self.m(d2, d8)
                term = np.where(d2 <= d8, term, 0.0)
            sc = term.sum(1) / lnorm
            cand_sc.append(sc)
            cand_id.append(ia * (N_ITER + 1) + it)
            cand_rt.append((R, t))
            if it == N_ITER:
                break
            Sn = self.cut_d(d2, d0s - 1.0 if it == 0 else d0s + 1.0, n)
            same = (Sn == S[ia]).all(1) if it > 0 else np.zeros(len(ia), bool)
            stop = same | (Sn.sum(1) < 3)
            S[ia] = Sn
            act[ia[stop]] = False
        sc = np.concatenate(cand_sc)
        cid = np.concatenate(cand_id)
        best = sc.max()
        self.m_argmax(sc, best)
        k = int(np.nonzero(sc == best)[0][np.argmin(cid[sc == best])])
        off = 0
        for R, t in cand_rt:
            if k < off + len(R):
                return float(best), R[k - off], t[k - off]
            off += len(R)

    def pairs_of(self, y2x):
        j = np.nonzero(y2x >= 0)[0]
        return self.X[y2x[j]], self.Y[j]

    def detailed(self, y2x, step=STEP_SEARCH):
        """TM search on the alignment (score_sum_method 8, search d0, normalised by Lmin); sets the transform"""
        xa, ya = self.pairs_of(y2x)
        sc, R, t = self.tm_search(xa, ya, step, self.d8 * self.d8, self.d0, self.d0s, self.lmin)
        if R is not None:
            self.R, self.t = R, t
        return sc

    # ---- NWDP_TM ----
    def nwdp(self, S, gap):
        """S [B,Lx,Ly] cell scores -> y2x [B,Ly]"""
        self.stats["dp"] += len(S)
        B, Lx, Ly = S.shape
        val = np.zeros((B, Lx + 1, Ly + 1))
        diag = np.zeros((B, Lx + 1, Ly + 1), bool)
        code = np.zeros((B, Lx + 1, Ly + 1), np.int8)
        for k in range(2, Lx + Ly + 1):
            i = np.arange(max(1, k - Ly), min(Lx, k - 1) + 1)
            j = k - i
            d = val[:, i - 1, j - 1] + S[:, i - 1, j - 1]
            h = np.where(diag[:, i - 1, j], val[:, i - 1, j] + gap, val[:, i - 1, j])
            v = np.where(diag[:, i, j - 1], val[:, i, j - 1] + gap, val[:, i, j - 1])
            dg = (d >= h) & (d >= v)
            vh = v >= h
            self.m(d, h)
            self.m(d, v)
            self.m(v, h, ~dg)
            val[:, i, j] = np.where(dg, d, np.where(vh, v, h))
            diag[:, i, j] = dg
            code[:, i, j] = np.where(dg, 0, np.where(vh, 1, 2))
        out = np.full((B, Ly), -1, np.int64)
        for b in range(B):
            c = code[b].tolist()
            i, j = Lx, Ly
            while i > 0 and j > 0:
                q = c[i][j]
                if q == 0:
                    out[b, j - 1] = i - 1
                    i -= 1
                    j -= 1
                elif q == 1:
                    j -= 1
                else:
                    i -= 1
        return out

    def score_tm(self, R, t, d02):
        """[B,Lx,Ly] 1 / (1 + d^2 / d02) under the transforms R [B,3,3], t [B,3]"""
        xx = apply(R, t, self.X[None])                              # [B,Lx,3]
        e = xx[:, :, None, :] - self.Y[None, None]
        return 1.0 / (1.0 + (e * e).sum(-1) / d02)

    # ---- get_score_fast, over candidates ----
    def quick_b(self, y2x):
        """y2x [B,Ly] -> quick scores [B] (not normalised)"""
        B = len(y2x)
        W = y2x >= 0
        XA = self.X[np.maximum(y2x, 0)]
        YA = np.broadcast_to(self.Y[None], XA.shape)
        n = W.sum(1)
        d02 = self.d0 * self.d0
        R, t = kabsch_b(XA, YA, W)
        d2 = np.where(W, dist2_b(R, t, XA, YA), np.inf)
        s0 = np.where(W, 1.0 / (1.0 + d2 / d02), 0.0).sum(1)
        sel = self.cut_sq(d2, self.d0s * self.d0s, n)
        full = sel.sum(1) == n
        R, t = kabsch_b(XA, YA, sel)
        d2 = np.where(W, dist2_b(R, t, XA, YA), np.inf)
        s1 = np.where(W, 1.0 / (1.0 + d2 / d02), 0.0).sum(1)
        sel = self.cut_sq(d2, self.d0s * self.d0s + 1.0, n)
        R, t = kabsch_b(XA, YA, sel)
        d2 = np.where(W, dist2_b(R, t, XA, YA), np.inf)
        s2 = np.where(W, 1.0 / (1.0 + d2 / d02), 0.0).sum(1)
        s1 = np.where(full, s0, s1)
        s2 = np.where(full, s0, s2)
        return np.maximum(np.maximum(s0, s1), s2)

    def pick(self, sc, last):
        """arg-max: the last of equal scores when `last` (>=), else the first (>)"""
        best = sc.max()
        self.m_argmax(sc, best)
        idx = np.nonzero(sc == best)[0]
        return int(idx[-1] if last else idx[0])

    # ---- DP_iter ----
    def dp_iter(self, y2x, gaps, iters):
        best, best_map, old = -1.0, y2x, 0.0
        d02 = self.d0 * self.d0
        for g in gaps:
            for it in range(iters):
                mp = self.nwdp(self.score_tm(self.R[None], self.t[None], d02), g)[0]
                sc = self.detailed(mp)
                self.m(sc, best)
                if sc > best:
                    best, best_map = sc, mp
                if it > 0:
                    self.m(abs(old - sc), 1e-6)
                    if abs(old - sc) < 1e-6:
                        break
                old = sc
        return best, best_map

    # ---- initial alignments ----
    def shifts(self, n1, n2, lx_run, ifr_x=None, ifr_y=None):
        """maps of the gapless shifts k = n1 .. n2 (get_initial / get_initial_fgt)"""
        K = np.arange(n1, n2 + 1)
        maps = np.full((len(K), self.Ly), -1, np.int64)
        if ifr_y is None:                                           # y_j <-> run_x[j + k]
            j = np.arange(self.Ly)
            i = j[None] + K[:, None]
            ok = (i >= 0) & (i < lx_run)
            src = np.arange(lx_run) if ifr_x is None else ifr_x
            maps[ok] = src[i[ok]]
        else:                                                       # run_y[j] <-> x[j + k]
            j = np.arange(len(ifr_y))
            i = j[None] + K[:, None]
            ok = (i >= 0) & (i < self.Lx)
            for b in range(len(K)):
                maps[b, ifr_y[j[ok[b]]]] = i[b, ok[b]]
        return maps

    def get_initial(self):
        min_ali = max(self.lmin // 2, 5)
        n1, n2 = -self.Ly + min_ali, self.Lx - min_ali
        if n1 > n2:
            return self.shifts(n1, n1, self.Lx)[0]
        maps = self.shifts(n1, n2, self.Lx)
        return maps[self.pick(self.quick_b(maps), True)]

    def get_initial_ss(self, ssx, ssy):
        return self.nwdp((ssx[:, None] == ssy[None, :]).astype(np.float64)[None], -1.0)[0]

    def get_initial5(self):
        d01 = max(self.d0 + 1.5, self.d0)
        jumps = []
        for L in (self.Lx, self.Ly):
            jp = 45 if L > 250 else 35 if L > 200 else 25 if L > 150 else 15
            jumps.append(min(jp, L // 3))
        cands = []
        for nf in (min(20, self.lmin // 3), min(100, self.lmin // 2)):
            for i in range(0, self.Lx - nf + 1, jumps[0]):
                for j in range(0, self.Ly - nf + 1, jumps[1]):
                    cands.append((nf, i, j))
        maps, gl = [], []
        for c0 in range(0, len(cands), 16):
            ch = cands[c0:c0 + 16]
            nfm = max(c[0] for c in ch)
            XF = np.zeros((len(ch), nfm, 3))
            YF = np.zeros((len(ch), nfm, 3))
            W = np.zeros((len(ch), nfm), bool)
            for b, (nf, i, j) in enumerate(ch):
                XF[b, :nf], YF[b, :nf], W[b, :nf] = self.X[i:i + nf], self.Y[j:j + nf], True
            R, t = kabsch_b(XF, YF, W)
            mp = self.nwdp(self.score_tm(R, t, d01 * d01), 0.0)
            maps.append(mp)
            gl.append(self.quick_b(mp))
        maps, gl = np.concatenate(maps), np.concatenate(gl)
        if not (gl.max() > 0.0):
            return None
        return maps[self.pick(gl, False)]

    def get_initial_ssplus(self, y2x0, ssx, ssy):
        d01 = max(self.d0 + 1.5, self.d0)
        xa, ya = self.pairs_of(y2x0)
        R, t = kabsch_b(xa[None], ya[None], np.ones((1, len(xa)), bool))
        S = self.score_tm(R, t, d01 * d01) + 0.5 * (ssx[:, None] == ssy[None, :])[None]
        return self.nwdp(S, -1.0)[0]

    def max_frag(self, Z):
        """find_max_frag: (start, end) of the first longest run of consecutive CAs closer than dcu, dcu = dcu0 * 1.1^inc (the
        factor by repeated multiplication) raised until the run reaches min(4, L / 3); at most 1000 raises"""
        L = len(Z)
        d2 = ((Z[1:] - Z[:-1]) ** 2).sum(1)
        r_min = min(4, L // 3)
        f = 1.0
        for inc in range(1001):
            dc = 4.25 * f
            cut = dc * dc
            self.m(d2, cut)
            best, bs, be, j, start = 0, 0, 0, 1, 0
            for i in range(1, L):
                if d2[i - 1] < cut:
                    j += 1
                    if i == L - 1:
                        if j > best:
                            best, bs, be = j, start, i
                        j = 1
                else:
                    if j > best:
                        best, bs, be = j, start, i - 1
                    j = 1
                    start = i
            if best >= r_min:
                break
            f *= 1.1
        return bs, be

    def get_initial_fgt(self, y2x):
        xs, xe = self.max_frag(self.X)
        ys, ye = self.max_frag(self.Y)
        lxf, lyf = xe - xs + 1, ye - ys + 1
        use_x = lxf < lyf or (lxf == lyf and self.Lx <= self.Ly)
        lfr = min(lxf, lyf)
        ifr = (xs if use_x else ys) + np.arange(lfr)
        L0 = min(self.Lx, self.Ly)
        if lfr == L0:                                               # a full-length run: trim 10 % at the ends
            ifr = ifr[int(L0 * 0.1):int(L0 * 0.89) + 1]
            lfr = len(ifr)
        if use_x:
            min_ali = max(int(min(lfr, self.Ly) / 2.5), 3)
            n1, n2 = -self.Ly + min_ali, lfr - min_ali
            if n1 > n2:
                return y2x
            maps = self.shifts(n1, n2, lfr, ifr_x=ifr)
        else:
            min_ali = max(int(min(self.Lx, lfr) / 2.5), 3)
            n1, n2 = -lfr + min_ali, self.Lx - min_ali
            if n1 > n2:
                return y2x
            maps = self.shifts(n1, n2, None, ifr_y=ifr)
        return maps[self.pick(self.quick_b(maps), True)]

    # ---- TMalign_main ----
    def run(self):
        ssx, mgx = sec_str(self.X)
        ssy, mgy = sec_str(self.Y)
        self.margin = min(self.margin, mgx, mgy)
        self.ssx, self.ssy = ssx, ssy
        tmmax = -1.0
        best = self.get_initial()                                   # stage 1 writes the best map directly
        tm = self.detailed(best)
        self.m(tm, tmmax)
        if tm > tmmax:
            tmmax = tm
        stage = [tm]

        def compete(tm, mp):
            nonlocal tmmax, best
            self.m(tm, tmmax)
            if tm > tmmax:
                tmmax, best = tm, mp

        def gate(tm, ratio):
            self.m(tm, ratio * tmmax)
            return tm > ratio * tmmax

        tm, mp = self.dp_iter(best, GAPS, 30)
        compete(tm, mp)
        # stage 2
        inv = self.get_initial_ss(ssx, ssy)
        tm = self.detailed(inv)
        compete(tm, inv)
        stage.append(tm)
        if gate(tm, 0.2):
            tm, inv = self.dp_iter(inv, GAPS, 30)
            compete(tm, inv)
        # stage 3
        m5 = self.get_initial5()
        if m5 is not None:
            inv = m5
            tm = self.detailed(inv)
            compete(tm, inv)
            stage.append(tm)
            if gate(tm, self.ddcc):
                tm, inv = self.dp_iter(inv, GAPS, 2)
                compete(tm, inv)
        else:
            stage.append(float("nan"))
        # stage 4
        inv = self.get_initial_ssplus(best, ssx, ssy)
        tm = self.detailed(inv)
        compete(tm, inv)
        stage.append(tm)
        if gate(tm, self.ddcc):
            tm, inv = self.dp_iter(inv, GAPS, 30)
            compete(tm, inv)
        # stage 5
        inv = self.get_initial_fgt(inv)
        tm = self.detailed(inv)
        compete(tm, inv)
        stage.append(tm)
        if gate(tm, self.ddcc):
            tm, inv = self.dp_iter(inv, GAPS[1:], 2)
            compete(tm, inv)
        self.stage_tm = stage
        self.best = best
        self.tmmax = tmmax

        # stage 6: the final search, the d <= score_d8 pairs, rmsd and the two normalised scores
        self.detailed(best, step=1)
        jj = np.nonzero(best >= 0)[0]
        ii = best[jj]
        d = np.sqrt(dist2_b(self.R, self.t, self.X[ii], self.Y[jj]))
        self.m(d, self.d8)
        keep = d <= self.d8
        ki, kj = ii[keep], jj[keep]
        xa, ya = self.X[ki], self.Y[kj]
        n8 = len(ki)
        out = dict(n_aligned=n8, kept_y=kj, search_R=self.R, search_t=self.t)
        if n8:
            R, t = kabsch_b(xa[None], ya[None], np.ones((1, n8), bool))
            out["rmsd"] = float(np.sqrt(dist2_b(R[0], t[0], xa, ya).sum() / n8))
        else:
            out["rmsd"] = float("nan")
        for key, L in (("tm_x", self.Lx), ("tm", self.Ly)):
            d0, d0s = params_final(L)
            sc, R, t = self.tm_search(xa, ya, 1, None, d0, d0s, L)
            out[key] = sc
            if key == "tm":
                out["rot"], out["trans"] = (R, t) if R is not None else (self.R, self.t)
        return out


def tm_align(x, y, mx=None, my=None):
    """x (chain 1, the model) [N,3], y (chain 2, the target) [M,3], masks (default all).
    -> dict(tm (normalised by Ly: tmtools' tm_norm_chain2), tm_x (by Lx), rmsd, n_aligned, len_x, len_y, y2x [M] (indices into
    x's N positions, -1 unaligned or masked), kept [M] bool, rot, trans (y ~ rot x + trans, the search behind tm), margin,
    ss_x, ss_y (compacted), stage_tm, stats).  NaN scores (and no map) when either chain has fewer than 3 residues."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    mx = np.ones(len(x), bool) if mx is None else np.asarray(mx, bool)
    my = np.ones(len(y), bool) if my is None else np.asarray(my, bool)
    ix, iy = np.nonzero(mx)[0], np.nonzero(my)[0]
    Lx, Ly = len(ix), len(iy)
    nan = float("nan")
    out = dict(tm=nan, tm_x=nan, rmsd=nan, n_aligned=0, len_x=Lx, len_y=Ly, y2x=np.full(len(y), -1, np.int64),
               kept=np.zeros(len(y), bool), rot=None, trans=None, margin=np.inf)
    if Lx < 3 or Ly < 3:
        return out
    r = _Run(x[ix], y[iy])
    res = r.run()
    y2x = np.full(len(y), -1, np.int64)
    j = np.nonzero(r.best >= 0)[0]
    y2x[iy[j]] = ix[r.best[j]]
    kept = np.zeros(len(y), bool)
    kept[iy[res["kept_y"]]] = True
    out.update(tm=res["tm"], tm_x=res["tm_x"], rmsd=res["rmsd"], n_aligned=res["n_aligned"], y2x=y2x, kept=kept,
               rot=res["rot"], trans=res["trans"], margin=r.margin, ss_x=r.ssx, ss_y=r.ssy, stage_tm=r.stage_tm,
               stats=r.stats, tmmax=r.tmmax)
    return out


def final_score(x, y, y2x, Ly, d8=None):
    """the final scoring of an alignment y2x (compacted indices) as tm_align does it: the step-1 search (score_sum_method 8) for
    the transform, the pairs with d <= score_d8, then the step-1 search normalised by Ly -- for enumerating alignments"""
    r = _Run(np.asarray(x, np.float64), np.asarray(y, np.float64))
    y2x = np.asarray(y2x, np.int64)
    r.detailed(y2x, step=1)
    jj = np.nonzero(y2x >= 0)[0]
    ii = y2x[jj]
    d = np.sqrt(dist2_b(r.R, r.t, r.X[ii], r.Y[jj]))
    keep = d <= r.d8
    d0, d0s = params_final(Ly)
    return r.tm_search(r.X[ii[keep]], r.Y[jj[keep]], 1, None, d0, d0s, Ly)[0]
