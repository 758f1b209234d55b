"""A plain numpy float64 restatement of DSSP (Kabsch & Sander, Biopolymers 22, 2577, 1983) with the DSSP 2.x conventions that
pf_dssp_fwd follows (include/pepflow_hip.h, pepflowww_amd/csrc/dssp.hip).  Written from the paper and those conventions; the
reference itself calls mdtraj, which is not a dependency here.

Two entry points, so that the pattern rules can be checked from hand-made bond lists:
  hbonds(bb, mask, chain, pro) -> the H-bond stage: breaks, each donor's two best acceptors, the bond matrix;
  assign(bonds, breaks, ca)    -> the pattern stage: turns, bridges, ladders and bulges, helices, T and S -> 8-state codes.
`dssp(...)` runs both, and reports the chain's smallest margin to a threshold."""
import math

import numpy as np

SYMBOLS = "HBEGITS-"                     # SSTRUCT_SYMB_TO_INDEX of pepflow/modules/protein/dssp.py: H 0, B 1, ..., '-' 7
H, B, E, G, I, T, S, LOOP = range(8)
MASKED = 255
PI_PRECEDENCE = True                     # PF_DSSP_PI_PRECEDENCE: DSSP >= 2.1, a pi-helix may overwrite H

Q = 0.084 * 332.0                        # kcal/mol: q1 q2 f of Kabsch & Sander
HB_MAX = -0.5                            # a bond needs E < HB_MAX
HB_MIN = -9.9                            # E for a contact closer than MIN_DIST, and the floor of E
MIN_DIST = 0.5
CA_CUT = 9.0                             # E is computed only for CA-CA < CA_CUT
CN_BREAK = 2.5                           # |C(i-1) - N(i)| > CN_BREAK breaks the chain
BEND_DEG = 70.0


def _dist(p, q):
    """|p - q| over the last axis, in the kernel's order of operations"""
    d = p - q
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def breaks_of(bb, mask, chain=None):
    """-> (brk [N] bool: a segment starts at i, margin |d_CN - 2.5| over the tested pairs).  brk[0] is True; brk[i] where either of
    i - 1, i is masked, the chain ids differ, or |C(i-1) - N(i)| > 2.5."""
    bb = np.asarray(bb, np.float64)
    mask = np.asarray(mask, bool)
    n = len(mask)
    chain = np.zeros(n, np.int64) if chain is None else np.asarray(chain)
    brk = np.ones(n, bool)
    margin = math.inf
    if n > 1:
        d = _dist(bb[:-1, 2], bb[1:, 0])
        tested = mask[:-1] & mask[1:] & (chain[:-1] == chain[1:])
        brk[1:] = ~tested | (d > CN_BREAK)
        if tested.any():
            margin = float(np.abs(d[tested] - CN_BREAK).min())
    return brk, margin


def hbonds(bb, mask, chain=None, pro=None):
    """bb [N,>=4,3] (N, CA, C, O), mask [N], chain [N] ints (None: one chain), pro [N] bool (None: no proline).

    -> dict: acc [N,2] int (-1: none), energy [N,2] float64 (0 with -1), bonds [N,N] bool (bonds[d, a]: donor d to acceptor a),
    brk [N] bool, margin (the smallest of |E + 0.5|, |d_CA - 9|, |d - 0.5| over the pairs tested, and |d_CN - 2.5|)."""
    bb = np.asarray(bb, np.float64)[:, :4]
    mask = np.asarray(mask, bool)
    n = len(mask)
    pro = np.zeros(n, bool) if pro is None else np.asarray(pro, bool)
    brk, margin = breaks_of(bb, mask, chain)
    Nn, CA, C, O = bb[:, 0], bb[:, 1], bb[:, 2], bb[:, 3]
    acc = np.full((n, 2), -1, np.int64)
    en = np.zeros((n, 2))
    bonds = np.zeros((n, n), bool)
    if n == 0:
        return {"acc": acc, "energy": en, "bonds": bonds, "brk": brk, "margin": margin}
    # H(i) = N(i) + unit(C(i-1) - O(i-1)) x 1 A
    Hp = np.zeros((n, 3))
    v = C[:-1] - O[:-1]
    ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    Hp[1:] = Nn[1:] + v / ln[:, None]
    donor = mask & ~brk & ~pro
    idx = np.arange(n)
    pair = donor[:, None] & mask[None, :] & (idx[None, :] != idx[:, None]) & (idx[None, :] != idx[:, None] - 1)
    dca = _dist(CA[:, None], CA[None, :])
    if pair.any():
        margin = min(margin, float(np.abs(dca[pair] - CA_CUT).min()))
    pair &= dca < CA_CUT
    with np.errstate(divide="ignore", invalid="ignore"):
        r_on = _dist(O[None, :], Nn[:, None])
        r_ch = _dist(C[None, :], Hp[:, None])
        r_oh = _dist(O[None, :], Hp[:, None])
        r_cn = _dist(C[None, :], Nn[:, None])
        e = Q * (((1.0 / r_on + 1.0 / r_ch) - 1.0 / r_oh) - 1.0 / r_cn)
    close = (r_on < MIN_DIST) | (r_ch < MIN_DIST) | (r_oh < MIN_DIST) | (r_cn < MIN_DIST)
    e = np.where(close, HB_MIN, np.maximum(e, HB_MIN))
    if pair.any():
        dmin = np.minimum(np.minimum(r_on, r_ch), np.minimum(r_oh, r_cn))
        margin = min(margin, float(np.abs(e[pair] - HB_MAX).min()), float(np.abs(dmin[pair] - MIN_DIST).min()))
    for d in np.nonzero(donor)[0]:
        cand = np.nonzero(pair[d] & (e[d] < 0.0))[0]               # DSSP keeps energies below its initial 0
        order = cand[np.argsort(e[d, cand], kind="stable")][:2]     # lowest two, ties to the lower acceptor index
        for k, a in enumerate(order):
            acc[d, k], en[d, k] = a, e[d, a]
            bonds[d, a] = e[d, a] < HB_MAX
    return {"acc": acc, "energy": en, "bonds": bonds, "brk": brk, "margin": margin}


def bends(ca, brk):
    """-> (bend [N] bool, margin |kappa - 70|): kappa = the angle between CA(i) - CA(i-2) and CA(i+2) - CA(i), DSSP's, on residues
    2 .. N-3 with no break from i - 2 to i + 2."""
    ca = np.asarray(ca, np.float64)
    n = len(brk)
    seg = np.cumsum(brk)
    bend = np.zeros(n, bool)
    margin = math.inf
    for i in range(2, n - 2):
        if seg[i - 2] != seg[i + 2]:
            continue
        u, w = ca[i] - ca[i - 2], ca[i + 2] - ca[i]
        x = ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) * ((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        c = ((u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]) / math.sqrt(x) if x > 0 else 0.0
        kappa = math.degrees(math.acos(min(1.0, max(-1.0, c))))
        bend[i] = kappa > BEND_DEG
        margin = min(margin, abs(kappa - BEND_DEG))
    return bend, margin


def _bond_matrix(bonds, n):
    if isinstance(bonds, np.ndarray) and bonds.dtype == bool and bonds.shape == (n, n):
        return bonds
    m = np.zeros((n, n), bool)
    for d, a in bonds:
        m[d, a] = True
    return m


def ladders(bm, seg):
    """bridges, then ladders, then bulge joins -> list of dicts (type 'P' | 'A', ib, ie, jb, je, n = bridges), in DSSP's order"""
    n = len(seg)
    ladder_list = []
    if n < 5:
        return ladder_list
    bp = np.zeros((n + 2, n + 2), bool)                                # bp[d + 1, a + 1] = bond(d -> a), False off the chain
    bp[1:-1, 1:-1] = bm
    I, J = np.meshgrid(np.arange(1, n - 1), np.arange(1, n - 1), indexing="ij")
    ok = (J >= I + 3) & (seg[I - 1] == seg[I + 1]) & (seg[J - 1] == seg[J + 1])
    # parallel: bond(i+1 -> j) and bond(j -> i-1), or bond(j+1 -> i) and bond(i -> j-1)
    par = ok & ((bp[I + 2, J + 1] & bp[J + 1, I]) | (bp[J + 2, I + 1] & bp[I + 1, J]))
    # antiparallel: bond(i+1 -> j-1) and bond(j+1 -> i-1), or bond(j -> i) and bond(i -> j)
    anti = ok & ~par & ((bp[I + 2, J] & bp[J + 2, I]) | (bp[J + 1, I + 1] & bp[I + 1, J + 1]))
    for i, j in zip(*np.nonzero(par | anti)):                         # in order of i, then j
        t = "P" if par[i, j] else "A"
        i, j = int(i) + 1, int(j) + 1
        for lad in ladder_list:                                   # continue a ladder: (i-1, j-1) parallel, (i-1, j+1) anti
            if lad["type"] == t and lad["ie"] + 1 == i and ((t == "P" and lad["je"] + 1 == j) or (t == "A" and lad["jb"] - 1 == j)):
                lad["ie"] = i
                if t == "P":
                    lad["je"] = j
                else:
                    lad["jb"] = j
                lad["n"] += 1
                break
        else:
            ladder_list.append({"type": t, "ib": i, "ie": i, "jb": j, "je": j, "n": 1})
    # bulges: DSSP 2.x's pass over the ladders in order of their first i (creation order here), each joined into the first
    # earlier live ladder that takes it; a joined ladder is removed.  Gap on the i strand 1..5, on the j strand >= 0; one of
    # them < 3 and the other < 6.  No break anywhere in the joined spans (DSSP 2.x only compares chain ids there).
    k = 0
    while k < len(ladder_list):
        x = ladder_list[k]
        m = k + 1
        while m < len(ladder_list):
            y = ladder_list[m]
            gi = y["ib"] - x["ie"]
            if gi >= 6:
                break
            gj = y["jb"] - x["je"] if x["type"] == "P" else x["jb"] - y["je"]
            if (y["type"] == x["type"] and seg[min(x["ib"], y["ib"])] == seg[max(x["ie"], y["ie"])]
                    and seg[min(x["jb"], y["jb"])] == seg[max(x["je"], y["je"])] and gi >= 1 and gj >= 0
                    and ((gj < 6 and gi < 3) or gj < 3)):
                x["ie"] = y["ie"]
                if x["type"] == "P":
                    x["je"] = y["je"]
                else:
                    x["jb"] = y["jb"]
                x["n"] += y["n"]
                del ladder_list[m]
                continue
            m += 1
        k += 1
    return ladder_list


def turns(bm, seg):
    """-> turn {3,4,5: [N] bool}: an n-turn at i is a bond from donor i + n to acceptor i with no break from i to i + n"""
    n = len(seg)
    out = {}
    for st in (3, 4, 5):
        t = np.zeros(n, bool)
        for i in range(n - st):
            t[i] = seg[i] == seg[i + st] and bm[i + st, i]
        out[st] = t
    return out


def assign(bonds, breaks, ca=None, mask=None):
    """bonds: [N,N] bool (bonds[d, a]) or a list of (donor, acceptor); breaks [N] bool (a segment starts at i; breaks[0] is taken as
    True); ca [N,3] for the bends (None: no S); mask [N] (None: all; a masked residue is cut off from both neighbours).
    -> (ss [N] uint8, details: turns, ladders, bend)."""
    brk = np.array(breaks, bool)
    n = len(brk)
    mask = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    if n:
        brk[0] = True
        brk |= ~mask
        brk[1:] |= ~mask[:-1]
    seg = np.cumsum(brk)
    bm = _bond_matrix(bonds, n)
    ss = np.full(n, LOOP, np.uint8)
    lads = ladders(bm, seg)
    for lad in lads:                                                   # E over a ladder of > 1 bridge; B never replaces E
        code = E if lad["n"] > 1 else B
        for k in list(range(lad["ib"], lad["ie"] + 1)) + list(range(lad["jb"], lad["je"] + 1)):
            if ss[k] != E:
                ss[k] = code
    tn = turns(bm, seg)
    for i in range(1, n):
        if tn[4][i - 1] and tn[4][i]:
            ss[i:i + 4] = H
    for i in range(1, n):
        if tn[3][i - 1] and tn[3][i] and all(ss[k] in (LOOP, G) for k in range(i, i + 3)):
            ss[i:i + 3] = G
    free5 = (LOOP, I, H) if PI_PRECEDENCE else (LOOP, I)
    for i in range(1, n):
        if tn[5][i - 1] and tn[5][i] and all(ss[k] in free5 for k in range(i, i + 5)):
            ss[i:i + 5] = I
    bend = bends(ca, brk)[0] if ca is not None else np.zeros(n, bool)
    for i in range(n):
        if ss[i] != LOOP:
            continue
        if any(i - k >= 0 and tn[st][i - k] for st in (3, 4, 5) for k in range(1, st)):
            ss[i] = T
        elif bend[i]:
            ss[i] = S
    ss[~mask] = MASKED
    return ss, {"turns": tn, "ladders": lads, "bend": bend}


def dssp(bb, mask, chain=None, pro=None):
    """the whole pipeline on one chain slot -> dict: ss [N] uint8, acc, energy, bonds, brk, margin"""
    hb = hbonds(bb, mask, chain, pro)
    ca = np.asarray(bb, np.float64)[:, 1]
    ss, info = assign(hb["bonds"], hb["brk"], ca, mask)
    margin = min(hb["margin"], bends(ca, hb["brk"])[1])
    return dict(hb, ss=ss, margin=margin, **info)


def to_string(ss):
    return "".join("." if c == MASKED else SYMBOLS[c] for c in ss)
