"""Backbones with known secondary structure for the DSSP tests: NeRF chains with Engh-Huber bond geometry (omega 180, O in the
peptide plane) and strand pairs whose partner is placed by fitting its rigid transform to the intended H-bonds."""
import math

import numpy as np

B_NCA, B_CAC, B_CN, B_CO = 1.458, 1.525, 1.329, 1.231          # A
A_NCAC, A_CACN, A_CNCA, A_CACO = 111.2, 116.2, 121.7, 120.8     # degrees

ALPHA = (-57.8, -47.0)
HELIX_310 = (-49.0, -26.0)
PI = (-57.0, -70.0)
STRAND = (-139.0, 135.0)
BASINS = {"helix": ((-60.0, -45.0), 8.0), "strand": ((-125.0, 130.0), 15.0), "coil": (None, None)}


def place(a, b, c, bond, angle, torsion):
    """NeRF: the atom d with |cd| = bond, angle bcd = angle and dihedral abcd = torsion (degrees)"""
    bc = c - b
    bc /= np.linalg.norm(bc)
    n = np.cross(b - a, bc)
    n /= np.linalg.norm(n)
    m = np.cross(n, bc)
    th, ph = math.radians(angle), math.radians(torsion)
    d2 = np.array([-bond * math.cos(th), bond * math.sin(th) * math.cos(ph), bond * math.sin(th) * math.sin(ph)])
    return c + d2[0] * bc + d2[1] * m + d2[2] * n


def chain(phi, psi, omega=180.0):
    """phi, psi [n] (degrees; phi[0] and psi[-1] only orient O) -> [n,4,3] N, CA, C, O"""
    n = len(phi)
    out = np.zeros((n, 4, 3))
    out[0, 0] = [0.0, 0.0, 0.0]
    out[0, 1] = [B_NCA, 0.0, 0.0]
    t = math.radians(180.0 - A_NCAC)
    out[0, 2] = out[0, 1] + B_CAC * np.array([math.cos(t), math.sin(t), 0.0])
    for i in range(n):
        Nn, CA, C = out[i, 0], out[i, 1], out[i, 2]
        out[i, 3] = place(Nn, CA, C, B_CO, A_CACO, psi[i] + 180.0)
        if i + 1 < n:
            out[i + 1, 0] = place(Nn, CA, C, B_CN, A_CACN, psi[i])
            out[i + 1, 1] = place(CA, C, out[i + 1, 0], B_NCA, A_CNCA, omega)
            out[i + 1, 2] = place(C, out[i + 1, 0], out[i + 1, 1], B_CAC, A_NCAC, phi[i + 1])
    return out


def helix(n, angles):
    return chain(np.full(n, angles[0]), np.full(n, angles[1]))


def rotation(v):
    """rotation vector (radians) -> 3x3"""
    th = float(np.linalg.norm(v))
    if th < 1e-15:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def _hydrogens(bb):
    v = bb[:-1, 2] - bb[:-1, 3]
    h = np.full((len(bb), 3), np.nan)
    h[1:] = bb[1:, 0] + v / np.linalg.norm(v, axis=1, keepdims=True)
    return h


def pair_energy(bb, h, d, a):
    """E of donor d to acceptor a (the DSSP formula, no cut-offs)"""
    Nn, C, O = bb[d, 0], bb[a, 2], bb[a, 3]
    r = lambda p, q: np.linalg.norm(p - q)  # noqa: E731
    return 0.084 * 332 * (1 / r(O, Nn) + 1 / r(C, h[d]) - 1 / r(O, h[d]) - 1 / r(C, Nn))


def fit_partner(s1, s2, wanted, x0):
    """rigid motion (rotation vector, shift) of strand s2 that minimises the summed energy of the `wanted` (donor, acceptor)
    pairs of the joined chain s1 + s2 (indices into it), with a penalty on atoms closer than 3 A across the strands"""
    from scipy.optimize import minimize
    n1 = len(s1)

    def build(p):
        return np.concatenate([s1, s2 @ rotation(p[:3]).T + p[3:]])

    def loss(p):
        bb = build(p)
        h = np.concatenate([_hydrogens(bb[:n1]), _hydrogens(bb[n1:])])
        h[n1] = bb[n1, 0] + (bb[n1 + 1, 0] - bb[n1 + 1, 0])       # no H on a chain start: never a wanted donor
        e = sum(max(pair_energy(bb, h, d, a), -4.0) for d, a in wanted)
        x, y = bb[:n1].reshape(-1, 3), bb[n1:].reshape(-1, 3)
        dd = np.linalg.norm(x[:, None] - y[None], axis=-1)
        return e + 10.0 * np.square(np.clip(3.0 - dd, 0, None)).sum()

    res = minimize(loss, np.asarray(x0, float), method="Powell", options={"xtol": 1e-6, "ftol": 1e-9, "maxfev": 20000})
    return build(res.x)


def strand_pair(kind):
    """two 6-residue strands, chain ids 0 and 1; the partner's rigid motion fitted to the intended bonds"""
    s1 = chain(np.full(6, STRAND[0]), np.full(6, STRAND[1]))
    ca = s1[:, 1]
    u = ca[-1] - ca[0]
    u /= np.linalg.norm(u)
    cd = s1[1, 3] - s1[1, 2]
    cd -= cd @ u * u
    cd /= np.linalg.norm(cd)
    if kind == "anti":
        rv = np.pi * cd
        shift = s1.reshape(-1, 3).mean(0) - (s1.reshape(-1, 3) @ rotation(rv).T).mean(0) + 4.8 * cd
        bb = fit_partner(s1, s1, [(1, 10), (10, 1), (3, 8), (8, 3)], np.r_[rv, shift])
    else:
        bb = fit_partner(s1, s1, [(2, 7), (7, 0), (4, 9), (9, 2)], np.r_[np.zeros(3), -4.8 * cd])
    return bb, np.r_[np.zeros(6), np.ones(6)].astype(np.int64)


def random_chain(rng, n):
    """NeRF chain with phi / psi drawn per segment (3 - 12 residues) from the helix, strand or coil basins"""
    phi, psi = np.zeros(n), np.zeros(n)
    k = 0
    while k < n:
        m = min(n - k, int(rng.integers(3, 13)))
        kind = rng.choice(list(BASINS))
        if kind == "coil":
            phi[k:k + m] = rng.uniform(-170, -50, m)
            psi[k:k + m] = rng.uniform(-60, 170, m)
        else:
            (p0, s0), sd = BASINS[kind]
            phi[k:k + m] = p0 + sd * rng.standard_normal(m)
            psi[k:k + m] = s0 + sd * rng.standard_normal(m)
        k += m
    return chain(phi, psi)
