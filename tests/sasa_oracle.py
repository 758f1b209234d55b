"""numpy float64 restatement of pf_sasa_fwd's conventions (csrc/sasa.hip): Shrake-Rupley solvent-accessible surface of one structure.

  Atoms     slots 0 .. min(A, 15) - 1 of pos [N,A,3] (fp32); an atom exists where mask is set and radius [21,15] (fp32, indexed by the
            residue type, a type outside 0..19 reading row 20, and the slot) is non-zero.
  Points    the fp32 table points [P,3] (geometry.sphere_points), its values taken as they are.
  Test      R_a = radius_a + probe rounded to fp32.  Point k of atom a is buried by atom b when b != a, b exists, and
            |d + R_a u_k| < R_b, with d = x_a - x_b formed in fp32 from the fp32 coordinates and everything after it in float64.
  Outputs   count [N,15] accessible points, sasa_atom = 4 pi R_a^2 count / P, sasa_residue, sasa_total; an absent atom 0.
  group     [N] zero / non-zero: the *_own outputs use only atoms of residues of a's own group as partners.
  query     [N]: only atoms of query residues are evaluated (every existing atom is a partner); an existing atom that is not
            evaluated has count -1 and area 0.
  marginal  [N,15] (and marginal_own): the atom's points whose decisive margin | |d + R_a u_k| - R_b | is below EPS_FACTOR * 2^-23 * 2 *
            (max radius + probe): the decisive partner is the one that would flip the point's state, the deepest burier of a buried
            point, the nearest surface of an accessible one.  An fp32 evaluation of the test may decide those points either way."""
import numpy as np

SLOTS = 15
EPS_FACTOR = 32.0


def margin_eps(radius, probe):
    return EPS_FACTOR * 2.0 ** -23 * 2.0 * (float(np.max(radius)) + float(np.float32(probe)))


def sasa(pos, mask, aa, radius, points, probe=1.4, query=None, group=None, eps=None):
    pos = np.asarray(pos, np.float32)
    N, A = pos.shape[:2]
    S = min(A, SLOTS)
    P = len(points)
    u = np.asarray(points, np.float32).astype(np.float64)
    aa = np.asarray(aa)
    rows = np.where((aa < 0) | (aa > 20), 20, aa)
    rad = np.asarray(radius, np.float32)[rows][:, :S]
    exists = np.asarray(mask, bool)[:, :S] & (rad > 0)
    R32 = (rad + np.float32(probe)).astype(np.float32)
    eps = margin_eps(radius, probe) if eps is None else eps
    grp = np.zeros(N, bool) if group is None else np.asarray(group) != 0
    evaluated = np.ones(N, bool) if query is None else np.asarray(query) != 0

    # flat list of the existing atoms
    res, slot = np.nonzero(exists)
    X32 = pos[res, slot]
    R = R32[res, slot].astype(np.float64)
    G = grp[res]
    out = {k: np.zeros((N, SLOTS), np.int64) for k in ("count", "marginal", "count_own", "marginal_own")}
    for i in range(len(res)):
        n, s = res[i], slot[i]
        if not evaluated[n]:
            out["count"][n, s] = out["count_own"][n, s] = -1
            continue
        d = (X32[i] - X32).astype(np.float64)                 # fp32 differences, taken as they are
        near = np.sqrt((d * d).sum(1)) < R[i] + R + 1e-3       # the others are further than 1e-3 from every point: never decisive
        near[i] = False
        for tag, part in (("", near), ("_own", near & (G == G[i]))):
            if part.any():
                q = d[part][:, None, :] + R[i] * u[None, :, :]
                depth = (R[part][:, None] - np.sqrt((q * q).sum(-1))).max(0)        # > 0: buried by the deepest partner
            else:
                depth = np.full(P, -np.inf)
            out["count" + tag][n, s] = int((depth <= 0).sum())
            out["marginal" + tag][n, s] = int((np.abs(depth) < eps).sum())
    area = 4.0 * np.pi * np.where(exists, R32.astype(np.float64), 0.0) ** 2 / P
    area = np.concatenate([area, np.zeros((N, SLOTS - S))], 1)
    for tag in ("", "_own"):
        c = np.maximum(out["count" + tag], 0)
        out["sasa_atom" + tag] = area * c
        out["sasa_residue" + tag] = out["sasa_atom" + tag].sum(1)
        out["sasa_total" + tag] = float(out["sasa_atom" + tag].sum())
    out["sphere"] = area            # 4 pi R_a^2 / P per atom: sasa_atom = sphere * count
    out["exists"] = np.concatenate([exists, np.zeros((N, SLOTS - S), bool)], 1)
    if group is None:
        for k in [k for k in out if k.endswith("_own")]:
            del out[k]
    return out
