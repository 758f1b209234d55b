"""numpy float64 restatement of the structural-violation checks of csrc/violations.hip (AlphaFold's between-residue violations with
the conventions of OpenFold's between_residue_clash_loss, between_residue_bond_loss and extreme_ca_ca_distance_violations), with
`query` and `group`.  One sample at a time, dense over the atom pairs (in blocks of rows), so it is test infrastructure only.

Besides the outputs it returns what the comparisons need: the number of nonzero terms behind every float (`*_terms`) and the
distance of every flag from its threshold (`*_margin`, inf where nothing was tested)."""
import numpy as np

SLOTS = 14
VDW = {"C": 1.7, "N": 1.55, "O": 1.52, "S": 1.8}
CA_CA, CA_CA_TOL = 3.80209737096, 1.5
CN_LEN, CN_SD = (1.329, 1.341), (0.014, 0.016)
COS_CA_C_N, COS_C_N_CA, COS_C_N_CA_SD = -0.4473, -0.5203, 0.0353


def flag_margin(over):
    """over [..., K]: how far each tested term is beyond its threshold (> 0: it sets the flag; -inf: not tested) -> how far the
    terms must move to change the flag `any(over > 0)`: the largest excess where it is set, else the smallest shortfall"""
    top = over.max(-1) if over.shape[-1] else np.full(over.shape[:-1], -np.inf)
    return np.abs(top)


def clashes(pos, exists, radius, index, query=None, group=None, tol=1.5, block=64):
    """pos [N,14,3] float64, exists [N,14] bool, radius [N,14] (of existing atoms), index [N] -> dict"""
    N = pos.shape[0]
    x = pos.reshape(N * SLOTS, 3)
    ex = exists.reshape(-1)
    rad = np.where(ex, radius.reshape(-1), 0.0)
    res = np.repeat(np.arange(N), SLOTS)
    slot = np.tile(np.arange(SLOTS), N)
    idx = index.astype(np.int64)[res]
    q = None if query is None else query.astype(bool)[res]
    g = None if group is None else group.astype(bool)[res]
    out = {k: np.zeros(N * SLOTS) for k in ("clash_atom_loss", "clash_atom_loss_cross")}
    out.update({k: np.zeros(N * SLOTS, bool) for k in ("clash_atom", "clash_atom_cross")})
    out.update({k: np.zeros(N * SLOTS, np.int64) for k in ("clash_atom_pairs", "clash_atom_terms", "clash_atom_terms_cross")})
    out.update({k: np.full(N * SLOTS, np.inf) for k in ("clash_atom_margin", "clash_atom_margin_cross")})
    for r0 in range(0, N * SLOTS, block * SLOTS):
        r = slice(r0, min(N * SLOTS, r0 + block * SLOTS))
        m = ex[r, None] & ex[None, :] & (idx[r, None] != idx[None, :])
        m &= ~((slot[r, None] == 2) & (slot[None, :] == 0) & (idx[r, None] + 1 == idx[None, :]))
        m &= ~((slot[r, None] == 0) & (slot[None, :] == 2) & (idx[None, :] + 1 == idx[r, None]))
        m &= ~((slot[r, None] == 5) & (slot[None, :] == 5))
        if q is not None:
            m &= q[r, None] | q[None, :]
        d = np.sqrt(1e-10 + ((x[r, None, :] - x[None, :, :]) ** 2).sum(-1))
        lim = rad[r, None] + rad[None, :] - tol
        e = np.where(m, np.maximum(lim - d, 0.0), 0.0)
        hit = m & (d < lim)
        over = np.where(m, lim - d, -np.inf)                                 # > 0: a hit
        out["clash_atom_loss"][r] = e.sum(1)
        out["clash_atom"][r] = hit.any(1)
        out["clash_atom_pairs"][r] = m.sum(1)
        out["clash_atom_terms"][r] = (e > 0).sum(1)
        out["clash_atom_margin"][r] = flag_margin(over)
        if g is not None:
            c = g[r, None] != g[None, :]
            out["clash_atom_loss_cross"][r] = (e * c).sum(1)
            out["clash_atom_cross"][r] = (hit & c).any(1)
            out["clash_atom_terms_cross"][r] = ((e > 0) & c).sum(1)
            out["clash_atom_margin_cross"][r] = flag_margin(np.where(c, over, -np.inf))
    pairs = out["clash_atom_pairs"].sum() / 2
    res_out = {k: v.reshape(N, SLOTS) for k, v in out.items()}
    res_out["clash_mean_loss"] = 0.5 * out["clash_atom_loss"].sum() / (1e-6 + pairs)
    res_out["clash_mean_terms"] = int(out["clash_atom_terms"].sum() // 2)
    if g is None:
        for k in list(res_out):
            if k.endswith("_cross"):
                del res_out[k]
    return res_out


def connections(pos, mask, index, is_pro, tol_factor=12.0):
    """pos [N,>=3,3] float64, mask [N,>=3] bool, index [N], is_pro [N] bool -> dict"""
    N = pos.shape[0]
    eps = 1e-6
    ca, c, n1, ca1 = pos[:-1, 1], pos[:-1, 2], pos[1:, 0], pos[1:, 1]
    m_ca, m_c, m_n1, m_ca1 = mask[:-1, 1], mask[:-1, 2], mask[1:, 0], mask[1:, 1]
    idx = index.astype(np.int64)
    nogap = (idx[1:] - idx[:-1]) == 1
    dist = lambda p, q: np.sqrt(eps + ((p - q) ** 2).sum(-1))  # noqa: E731
    cn, cac, nca = dist(c, n1), dist(ca, c), dist(n1, ca1)
    pro = is_pro[1:]
    length, sd = np.where(pro, CN_LEN[1], CN_LEN[0]), np.where(pro, CN_SD[1], CN_SD[0])
    e_cn = np.sqrt(eps + (cn - length) ** 2)
    l_cn = np.maximum(e_cn - tol_factor * sd, 0.0)
    k_cn = m_c & m_n1 & nogap
    u_cca, u_cn, u_nca = (ca - c) / cac[:, None], (n1 - c) / cn[:, None], (ca1 - n1) / nca[:, None]
    e_a1 = np.sqrt(eps + ((u_cca * u_cn).sum(-1) - COS_CA_C_N) ** 2)
    l_a1 = np.maximum(e_a1 - tol_factor * CN_SD[0], 0.0)               # the bond-length stddev: loss.py:807
    k_a1 = m_ca & m_c & m_n1 & nogap
    e_a2 = np.sqrt(eps + ((-u_cn * u_nca).sum(-1) - COS_C_N_CA) ** 2)
    l_a2 = np.maximum(e_a2 - tol_factor * COS_C_N_CA_SD, 0.0)
    k_a2 = m_c & m_n1 & m_ca1 & nogap
    mean = lambda l, k: (l * k).sum() / (k.sum() + eps)  # noqa: E731
    per = l_cn + l_a1 + l_a2
    pad = lambda v, fill: (np.concatenate([v, [fill]]), np.concatenate([[fill], v]))  # noqa: E731
    a, b = pad(per, 0.0)
    viol = (k_cn & (e_cn > tol_factor * sd)) | (k_a1 & (e_a1 > tol_factor * CN_SD[0])) | (k_a2 & (e_a2 > tol_factor * COS_C_N_CA_SD))
    va, vb = pad(viol, False)
    over = np.stack([np.where(k_cn, e_cn - tol_factor * sd, -np.inf), np.where(k_a1, e_a1 - tol_factor * CN_SD[0], -np.inf),
                     np.where(k_a2, e_a2 - tol_factor * COS_C_N_CA_SD, -np.inf)], -1)
    oa, ob = np.concatenate([over, np.full((1, 3), -np.inf)]), np.concatenate([np.full((1, 3), -np.inf), over])
    k_caca = m_ca & m_ca1 & nogap
    caca = dist(ca, ca1)
    brk = k_caca & (caca - CA_CA > CA_CA_TOL)
    ta, tb = pad((per > 0).astype(np.int64), 0)
    return {"bond_c_n_loss_mean": mean(l_cn, k_cn), "angle_ca_c_n_loss_mean": mean(l_a1, k_a1), "angle_c_n_ca_loss_mean": mean(l_a2, k_a2),
            "bond_c_n_terms": int(((l_cn > 0) & k_cn).sum()), "angle_ca_c_n_terms": int(((l_a1 > 0) & k_a1).sum()),
            "angle_c_n_ca_terms": int(((l_a2 > 0) & k_a2).sum()),
            "connection_loss": 0.5 * (a + b), "connection_terms": 3 * (ta + tb), "connection_violation": va | vb,
            "connection_margin": flag_margin(np.concatenate([oa, ob], -1)),
            "ca_ca_break": pad(brk, False)[0], "ca_ca_margin": pad(np.where(k_caca, np.abs(caca - CA_CA - CA_CA_TOL), np.inf), np.inf)[0],
            "ca_ca_extreme": brk.sum() / (1e-4 + k_caca.sum())}


def violations(pos, atom_mask, aa, index, radius_table, pro, query=None, group=None, tol_factor=12.0, clash_tol=1.5):
    """One sample: pos [N,A,3] (A >= 14), atom_mask [N,A], aa [N] in the package's numbering, index [N], radius_table [21,14] ->
    the outputs of pf_violations_fwd in float64 plus `*_terms` and `*_margin`."""
    pos = np.asarray(pos, np.float64)[:, :SLOTS]
    atom_mask = np.asarray(atom_mask).astype(bool)[:, :SLOTS]
    aa = np.asarray(aa)
    t = np.where((aa < 0) | (aa > 20), 20, aa)
    radius = np.asarray(radius_table, np.float64)[t]
    exists = atom_mask & (radius > 0)
    if pos.shape[0] == 0:
        raise ValueError("no residues")
    out = clashes(pos, exists, radius, np.asarray(index), query, group, clash_tol)
    out.update(connections(pos, atom_mask, np.asarray(index), aa == pro, tol_factor))
    return out
