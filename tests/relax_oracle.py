"""numpy restatement of the restraint force field of csrc/relax.hip, of its analytic gradient and of the monotone minimiser around
it: test infrastructure.  One structure at a time; `dtype` switches every per-atom operation between float64 (the oracle) and float32
(the same code at the kernel's precision, which the replay test uses to size its tolerance).  The per-structure sums are float64
either way.  The tables are the package's own (geometry.sasa_radius_table, geometry.restrained_pair_table), which test_relax_cpu.py
checks on their own; everything else is stated here."""
import numpy as np

SLOTS = 15
TERMS = ("rest", "intra", "conn", "clash")
DEFAULTS = dict(k_rest=10.0, k_intra=300.0, k_bond=300.0, k_angle=150.0, k_clash=200.0, clash_overlap_tolerance=1.5, clash_margin=0.2,
                step0=0.002, gtol=0.0)
CN_LEN, CN_LEN_PRO, COS_CA_C_N, COS_C_N_CA = 1.329, 1.341, -0.4473, -0.5203
PRO = 12
ALPHA_MAX = 1e3            # the cap of the step size
_TABLES = None


def tables():
    """-> (radius [21,15] float64, restrained pairs [21,15,15] bool)"""
    global _TABLES
    if _TABLES is None:
        from pepflowww_amd import geometry
        _TABLES = (geometry.sasa_radius_table().numpy().astype(np.float64), geometry.restrained_pair_table().numpy())
    return _TABLES


def params_of(kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def _norm(v):
    return np.sqrt((v * v).sum(-1))


def energy(pos, ref, atom_mask, aa, index, movable, dtype=np.float64, delta=0.0, **kw):
    """pos, ref [N,A,3], atom_mask [N,A], aa [N], index [N], movable [N] -> dict: terms [4], energy, gradient [N,15,3], terms_atom
    [N,15,4], energy_atom [N,15] (float64 arrays holding `dtype` numbers; the sums in float64), moving [N,15] bool; and what the
    comparison rule of relax_cases.py needs, per atom: n_terms (the additions behind it, pairs within `delta` of overlapping
    included), e_slope = sum |de/dd| and g_abs = sum |g_i|, g_slope = sum of the bounds of |dg_i/dx| over its terms."""
    p = params_of(kw)
    f = dtype
    N, A = pos.shape[0], pos.shape[1]
    S = min(A, SLOTS)
    rad_t, pair_t = tables()
    trow = np.where((aa < 0) | (aa > 20), 20, aa)
    rad = rad_t[trow]
    ex = np.zeros((N, SLOTS), bool)
    ex[:, :S] = atom_mask[:, :S].astype(bool) & (rad[:, :S] > 0)
    X, R = np.zeros((N, SLOTS, 3), f), np.zeros((N, SLOTS, 3), f)
    X[:, :S], R[:, :S] = pos[:, :S].astype(f), ref[:, :S].astype(f)
    mov = movable.astype(bool)
    moving = ex & mov[:, None]
    k = {n: f(p[n]) for n in ("k_rest", "k_intra", "k_bond", "k_angle", "k_clash")}
    half, quarter = f(0.5), f(0.25)
    e = np.zeros((N, SLOTS, 4), f)
    g = np.zeros((N, SLOTS, 3), f)
    n_terms, e_slope = np.zeros((N, SLOTS)), np.zeros((N, SLOTS))
    g_abs, g_slope = np.zeros((N, SLOTS)), np.zeros((N, SLOTS))

    # restraint
    d = X - R
    e[..., 0] = np.where(moving, (half * k["k_rest"]) * ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]), 0)
    g_rest = np.where(moving[..., None], k["k_rest"] * d, 0).astype(f)
    n_terms += moving * 3
    e_slope += moving * p["k_rest"] * _norm(d.astype(np.float64))
    g_abs += _norm(g_rest.astype(np.float64))
    g_slope += moving * p["k_rest"]

    # internal distances
    m = pair_t[trow] & ex[:, :, None] & ex[:, None, :] & mov[:, None, None]
    D, D0 = X[:, :, None] - X[:, None, :], R[:, :, None] - R[:, None, :]
    dd = np.sqrt((D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2]).astype(f)
    d0 = np.sqrt((D0[..., 0] * D0[..., 0] + D0[..., 1] * D0[..., 1]) + D0[..., 2] * D0[..., 2]).astype(f)
    diff = np.where(m, dd - d0, 0).astype(f)
    e[..., 1] = (quarter * k["k_intra"]) * (diff * diff).sum(-1, dtype=f)
    with np.errstate(divide="ignore", invalid="ignore"):
        fac = np.where(dd > 0, diff / dd, 0).astype(f)
    g_in = (k["k_intra"] * (fac[..., None] * D).sum(2, dtype=f)).astype(f)
    n_terms += m.sum(-1)
    e_slope += p["k_intra"] * np.abs(diff.astype(np.float64)).sum(-1)           # 1/2 k |diff| for d and again for d0
    g_abs += p["k_intra"] * np.abs(diff.astype(np.float64)).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        g_slope += p["k_intra"] * np.where(m, 1.0 + np.abs(diff) / np.maximum(dd, 1e-30), 0).astype(np.float64).sum(-1)

    # connections
    g_conn = np.zeros((N, SLOTS, 3), f)
    idx = index.astype(np.int64)
    for n in range(N - 1):
        if idx[n + 1] - idx[n] != 1 or not (mov[n] or mov[n + 1]) or not (ex[n, 2] and ex[n + 1, 0]):
            continue
        u, v, w = X[n, 1] - X[n, 2], X[n + 1, 0] - X[n, 2], X[n + 1, 1] - X[n + 1, 0]
        dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]  # noqa: E731
        lv = np.sqrt(dot(v, v))
        if not lv > 0:
            continue
        l0 = f(CN_LEN_PRO if aa[n + 1] == PRO else CN_LEN)
        dl = lv - l0
        en = (half * k["k_bond"]) * (dl * dl)
        gr = np.zeros((4, 3), f)                            # CA_n, C_n, N_n+1, CA_n+1
        vh = v / lv
        fb = k["k_bond"] * dl
        gr[2] = fb * vh
        gr[1] = -(fb * vh)
        slope_e, slope_g, absg, cnt = p["k_bond"] * abs(float(dl)), p["k_bond"] * (1 + abs(float(dl)) / float(lv)), abs(float(fb)), 1
        lu, lw = np.sqrt(dot(u, u)), np.sqrt(dot(w, w))
        if ex[n, 1] and lu > 0:
            uh = u / lu
            c = dot(uh, vh)
            dc = c - f(COS_CA_C_N)
            fa = k["k_angle"] * dc
            en = en + (half * k["k_angle"]) * (dc * dc)
            d_ca, d_n = (vh - c * uh) / lu, (uh - c * vh) / lv
            gr[0] += fa * d_ca
            gr[2] += fa * d_n
            gr[1] -= fa * (d_ca + d_n)
            lmin = float(min(lu, lv))
            slope_e += p["k_angle"] * abs(float(dc)) * 4 / lmin
            slope_g += p["k_angle"] * (1 + abs(float(dc))) * 12 / lmin ** 2
            absg += abs(float(fa)) * 2 / lmin
            cnt += 1
        if ex[n + 1, 1] and lw > 0:
            wh, ph = w / lw, -vh
            c = dot(ph, wh)
            dc = c - f(COS_C_N_CA)
            fa = k["k_angle"] * dc
            en = en + (half * k["k_angle"]) * (dc * dc)
            d_c, d_ca = (wh - c * ph) / lv, (ph - c * wh) / lw
            gr[1] += fa * d_c
            gr[3] += fa * d_ca
            gr[2] -= fa * (d_c + d_ca)
            lmin = float(min(lw, lv))
            slope_e += p["k_angle"] * abs(float(dc)) * 4 / lmin
            slope_g += p["k_angle"] * (1 + abs(float(dc))) * 12 / lmin ** 2
            absg += abs(float(fa)) * 2 / lmin
            cnt += 1
        owner = (n, 2) if mov[n] else (n + 1, 0)
        e[owner + (2,)] = en
        n_terms[owner] += 8 * cnt
        e_slope[owner] += slope_e
        for i, at in enumerate(((n, 1), (n, 2), (n + 1, 0), (n + 1, 1))):
            if moving[at]:
                g_conn[at] = (g_conn[at] + gr[i]).astype(f)
                n_terms[at] += 8 * cnt
                g_abs[at] += absg
                g_slope[at] += slope_g

    # clashes
    n = N * SLOTS
    x = X.reshape(n, 3)
    exf, movf, radf = ex.reshape(n), np.repeat(mov, SLOTS), rad.reshape(n).astype(f)
    res_idx, slot = np.repeat(idx, SLOTS), np.tile(np.arange(SLOTS), N)
    pm = exf[:, None] & exf[None, :] & (res_idx[:, None] != res_idx[None, :]) & (movf[:, None] | movf[None, :])
    cn = (slot[:, None] == 2) & (slot[None, :] == 0) & (res_idx[:, None] + 1 == res_idx[None, :])
    pm &= ~(cn | cn.T) & ~((slot[:, None] == 5) & (slot[None, :] == 5))
    Dx = x[:, None, :] - x[None, :, :]
    d2 = (Dx[..., 0] * Dx[..., 0] + Dx[..., 1] * Dx[..., 1]) + Dx[..., 2] * Dx[..., 2]
    dist = np.sqrt(f(1e-10) + d2).astype(f)
    lim = (((radf[:, None] + radf[None, :]) - f(p["clash_overlap_tolerance"])) + f(p["clash_margin"])).astype(f)
    over = np.where(pm & (dist < lim), lim - dist, 0).astype(f)
    wgt = np.where(movf[None, :], half, f(1.0))
    e_cl = ((half * k["k_clash"]) * (wgt * (over * over)).sum(1, dtype=f)).astype(f)
    g_cl = (-(k["k_clash"] * ((over / dist)[..., None] * Dx).sum(1, dtype=f))).astype(f)
    rowm = (exf & movf)
    e[..., 3] = np.where(rowm, e_cl, 0).reshape(N, SLOTS)
    g_cl = np.where(rowm[:, None], g_cl, 0).reshape(N, SLOTS, 3).astype(f)
    near = pm & (lim - dist > -delta) & rowm[:, None]
    o64 = over.astype(np.float64)
    n_terms += near.sum(1).reshape(N, SLOTS)
    e_slope += (p["k_clash"] * (near * o64).sum(1)).reshape(N, SLOTS)
    g_abs += (p["k_clash"] * (near * o64).sum(1)).reshape(N, SLOTS)
    g_slope += (p["k_clash"] * (near * (1.0 + o64 / dist)).sum(1)).reshape(N, SLOTS)

    grad = (((g_rest + g_in).astype(f) + g_conn).astype(f) + g_cl).astype(f)
    grad = np.where(moving[..., None], grad, 0)
    e = np.where(moving[..., None], e, 0)
    e_atom = (((e[..., 0] + e[..., 1]).astype(f) + e[..., 2]).astype(f) + e[..., 3]).astype(f)
    terms = e.astype(np.float64).reshape(-1, 4).sum(0)
    return dict(terms=terms, energy=float(((terms[0] + terms[1]) + terms[2]) + terms[3]), gradient=grad.astype(np.float64),
                terms_atom=e.astype(np.float64), energy_atom=e_atom.astype(np.float64), moving=moving, n_terms=n_terms,
                e_slope=e_slope, g_abs=g_abs, g_slope=g_slope)


def minimise(pos, atom_mask, aa, index, movable, steps, replay=None, dtype=np.float64, bound=None, **kw):
    """The minimiser of csrc/relax.hip from pos [N,A,3] with ref = pos.  replay: a list of `steps` decisions taken instead of the
    oracle's own E(y) <= E.  alpha is kept in float32 (1.2f, 0.5f), as the kernel keeps it, whatever `dtype` is.
    -> dict: pos [N,15,3] (float64 array of `dtype` numbers), energy_trace [steps+1], accepted [steps], step_size [steps] float32,
    delta_e [steps] = E(y) - E of every trial in this run's own sums (nan once frozen); with bound(oracle dict, positions) -> the
    allowance of that state's energy, decision_bound [steps] = bound at x + bound at the trial y; terms_initial, terms_final, grad_max,
    iterations."""
    p = params_of(kw)
    f = dtype
    A = pos.shape[1]
    S = min(A, SLOTS)
    ref = np.zeros((pos.shape[0], SLOTS, 3), np.float32)
    ref[:, :S] = pos[:, :S]
    mask = np.zeros((pos.shape[0], SLOTS), bool)
    mask[:, :S] = atom_mask[:, :S]
    ev = lambda x: energy(x, ref, mask, aa, index, movable, dtype=dtype, **kw)  # noqa: E731
    x = ref.astype(f)
    cur = ev(x)
    E, g = cur["energy"], cur["gradient"].astype(f)
    alpha = np.float32(p["step0"])
    trace, acc, step, dE, dB = [E], [], [], [], []
    first = cur
    frozen = float(np.abs(g).max(initial=0.0)) <= p["gtol"]
    its = 0
    for i in range(steps):
        step.append(alpha)
        if frozen:
            trace.append(E)
            acc.append(False)
            dE.append(float("nan"))
            dB.append(float("nan"))
            continue
        its = i + 1
        y = (x - f(alpha) * g).astype(f)
        new = ev(y)
        dE.append(new["energy"] - E)
        dB.append(bound(cur, x) + bound(new, y) if bound is not None else float("nan"))
        ok = bool(replay[i]) if replay is not None else new["energy"] <= E
        if ok:
            x, cur = y, new
            E, g = new["energy"], new["gradient"].astype(f)
            alpha = np.minimum(np.float32(1.2) * alpha, np.float32(ALPHA_MAX))
            frozen = float(np.abs(g).max(initial=0.0)) <= p["gtol"]
        else:
            alpha = np.float32(0.5) * alpha
        trace.append(E)
        acc.append(ok)
    return dict(pos=x.astype(np.float64), energy_trace=np.array(trace), accepted=np.array(acc, bool),
                step_size=np.array(step, np.float32), delta_e=np.array(dE), decision_bound=np.array(dB), terms_initial=first["terms"], terms_final=cur["terms"],
                grad_max=float(np.abs(g).max(initial=0.0)), iterations=its, moving=cur["moving"])
