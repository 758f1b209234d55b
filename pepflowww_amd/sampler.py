"""Device-resident Euler sampler (FlowModel.sample loop, flow_model.py:279-374).

The reference syncs with the host nine times per step (`.cpu()` into clean_traj, 313-314) and
rebuilds `t` on the host every step (288).  Here the whole loop lives on the GPU:
  * state (R_t, x_t, angles_t, seq_t, simplex_t), the time grid and a step counter are device
    buffers; one step = DenoiseEngine plan + pf_sampler_step;
  * that step is captured ONCE into a hipGraph and replayed num_steps times (launch-bound inner
    loop -> one graph launch per step);
  * every step's clean prediction is written into [num_steps, ...] trajectory buffers; a single
    D2H copy at the end produces the reference's list of dicts of CPU tensors.
"""
import ctypes as C
import dataclasses
import math
import numbers

import numpy as np
import torch

from . import _capi


def quat_to_rot_host(q):
    """Unit quaternions [..., 4] -> rotation matrices [..., 3, 3] on the host, in NUMPY: torch's CPU ops fork an OpenMP team for any
    tensor beyond 32 k elements, and in a process whose (often > 100) pool threads were used elsewhere that fork was measured at 20 - 200 ms
    for a 150 KB tensor (profiles/r05/README.md, per-call stalls) -- numpy's elementwise loops stay on the calling thread."""
    q = q.numpy() if torch.is_tensor(q) else q
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    a, b, c, d = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    rot = np.stack([a*a+b*b-c*c-d*d, 2*(b*c-a*d), 2*(b*d+a*c),
                    2*(b*c+a*d), a*a-b*b+c*c-d*d, 2*(c*d-a*b),
                    2*(b*d-a*c), 2*(c*d+a*b), a*a-b*b-c*c+d*d], -1).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(rot.reshape(q.shape[:-1] + (3, 3))))


def default_noise(B, L, generator=None):
    """Initial noise drawn on the host like the reference's uniform_so3 (pepflow/modules/so3/dist.py:40-45,
    Haar via normalised Gaussian quaternions) + randn / rand (flow_model.py:255,264,269)."""
    g = generator
    q = torch.randn(B, L, 4, generator=g)                 # (draw order as before: rotations, translations, angles, simplex)
    trans0 = torch.randn(B, L, 3, generator=g)
    ang = torch.rand(B, L, 5, generator=g)
    return {"rot0": quat_to_rot_host(q), "trans0": trans0, "ang0": torch.from_numpy(ang.numpy() * np.float32(2 * math.pi)),
            "simplex0": torch.randn(B, L, 20, generator=g)}


# ---- conditioned sampling: host-side validation and packing (no GPU needed) ------------------------------------------------------
# The reference's sample() (flow_model.py:229-374) has none of this: it starts from pure noise on linspace(1e-2, 1, num_steps), its three
# switches cover the whole peptide, and any of the 20 residue types may be drawn.  A partial start places the initial state on the
# training corruption's interpolants (flow_model.py:125-158) between the noise and a given state: an OFF-LABEL use of the trained flow.
ALL_AA = (1 << 20) - 1                       # every class allowed (pf_sampler_cond_args.aa_allowed)
FLAG_BB, FLAG_ANG, FLAG_SEQ = 1, 2, 4        # bits of pf_sampler_cond_args.res_flags
_START_KEYS = {"rotmats": (3, 3), "trans": (3,), "angles": (5,), "seqs": ()}      # the entries of a trajectory dict a start may give
COND_ROW_KEYS = ("res_flags", "aa_allowed") + tuple(_START_KEYS)                  # the per-residue tensors of a packed `cond`
_COND_PAD = {"res_flags": 0, "aa_allowed": ALL_AA, "rotmats": 0, "trans": 0, "angles": 0, "seqs": 21}


def make_grid(num_steps, t_start=None, ts=None):
    """The time grid of a call as an fp32 CPU tensor [num_steps]: linspace(1e-2, 1, N) (flow_model.py:280), linspace(t_start, 1, N) for
    0 < t_start < 1, or the caller's own strictly increasing `ts` in (0, 1].  ValueError otherwise."""
    num_steps = int(num_steps)
    if num_steps < 1:
        raise ValueError(f"num_steps = {num_steps}: at least one step")
    if ts is not None:
        if t_start is not None:
            raise ValueError("t_start and ts exclude each other: ts IS the grid")
        g = torch.as_tensor(ts).detach().to("cpu", torch.float32)
        if g.dim() != 1 or g.numel() != num_steps:
            raise ValueError(f"ts: expected a 1-D grid of num_steps = {num_steps} values, got shape {tuple(g.shape)}")
        if not (bool(g[0] > 0) and bool(g[-1] <= 1) and bool((g[1:] > g[:-1]).all())):
            raise ValueError("ts: expected strictly increasing values in (0, 1]")
        return g.clone().contiguous()
    if t_start is None:
        return torch.linspace(1e-2, 1.0, num_steps)
    t = float(t_start)
    if not 0.0 < t < 1.0:
        raise ValueError(f"t_start = {t_start}: expected 0 < t_start < 1")
    return torch.linspace(t, 1.0, num_steps)


def pack_res_flags(sample_bb, sample_ang, sample_seq, B, L):
    """-> (scalar flags, byte plane).  All three plain bools: (the bools, None).  Any bool [B, L] tensor among them: the scalars are
    broadcast and the call runs on the uint8 [B, L] plane (bit 0 backbone, 1 angles, 2 sequence); the scalar flags are then unused
    by the kernels and returned as all-True (one cached sampler serves every plane)."""
    vals = (sample_bb, sample_ang, sample_seq)
    if not any(torch.is_tensor(v) for v in vals):
        return tuple(bool(v) for v in vals), None
    plane = np.zeros((B, L), dtype=np.uint8)
    for bit, (name, v) in enumerate(zip(("sample_bb", "sample_ang", "sample_seq"), vals)):
        if torch.is_tensor(v):
            if v.dtype != torch.bool or tuple(v.shape) != (B, L):
                raise ValueError(f"{name}: expected a bool or a bool tensor [{B}, {L}], got {v.dtype} {tuple(v.shape)}")
            m = v.detach().cpu().numpy()
        else:
            m = np.full((B, L), bool(v))
        plane |= m.astype(np.uint8) << np.uint8(bit)
    return (True, True, True), torch.from_numpy(plane)


def pack_aa_allowed(aa_allowed, B, L):
    """bool [20] / [L, 20] / [B, L, 20] -> int32 [B, L] with bit k = class k may be drawn; None -> None.  A row that allows no class
    raises ValueError."""
    if aa_allowed is None:
        return None
    m = torch.as_tensor(aa_allowed)
    if m.dtype != torch.bool or m.dim() not in (1, 2, 3) or tuple(m.shape) != (B, L, 20)[3 - m.dim():]:
        raise ValueError(f"aa_allowed: expected bool [20], [{L}, 20] or [{B}, {L}, 20], got {m.dtype} {tuple(m.shape)}")
    a = np.broadcast_to(m.detach().cpu().numpy(), (B, L, 20))
    bits = (a.astype(np.int64) << np.arange(20, dtype=np.int64)).sum(-1).astype(np.int32)
    if (bits == 0).any():
        b, l = np.argwhere(bits == 0)[0]
        raise ValueError(f"aa_allowed: no class allowed at sample {b}, residue {l}")
    return torch.from_numpy(np.ascontiguousarray(bits))


def check_start(start, B, L):
    """None -> None (pure noise); "native" -> {} (every entry from the batch's own peptide); a dict with any of rotmats [B,L,3,3],
    trans [B,L,3], angles [B,L,5], seqs [B,L] (the entries of a trajectory dict; others are ignored, a missing one takes the
    native's value) -> those entries as fp32 / int64 tensors on the device they came from.  seqs outside 0..21 raise (for a device
    tensor that is one host read of its extremes)."""
    if start is None:
        return None
    if isinstance(start, str):
        if start != "native":
            raise ValueError(f"start = {start!r}: expected None, 'native' or a dict")
        return {}
    if not isinstance(start, dict):
        raise ValueError(f"start: expected None, 'native' or a dict, got {type(start).__name__}")
    out = {}
    for k, tail in _START_KEYS.items():
        v = start.get(k)
        if v is None:
            continue
        if not torch.is_tensor(v) or tuple(v.shape) != (B, L) + tail:
            raise ValueError(f"start[{k!r}]: expected a tensor {(B, L) + tail}, got {tuple(v.shape) if torch.is_tensor(v) else type(v).__name__}")
        if k == "seqs":
            if v.dtype not in (torch.int64, torch.int32):
                raise ValueError(f"start['seqs']: expected an integer tensor, got {v.dtype}")
            # residue types 0..19; 20 (UNK) and 21 (PAD) as a batch's `aa` may hold them on context rows: like seq_to_simplex
            # (flow_model.py:108-109) they give the simplex of no class.  Anything else is a mistake, not a residue type.
            if v.numel() and not (0 <= int(v.min()) and int(v.max()) <= 21):
                raise ValueError(f"start['seqs']: residue types must lie in 0..21, got {int(v.min())}..{int(v.max())}")
            out[k] = v.detach().to(torch.int64)
        else:
            if not v.dtype.is_floating_point:
                raise ValueError(f"start[{k!r}]: expected a floating-point tensor, got {v.dtype}")
            out[k] = v.detach().to(torch.float32)
    return out


def make_cond(B, L, num_steps, sample_bb=True, sample_ang=True, sample_seq=True, t_start=None, ts=None, start=None, aa_allowed=None):
    """Everything sample()'s conditioning arguments say, validated: (grid, scalar flags, cond).  cond is None for a call that uses none
    of them beyond the grid, else a dict: "partial" (bool) and any of the per-residue tensors COND_ROW_KEYS at the caller's [B, L]."""
    grid = make_grid(num_steps, t_start, ts)
    flags, plane = pack_res_flags(sample_bb, sample_ang, sample_seq, B, L)
    allowed = pack_aa_allowed(aa_allowed, B, L)
    st = check_start(start, B, L)
    if st is not None and t_start is None and ts is None:
        raise ValueError("start needs a grid: pass t_start or ts (the state is placed at the grid's first time)")
    if plane is None and allowed is None and st is None:
        return grid, flags, None
    cond = {"partial": st is not None}
    if plane is not None:
        cond["res_flags"] = plane
    if allowed is not None:
        cond["aa_allowed"] = allowed
    cond.update(st or {})
    return grid, flags, cond


def _pad_axis1(v, n, value=0):
    """[B, L0, ...] -> [B, L0 + n, ...] with `value` appended along the residue axis.  Host tensors go through numpy (torch's CPU ops fork
    an OpenMP team beyond 32 k elements: 20 - 200 ms stalls were measured on a 150 KB pad, see quat_to_rot_host), device tensors
    through one GPU kernel."""
    if v.is_cuda:
        return torch.nn.functional.pad(v, [0, 0] * (v.dim() - 2) + [0, n], value=value)
    a = v.numpy()
    out = np.full((a.shape[0], a.shape[1] + n) + a.shape[2:], value, dtype=a.dtype)
    out[:, :a.shape[1]] = a
    return torch.from_numpy(out)


def _rows(v, idx, axis=0):
    """v[idx] along `axis`: device tensors by one GPU gather, host tensors through numpy (for the reason _pad_axis1 gives)."""
    if v.is_cuda:
        return v.index_select(axis, torch.as_tensor(idx, dtype=torch.int64, device=v.device))
    return torch.from_numpy(np.ascontiguousarray(np.take(v.numpy(), np.asarray(idx, dtype=np.int64), axis=axis)))


def _fit(v, L0, Lk, axis=1, value=0):
    """Residue axis cut or padded from L0 to Lk."""
    if Lk == L0:
        return v
    if Lk < L0:
        return v.narrow(axis, 0, Lk).contiguous()
    if axis == 1:
        return _pad_axis1(v, Lk - L0, value)
    lead = tuple(v.shape[:axis - 1])                     # ([2N, B, L0, 20]: fold the leading axis, pad, unfold)
    w = _pad_axis1(v.reshape((-1,) + tuple(v.shape[axis:])), Lk - L0, value)
    return w.reshape(lead + tuple(v.shape[axis - 1:axis]) + (Lk,) + tuple(v.shape[axis + 1:]))


def fit_cond(cond, L0, Lk, idx=None):
    """The packed conditioning of the samples `idx` (None: all) with the residue axis cut or padded from L0 to Lk by INERT rows: no
    flag set, every class allowed, identity frame, zeros, residue type 21 (none of it is read: padded rows are not generated)."""
    if cond is None:
        return None
    out = {"partial": cond["partial"]}
    for k in COND_ROW_KEYS:
        v = cond.get(k)
        if v is None:
            continue
        w = _fit(v if idx is None else _rows(v, idx), L0, Lk, 1, _COND_PAD[k])
        if k == "rotmats" and Lk > L0:
            for d in range(3):
                w[:, L0:, d, d] = 1
        out[k] = w
    return out


def _options(name, given, defaults):
    """The checks every extension's option dict starts with: a dict, known entries only; -> the entries over their defaults."""
    if not isinstance(given, dict):
        raise ValueError(f"{name}: expected None or a dict, got {type(given).__name__}")
    for k in given:
        if k not in defaults:
            raise ValueError(f"{name}: unknown entry {k!r}; the entries are {tuple(defaults)}")
    return {**defaults, **given}


def shard_cond_kwargs(kw, lo, hi, total):
    """sample()'s conditioning keywords with every per-sample tensor ([total, ...]) cut to the shard [lo, hi)."""
    out = dict(kw)
    for k in ("sample_bb", "sample_ang", "sample_seq"):
        if torch.is_tensor(out.get(k)) and out[k].dim() == 2 and out[k].shape[0] == total:
            out[k] = out[k][lo:hi]
    a = out.get("aa_allowed")
    if a is not None and torch.as_tensor(a).dim() == 3 and torch.as_tensor(a).shape[0] == total:
        out["aa_allowed"] = torch.as_tensor(a)[lo:hi]
    if isinstance(out.get("start"), dict):
        out["start"] = {k: (v[lo:hi] if k in _START_KEYS and torch.is_tensor(v) and v.dim() >= 2 and v.shape[0] == total else v)
                        for k, v in out["start"].items()}
    return out


# ---- guided sampling: host-side validation and packing (no GPU needed) -----------------------------------------------------------
# C-alpha potentials that shift the translation prediction of every step (csrc/guidance.hip; formulas: include/pepflow_hip.h and
# INTEGRATION.md).  The reference has none of this: like the partial start an OFF-LABEL use of the trained flow.  The defaults are
# starting values: nothing has been tuned on a trained checkpoint.
GUIDE_TERMS = ("receptor_clash", "self_clash", "ca_bond", "hotspot", "restraint")
GUIDE_DEFAULTS = {"weights": None, "r_receptor": 4.5, "r_self": 4.5, "min_sep": 3, "bond_tol": 0.1, "r_hotspot": 8.0, "beta": 1.0,
                  "hotspots": None, "restraints": None, "scale": 1.0, "t_on": 0.0, "power": 1, "max_shift": 2.0}
# slots of the device parameter vector (pf_guidance_args.params): the four weights first
_GUIDE_SLOTS = ("r_receptor", "r_self", "min_sep", "bond_tol", "r_hotspot", "beta", "scale", "t_on", "power", "max_shift")


def _guide_weights(w):
    """weights of terms 0-3: None, a dict by term name or a sequence of four -> four floats >= 0"""
    if w is None:
        return [0.0] * 4
    if isinstance(w, dict):
        for k in w:
            if k not in GUIDE_TERMS[:4]:
                raise ValueError(f"guide['weights']: unknown term {k!r}; the weighted terms are {GUIDE_TERMS[:4]} (a restraint carries its own weight)")
        w = [w.get(k, 0.0) for k in GUIDE_TERMS[:4]]
    w = [float(v) for v in w]
    if len(w) != 4:
        raise ValueError(f"guide['weights']: expected the weights of {GUIDE_TERMS[:4]}, got {len(w)} values")
    for k, v in zip(GUIDE_TERMS, w):
        if not (math.isfinite(v) and v >= 0):
            raise ValueError(f"guide['weights'][{k!r}] = {v}: a weight is a finite number >= 0")
    return w


def _one_list_for_all(rs):
    """a non-empty list whose entries are restraints themselves, (i, j, lo, hi, weight), not lists of restraints"""
    return len(rs) > 0 and all(isinstance(r, (list, tuple)) and len(r) == 5 and not isinstance(r[0], (list, tuple)) for r in rs)


def _guide_restraints(restraints, B):
    """None, one list of (i, j, lo, hi, weight) for every sample, or a list of B such lists -> B lists"""
    if restraints is None:
        return [[] for _ in range(B)]
    rs = list(restraints)
    if not rs:
        return [[] for _ in range(B)]
    if _one_list_for_all(rs):
        return [rs for _ in range(B)]
    if len(rs) != B:
        raise ValueError(f"guide['restraints']: expected one list of (i, j, lo, hi, weight) or one list per sample ({B}), got {len(rs)} lists")
    return [list(r) for r in rs]


def make_guide(guide, B, L, generate_mask=None, res_mask=None):
    """sample()'s `guide` dict, validated and packed on the host: None -> None, else a dict of CPU tensors at the caller's [B, L]:
    params fp32 [16] (pf_guidance_args.params), hotspots uint8 [B, L] or None, pair_idx int32 [B, 64, 2], pair_par fp32 [B, 64, 3]
    (lo, hi, weight; weight 0 pads).  generate_mask / res_mask (bool [B, L]), when given, are what a hot spot and a restraint index
    are checked against.  ValueError with the offending value: a hot spot on a generated residue, an index outside the sample,
    lo > hi, a negative weight, a power outside {0, 1, 2}, t_on >= 1, more than 64 restraints of one sample."""
    if guide is None:
        return None
    g = _options("guide", guide, GUIDE_DEFAULTS)
    gen = None if generate_mask is None else torch.as_tensor(generate_mask).detach().cpu().bool()
    resm = None if res_mask is None else torch.as_tensor(res_mask).detach().cpu().bool()
    vals = {k: float(g[k]) for k in _GUIDE_SLOTS}
    for k in ("r_receptor", "r_self", "r_hotspot", "bond_tol", "scale", "max_shift", "min_sep"):
        if not (math.isfinite(vals[k]) and vals[k] >= 0):
            raise ValueError(f"guide[{k!r}] = {g[k]!r}: expected a finite number >= 0")
    if not (math.isfinite(vals["beta"]) and vals["beta"] > 0):
        raise ValueError(f"guide['beta'] = {g['beta']!r}: expected a finite number > 0")
    if g["power"] not in (0, 1, 2) or isinstance(g["power"], bool):
        raise ValueError(f"guide['power'] = {g['power']!r}: expected 0, 1 or 2")
    if int(g["min_sep"]) != g["min_sep"]:
        raise ValueError(f"guide['min_sep'] = {g['min_sep']!r}: expected an integer")
    if not 0.0 <= vals["t_on"] < 1.0:
        raise ValueError(f"guide['t_on'] = {g['t_on']!r}: expected 0 <= t_on < 1")
    params = np.zeros(_capi.GUIDE_NPARAMS, dtype=np.float32)
    params[:4] = _guide_weights(g["weights"])
    params[4:4 + len(_GUIDE_SLOTS)] = [vals[k] for k in _GUIDE_SLOTS]
    hot = None
    if g["hotspots"] is not None:
        h = torch.as_tensor(g["hotspots"]).detach().cpu()
        if h.dtype != torch.bool or tuple(h.shape) not in ((L,), (B, L)):
            raise ValueError(f"guide['hotspots']: expected bool [{L}] or [{B}, {L}], got {h.dtype} {tuple(h.shape)}")
        h = h.expand(B, L)
        for name, bad in (("a generated residue", gen), ("a residue outside the sample", None if resm is None else ~resm)):
            if bad is not None and bool((h & bad).any()):
                b, l = (h & bad).nonzero()[0].tolist()
                raise ValueError(f"guide['hotspots']: sample {b}, residue {l} is {name}; a hot spot is a context residue")
        hot = torch.from_numpy(np.ascontiguousarray(h.numpy().astype(np.uint8)))
    n_max = _capi.GUIDE_MAX_PAIRS
    idx, par = np.zeros((B, n_max, 2), dtype=np.int32), np.zeros((B, n_max, 3), dtype=np.float32)
    for b, rs in enumerate(_guide_restraints(g["restraints"], B)):
        if len(rs) > n_max:
            raise ValueError(f"guide['restraints']: sample {b} has {len(rs)} restraints; at most {n_max}")
        for p, r in enumerate(rs):
            if len(r) != 5:
                raise ValueError(f"guide['restraints']: sample {b}, restraint {p}: expected (i, j, lo, hi, weight), got {tuple(r)!r}")
            if int(r[0]) != r[0] or int(r[1]) != r[1]:
                raise ValueError(f"guide['restraints']: sample {b}, restraint {p}: residue indices must be integers, got {r[0]!r}, {r[1]!r}")
            i, j, lo, hi, w = int(r[0]), int(r[1]), float(r[2]), float(r[3]), float(r[4])
            for v in (i, j):
                if not 0 <= v < L or (resm is not None and not bool(resm[b, v])):
                    raise ValueError(f"guide['restraints']: sample {b}, restraint {p}: residue index {v} lies outside the sample")
            if not (math.isfinite(lo) and math.isfinite(hi)) or lo > hi:
                raise ValueError(f"guide['restraints']: sample {b}, restraint {p}: lo = {lo} > hi = {hi}")
            if not (math.isfinite(w) and w >= 0):
                raise ValueError(f"guide['restraints']: sample {b}, restraint {p}: weight {w}: a weight is a finite number >= 0")
            idx[b, p], par[b, p] = (i, j), (lo, hi, w)
    return {"params": torch.from_numpy(params), "hotspots": hot, "pair_idx": torch.from_numpy(idx), "pair_par": torch.from_numpy(par)}


def fit_guide(guide, L0, Lk, idx=None):
    """The packed guidance (make_guide) of the samples `idx` (None: all) with the residue axis of the hot-spot plane cut or padded
    from L0 to Lk (no hot spot on the padding).  Restraints carry residue INDICES: padding is appended at the end, so they stay."""
    if guide is None:
        return None
    out = dict(guide)
    if guide["hotspots"] is not None:
        h = guide["hotspots"] if idx is None else _rows(guide["hotspots"], idx)
        out["hotspots"] = _fit(h, L0, Lk, 1, 0)
    if idx is not None:
        out["pair_idx"], out["pair_par"] = _rows(guide["pair_idx"], idx), _rows(guide["pair_par"], idx)
    return out


def shard_guide(guide, lo, hi, total):
    """sample()'s `guide` dict with its per-sample entries (hotspots [total, L], one restraint list per sample) cut to the shard [lo, hi)"""
    if not isinstance(guide, dict):
        return guide
    out = dict(guide)
    h = out.get("hotspots")
    if h is not None and torch.as_tensor(h).dim() == 2 and torch.as_tensor(h).shape[0] == total:
        out["hotspots"] = torch.as_tensor(h)[lo:hi]
    r = out.get("restraints")
    if r is not None and len(r) == total and not _one_list_for_all(list(r)):
        out["restraints"] = list(r)[lo:hi]
    return out


# ---- tempered and stochastic sampling: host-side validation and packing (no GPU needed) ------------------------------------------
# A temperature on the prediction's sequence draw and Euler-Maruyama noise on the rotation and translation state (csrc/temper.hip;
# formulas: include/pepflow_hip.h and INTEGRATION.md).  The reference has none of this: like the partial start and the guidance an
# OFF-LABEL use of the trained flow.  The defaults are starting values: nothing has been tuned on a trained checkpoint.
TEMPER_DEFAULTS = {"seq_temperature": 1.0, "sigma_trans": 0.0, "sigma_rot": 0.0, "power": 1, "t_off": 1.0}
_TEMPER_SLOTS = ("sigma_trans", "sigma_rot", "power", "t_off")      # slots of the device parameter vector (pf_sampler_temper_args.params)


def make_temper(temper, B, L):
    """sample()'s `temper` dict, validated and packed on the host: None -> None, else a dict of CPU tensors at the caller's [B, L]:
    params fp32 [8] (pf_sampler_temper_args.params) and tau fp32 [B, L], or None when seq_temperature is absent or the scalar 1.0.
    ValueError with the offending value: a temperature that is not a finite number > 0, a negative or non-finite sigma, a power
    outside {0, 1, 2}, t_off outside (0, 1], an unknown entry."""
    if temper is None:
        return None
    t = _options("temper", temper, TEMPER_DEFAULTS)
    if t["power"] not in (0, 1, 2) or isinstance(t["power"], bool):
        raise ValueError(f"temper['power'] = {t['power']!r}: expected 0, 1 or 2")
    for k in ("sigma_trans", "sigma_rot", "t_off"):
        if isinstance(t[k], bool) or not isinstance(t[k], numbers.Real):
            raise ValueError(f"temper[{k!r}] = {t[k]!r}: expected a number")
    vals = {k: float(t[k]) for k in _TEMPER_SLOTS}
    for k in ("sigma_trans", "sigma_rot"):
        if not (math.isfinite(vals[k]) and vals[k] >= 0):
            raise ValueError(f"temper[{k!r}] = {t[k]!r}: expected a finite number >= 0")
    if not 0.0 < vals["t_off"] <= 1.0:
        raise ValueError(f"temper['t_off'] = {t['t_off']!r}: expected 0 < t_off <= 1")
    params = np.zeros(_capi.TEMPER_NPARAMS, dtype=np.float32)
    params[:len(_TEMPER_SLOTS)] = [vals[k] for k in _TEMPER_SLOTS]
    tau, st = None, t["seq_temperature"]
    if torch.is_tensor(st):
        if not st.dtype.is_floating_point or tuple(st.shape) not in ((L,), (B, L)):
            raise ValueError(f"temper['seq_temperature']: expected a number or a floating-point tensor [{L}] or [{B}, {L}], got {st.dtype} {tuple(st.shape)}")
        p = np.broadcast_to(st.detach().to("cpu", torch.float32).numpy(), (B, L))
        if not (np.isfinite(p) & (p > 0)).all():
            b, l = np.argwhere(~(np.isfinite(p) & (p > 0)))[0]
            raise ValueError(f"temper['seq_temperature']: sample {b}, residue {l} has temperature {p[b, l]}; a temperature is a finite number > 0")
        tau = torch.from_numpy(np.array(p, dtype=np.float32))          # (a copy: the broadcast view is read-only)
    else:
        if isinstance(st, bool) or not isinstance(st, numbers.Real) or not (math.isfinite(st) and st > 0):
            raise ValueError(f"temper['seq_temperature'] = {st!r}: a temperature is a finite number > 0")
        if float(st) != 1.0:
            tau = torch.full((B, L), float(st), dtype=torch.float32)
    return {"params": torch.from_numpy(params), "tau": tau}


def temper_has_noise(temper):
    """whether a packed `temper` (make_temper) puts noise on the backbone state at all"""
    return temper is not None and bool((temper["params"][:2] > 0).any())


def fit_temper(temper, L0, Lk, idx=None):
    """The packed tempering (make_temper) of the samples `idx` (None: all) with the residue axis of the temperature plane cut or padded
    from L0 to Lk (temperature 1 on the padding: its logits are divided by one and never drawn from)."""
    if temper is None:
        return None
    out = dict(temper)
    if temper["tau"] is not None:
        p = temper["tau"] if idx is None else _rows(temper["tau"], idx)
        out["tau"] = _fit(p, L0, Lk, 1, 1.0)
    return out


def shard_temper(temper, lo, hi, total):
    """sample()'s `temper` dict with its per-sample entry (seq_temperature [total, L]) cut to the shard [lo, hi)"""
    if not isinstance(temper, dict):
        return temper
    out = dict(temper)
    st = out.get("seq_temperature")
    if torch.is_tensor(st) and st.dim() == 2 and st.shape[0] == total:
        out["seq_temperature"] = st[lo:hi]
    return out


def check_gauss(noise, temper, num_steps, B, L):
    """The pre-drawn normals of a call (noise["gauss"], [num_steps - 1, B, L, 6]) against its packed tempering: a run on supplied
    categorical draws (noise["expo"]) with noise on the state must supply the normals too; without `expo` the kernel draws."""
    g = None if noise is None else noise.get("gauss")
    if g is not None and (not torch.is_tensor(g) or tuple(g.shape) != (num_steps - 1, B, L, 6)):
        raise ValueError(f"noise['gauss']: expected a tensor {(num_steps - 1, B, L, 6)}, got {tuple(g.shape) if torch.is_tensor(g) else type(g).__name__}")
    if temper_has_noise(temper) and noise is not None and noise.get("expo") is not None and g is None:
        raise ValueError("noise['expo'] is supplied and temper has a non-zero sigma: supply noise['gauss'] "
                         f"{(num_steps - 1, B, L, 6)} too (a run on supplied draws is supplied throughout)")


# ---- steered sampling: host-side validation and packing (no GPU needed) ----------------------------------------------------------
# Feynman-Kac steering: the samples of one complex are the particles of a group, weighted by a difference potential of the guidance
# energies and resampled systematically when their effective sample size drops (csrc/steer.hip; formulas: include/pepflow_hip.h and
# INTEGRATION.md).  The reference has none of this: like the guidance and the tempering an OFF-LABEL use of the trained flow.  The
# defaults are starting values: nothing has been tuned on a trained checkpoint.
STEER_DEFAULTS = {"groups": None, "lam": 1.0, "every": 1, "ess_frac": 0.5, "t_on": 0.0, "t_off": 1.0}
_STEER_SLOTS = ("lam", "every", "ess_frac", "t_on", "t_off")       # slots of the device parameter vector (pf_sampler_steer_args.params)


def pack_groups(labels):
    """arbitrary integer labels [B] -> (group_ptr int32 [B+1], members int32 [B], group_of int32 [B], n_groups).  Groups are numbered
    by their first member; the members of a group ascend.  group_ptr beyond n_groups repeats B."""
    lab = np.asarray(labels).reshape(-1)
    B = lab.shape[0]
    number, group_of = {}, np.zeros(B, dtype=np.int32)
    for b in range(B):
        group_of[b] = number.setdefault(int(lab[b]), len(number))
    G = len(number)
    members = np.argsort(group_of, kind="stable").astype(np.int32)
    ptr = np.full(B + 1, B, dtype=np.int32)
    ptr[:G + 1] = np.concatenate([[0], np.cumsum(np.bincount(group_of, minlength=G))])
    return ptr, members, group_of, G


def _steer_rows(batch, cond, guide, temper):
    """(name, tensor with the sample on axis 0) of everything the members of a group must share"""
    out = [(f"batch[{k!r}]", v) for k, v in batch.items() if torch.is_tensor(v) and v.dim() >= 1]
    for name, packed, keys in (("cond", cond, COND_ROW_KEYS), ("guide", guide, ("hotspots", "pair_idx", "pair_par")), ("temper", temper, ("tau",))):
        if packed is not None:
            out += [(f"{name}[{k!r}]", packed[k]) for k in keys if packed.get(k) is not None]
    return out


def make_steer(steer, B, L, batch=None, cond=None, guide=None, temper=None):
    """sample()'s `steer` dict, validated and packed on the host: None -> None, else a dict: params float64 [8]
    (pf_sampler_steer_args.params), group_ptr int32 [B+1], members int32 [B] (ascending inside a group), group_of int32 [B], n_groups,
    max_group.  batch / cond / guide / temper: the call's batch and its packed conditioning, guidance and tempering; the members of a
    group must be EXCHANGEABLE: every batch tensor and every per-sample entry of the three equal across them (what
    design.make_design_batch(n_samples=...) produces).  ValueError with the offending value: an unknown entry, steer without guide (the
    energies are the guidance's; guide["scale"] = 0 steers without a gradient shift), lam not a finite number >= 0, every not an
    integer >= 1, ess_frac outside [0, 1], not 0 <= t_on <= t_off <= 1, groups not an integer tensor [B], a group of more than 1024
    members, members that differ (the first differing key and the sample pair are named)."""
    if steer is None:
        return None
    s = _options("steer", steer, STEER_DEFAULTS)
    if guide is None:
        raise ValueError("steer needs guide: the energies the particles are weighted by are the guidance's (guide['scale'] = 0 steers "
                         "without a gradient shift)")
    for k in _STEER_SLOTS:
        if isinstance(s[k], bool) or not isinstance(s[k], numbers.Real):
            raise ValueError(f"steer[{k!r}] = {s[k]!r}: expected a number")
    if not (math.isfinite(s["lam"]) and s["lam"] >= 0):
        raise ValueError(f"steer['lam'] = {s['lam']!r}: expected a finite number >= 0")
    if not isinstance(s["every"], numbers.Integral) or s["every"] < 1:
        raise ValueError(f"steer['every'] = {s['every']!r}: expected an integer >= 1")
    if not 0.0 <= s["ess_frac"] <= 1.0:
        raise ValueError(f"steer['ess_frac'] = {s['ess_frac']!r}: expected a number in [0, 1]")
    if not 0.0 <= s["t_on"] <= s["t_off"] <= 1.0:
        raise ValueError(f"steer['t_on'] = {s['t_on']!r}, steer['t_off'] = {s['t_off']!r}: expected 0 <= t_on <= t_off <= 1")
    gr = s["groups"]
    if gr is None:
        labels = np.zeros(B, dtype=np.int64)
    else:
        if not torch.is_tensor(gr) or gr.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8) or tuple(gr.shape) != (B,):
            raise ValueError(f"steer['groups']: expected None or an integer tensor [{B}], got "
                             f"{(str(gr.dtype) + ' ' + str(tuple(gr.shape))) if torch.is_tensor(gr) else type(gr).__name__}")
        labels = gr.detach().cpu().numpy().astype(np.int64)
    ptr, members, group_of, G = pack_groups(labels)
    sizes = np.diff(ptr[:G + 1])
    if sizes.max() > _capi.STEER_MAX_GROUP:
        g = int(sizes.argmax())
        raise ValueError(f"steer['groups']: group {int(labels[members[ptr[g]]])} has {int(sizes[g])} members; at most {_capi.STEER_MAX_GROUP}")
    rows = _steer_rows(batch or {}, cond, guide, temper)
    for g in range(G):
        m = members[ptr[g]:ptr[g + 1]]
        if len(m) < 2:
            continue
        for name, v in rows:
            if v.shape[0] != B:
                continue
            w = v.detach()[torch.as_tensor(m, dtype=torch.int64, device=v.device)]
            same = (w == w[:1]) | ((w != w) & (w[:1] != w[:1])) if w.dtype.is_floating_point else w == w[:1]
            if not bool(same.all()):
                j = int((~same.reshape(len(m), -1).all(1)).nonzero()[0])
                raise ValueError(f"steer: the members of a group must be exchangeable, but {name} differs between samples {int(m[0])} and "
                                 f"{int(m[j])} of group {int(labels[m[0]])}")
    params = np.zeros(_capi.STEER_NPARAMS, dtype=np.float64)
    params[:len(_STEER_SLOTS)] = [float(s[k]) for k in _STEER_SLOTS]
    return {"params": torch.from_numpy(params), "group_ptr": torch.from_numpy(ptr), "members": torch.from_numpy(members),
            "group_of": torch.from_numpy(group_of), "n_groups": G, "max_group": int(sizes.max()),
            "group_ids": torch.arange(G, dtype=torch.int64)}


def fit_steer(steer, L0, Lk, idx=None):
    """The packed steering (make_steer) of the samples `idx` (None: all): their groups renumbered, "group_ids" = the caller's number of
    every group kept (the columns of noise["resample_u"] and of the records).  Nothing of it lies on the residue axis.  A group that
    `idx` cuts raises ValueError (length buckets cannot cut one: its members share a length)."""
    if steer is None or idx is None:
        return steer
    idx = np.asarray(idx, dtype=np.int64)
    of = steer["group_of"].numpy()
    sub = of[idx]
    whole = np.bincount(of, minlength=steer["n_groups"])
    part = np.bincount(sub, minlength=steer["n_groups"])
    cut = np.nonzero((part > 0) & (part != whole))[0]
    if len(cut):
        raise ValueError(f"steer: group {int(cut[0])} is cut: {int(part[cut[0]])} of its {int(whole[cut[0]])} members are in this part of the batch")
    ptr, members, group_of, G = pack_groups(sub)
    ids = steer["group_ids"].numpy()[sub[members[ptr[:G]]]]
    return {**steer, "group_ptr": torch.from_numpy(ptr), "members": torch.from_numpy(members), "group_of": torch.from_numpy(group_of),
            "n_groups": G, "max_group": int(np.diff(ptr[:G + 1]).max()), "group_ids": torch.from_numpy(np.ascontiguousarray(ids))}


def shard_steer(steer, lo, hi, total):
    """sample()'s `steer` dict with its per-sample entry (groups [total]) cut to the shard [lo, hi).  A boundary that cuts a group
    raises ValueError naming the group: particles are not resampled across ranks."""
    if not isinstance(steer, dict):
        return steer
    out = dict(steer)
    gr = out.get("groups")
    lab = np.zeros(total, dtype=np.int64) if gr is None else torch.as_tensor(gr).detach().cpu().numpy().reshape(-1)
    if lab.shape[0] != total:
        return out
    inside = set(lab[lo:hi].tolist())
    outside = set(lab[:lo].tolist()) | set(lab[hi:].tolist())
    cut = sorted(inside & outside)
    if cut:
        raise ValueError(f"steer: the shard [{lo}, {hi}) cuts group {cut[0]}; a group must lie on one rank")
    if gr is not None:
        out["groups"] = torch.as_tensor(gr)[lo:hi]
    return out


def steer_groups_of_shard(steer, lo, hi, total):
    """the caller's group numbers (columns of noise["resample_u"]) of the groups in the shard [lo, hi): groups are numbered by their
    first member, so a shard of whole groups holds a consecutive run of them"""
    gr = None if not isinstance(steer, dict) else steer.get("groups")
    lab = np.zeros(total, dtype=np.int64) if gr is None else torch.as_tensor(gr).detach().cpu().numpy().reshape(-1)
    of = pack_groups(lab)[2]
    return sorted(set(of[lo:hi].tolist()))


def steer_lineage(ancestors):
    """ancestors [num_steps, B] (the record of a steered run) -> int64 [num_steps, B]: for every FINAL slot b the slot its particle
    sat in at each step, lineage[num_steps-1, b] = b and lineage[s, b] = ancestors[s, lineage[s+1, b]].  Reading step s of the
    slot-indexed trajectory at lineage[s, b] gives one particle's coherent path.  Pure host code."""
    a = torch.as_tensor(ancestors).detach().cpu().to(torch.int64)
    N, B = a.shape
    lin = torch.empty(N, B, dtype=torch.int64)
    lin[N - 1] = torch.arange(B)
    for s in range(N - 2, -1, -1):
        lin[s] = a[s][lin[s + 1]]
    return lin


def check_resample_u(noise, steer, num_steps):
    """The pre-drawn uniforms of a call (noise["resample_u"], [num_steps, G], values in [0, 1)) against its packed steering: a run on
    supplied categorical draws (noise["expo"]) must supply them too, the rule of `gauss`; without `expo` the kernel draws."""
    u = None if noise is None else noise.get("resample_u")
    if u is not None and steer is None:
        raise ValueError("noise['resample_u'] is given but the call is not steered")
    if steer is None:
        return
    G = steer["n_groups"]
    if u is not None:
        if not torch.is_tensor(u) or tuple(u.shape) != (num_steps, G):
            raise ValueError(f"noise['resample_u']: expected a tensor {(num_steps, G)}, got {tuple(u.shape) if torch.is_tensor(u) else type(u).__name__}")
        if not bool(((u >= 0) & (u < 1)).all()):
            raise ValueError("noise['resample_u']: expected values in [0, 1)")
    elif noise is not None and noise.get("expo") is not None:
        raise ValueError(f"noise['expo'] is supplied and the call is steered: supply noise['resample_u'] {(num_steps, G)} too "
                         "(a run on supplied draws is supplied throughout)")


@dataclasses.dataclass(frozen=True, eq=False)
class SampleCall:
    """What one sample() call has validated and packed on the host: the time grid, the three scalar switches and the packed extensions
    (None: the call does not use that one).  Made once per call (make), fitted to an engine's padded length or to a length bucket
    (fit), bound by DeviceSampler.begin."""
    grid: torch.Tensor
    flags: tuple = (True, True, True)
    cond: dict = None
    guide: dict = None
    temper: dict = None
    steer: dict = None

    @classmethod
    def make(cls, batch, num_steps, sample_bb=True, sample_ang=True, sample_seq=True, *, t_start=None, ts=None, start=None,
             aa_allowed=None, guide=None, temper=None, steer=None, noise=None):
        """sample()'s arguments at the caller's [B, L].  The ORDER of the checks is behaviour: a call with two bad arguments raises
        the first one's error."""
        B, L = batch["aa"].shape
        grid, flags, cond = make_cond(B, L, num_steps, sample_bb, sample_ang, sample_seq, t_start, ts, start, aa_allowed)
        guide = make_guide(guide, B, L, batch.get("generate_mask"), batch.get("res_mask"))
        temper = make_temper(temper, B, L)
        check_gauss(noise, temper, int(num_steps), B, L)
        steer = make_steer(steer, B, L, batch, cond, guide, temper)
        check_resample_u(noise, steer, int(num_steps))
        return cls(grid, flags, cond, guide, temper, steer)

    def fit(self, L0, Lk, idx=None):
        """The call of the samples `idx` (None: all) with the residue axis cut or padded from L0 to Lk (fit_cond / fit_guide / fit_temper
        / fit_steer)."""
        return dataclasses.replace(self, cond=fit_cond(self.cond, L0, Lk, idx), guide=fit_guide(self.guide, L0, Lk, idx),
                                   temper=fit_temper(self.temper, L0, Lk, idx), steer=fit_steer(self.steer, L0, Lk, idx))

    @property
    def kinds(self):
        """which extensions the call uses: the keywords of DenoiseEngine.sampler / DeviceSampler"""
        return {"cond": self.cond is not None, "guide": self.guide is not None, "temper": self.temper is not None,
                "steer": self.steer is not None}


class DeviceSampler:
    """Owned by its engine (DenoiseEngine.sampler caches one per (num_steps, flags, cond, guide, temper, steer)): trajectory buffers and
    the captured graphs are reused by the next sample() call.  begin() is what a call changes: the seed, the grid, the context, the
    packed extensions of its SampleCall (set_cond / set_guide / set_temper / set_steer into buffers this sampler owns) and the
    initial state."""

    def __init__(self, engine, num_steps, flags=(True, True, True), first_sample=0, seed=0, cond=False, guide=False, temper=False,
                 steer=False):
        self.eng = engine
        self.lib = engine.lib
        self.N = num_steps
        B, L, dev = engine.B, engine.L, engine.device
        rows = B * L
        e = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
        self.rot1, self.trans1, self.ang1 = e(rows, 9), e(rows, 3), e(rows, 5)
        self.seq1 = e(rows, dt=torch.int64)
        self.gen = e(rows)
        self.simplex_t, self.trans0, self.simplex0 = e(rows, 20), e(rows, 3), e(rows, 20)
        self.traj_rot, self.traj_trans = e(num_steps, rows, 9), e(num_steps, rows, 3)
        self.traj_ang, self.traj_simplex = e(num_steps, rows, 5), e(num_steps, rows, 20)
        self.traj_seq = e(num_steps, rows, dt=torch.int64)
        self.ts = torch.linspace(1e-2, 1.0, num_steps).to(dev)          # flow_model.py:280 (built on CPU, then H2D)
        self.step = e(2, dt=torch.int32)                      # [0] step counter, [1] workgroup ticket
        self.expo = None
        a = _capi.SamplerArgs()
        a.rot1, a.trans1, a.ang1, a.seq1 = self.rot1.data_ptr(), self.trans1.data_ptr(), self.ang1.data_ptr(), self.seq1.data_ptr()
        a.gen_mask, a.res_mask = self.gen.data_ptr(), engine.mask.data_ptr()
        a.rot_t, a.trans_t, a.ang_t, a.seq_t = engine.rot_t.data_ptr(), engine.trans_t.data_ptr(), engine.ang_t.data_ptr(), engine.seq_t.data_ptr()
        a.simplex_t, a.trans0, a.simplex0 = self.simplex_t.data_ptr(), self.trans0.data_ptr(), self.simplex0.data_ptr()
        a.pred_rot, a.pred_trans = engine.rot.data_ptr(), engine.trans.data_ptr()
        a.pred_ang_raw, a.pred_logits = engine.ang_raw.data_ptr(), engine.logits.data_ptr()
        a.traj_rot, a.traj_trans, a.traj_ang = self.traj_rot.data_ptr(), self.traj_trans.data_ptr(), self.traj_ang.data_ptr()
        a.traj_seq, a.traj_simplex = self.traj_seq.data_ptr(), self.traj_simplex.data_ptr()
        a.ts, a.num_steps, a.step, a.t_out = self.ts.data_ptr(), num_steps, self.step.data_ptr(), engine.t.data_ptr()
        a.expo, a.seed, a.first_sample = None, seed & (2 ** 64 - 1), first_sample
        a.B, a.L = B, L
        a.sample_bb, a.sample_ang, a.sample_seq = (int(f) for f in flags)
        # Philox key in device memory (pf_sampler_args.seed_dev): a captured graph then serves every later call
        self.seed_dev = e(2, dt=torch.int64)
        a.seed_dev = self.seed_dev.data_ptr()
        # ... and the GLOBAL index of every local sample (pf_sampler_args.sample_ids, ABI 56): first_sample + b for a contiguous
        # shard (set_seed), the caller's own indices for a length bucket of a ragged batch (set_sample_ids, buckets.py)
        self.sample_ids = e(B, dt=torch.int64)
        a.sample_ids = self.sample_ids.data_ptr()
        self.args = a
        # conditioned calls (pf_sampler_*_cond): the constraint planes and the start state live in buffers THIS sampler owns, so the
        # pointers a captured graph bakes in never move; a call only rewrites their contents (set_cond)
        self.cond = bool(cond)
        if self.cond:
            self.res_flags, self.aa_allowed = e(rows, dt=torch.uint8), e(rows, dt=torch.int32)
            self.start_rot, self.start_trans, self.start_ang = e(rows, 9), e(rows, 3), e(rows, 5)
            self.start_seq = e(rows, dt=torch.int64)
            self.cargs = _capi.SamplerCondArgs()
        # guided calls (pf_guidance_fwd between the network and the step kernel): the parameters, the hot-spot plane, the restraint
        # list, the guided copy of the prediction and the per-step records live in buffers THIS sampler owns; the step kernel reads
        # the guided copy.  A call only rewrites the buffers' contents (set_guide), so the captured graphs keep serving.
        self.guide = bool(guide)
        if self.guide:
            n_pairs = _capi.GUIDE_MAX_PAIRS
            self.g_params, self.g_hot = e(_capi.GUIDE_NPARAMS), e(rows, dt=torch.uint8)
            self.g_pair_idx, self.g_pair_par = e(B, n_pairs, 2, dt=torch.int32), e(B, n_pairs, 3)
            self.guided_trans = e(rows, 3)
            self.g_energy, self.g_shift = e(num_steps, B, _capi.GUIDE_NTERMS), e(num_steps, B)
            self.g_error = e(B, dt=torch.int32)
            g = self.gargs = _capi.GuidanceArgs()
            g.pred_trans, g.trans1, g.gen_mask, g.res_mask = engine.trans.data_ptr(), a.trans1, a.gen_mask, a.res_mask
            g.pair_idx, g.pair_par, g.params = self.g_pair_idx.data_ptr(), self.g_pair_par.data_ptr(), self.g_params.data_ptr()
            g.ts, g.step, g.num_steps = a.ts, a.step, num_steps
            g.guided_trans, g.energy, g.shift_max = self.guided_trans.data_ptr(), self.g_energy.data_ptr(), self.g_shift.data_ptr()
            g.error, g.B, g.L, g.sample_bb = self.g_error.data_ptr(), B, L, a.sample_bb
            a.pred_trans = self.guided_trans.data_ptr()
        # tempered / stochastic calls (pf_sampler_temper between the guidance and the step kernel): the temperature plane, the tempered
        # copy of the logits, the parameters and the pre-drawn normals live in buffers THIS sampler owns.  A call only rewrites their
        # contents and says which of tau / gauss are NULL (set_temper, init_state); the step kernel reads the tempered copy when a
        # plane is given and the engine's logits otherwise.
        self.temper = bool(temper)
        if self.temper:
            self.t_tau, self.t_logits, self.t_params = e(rows), e(rows, 20), e(_capi.TEMPER_NPARAMS)
            self.t_gauss = e(max(num_steps - 1, 1), rows, 6)
            self._logits_ptr = a.pred_logits
            t = self.targs = _capi.SamplerTemperArgs()
            t.pred_logits, t.tempered_logits, t.tau = a.pred_logits, self.t_logits.data_ptr(), None
            t.rot_t, t.trans_t, t.gen_mask, t.res_flags = a.rot_t, a.trans_t, a.gen_mask, None
            t.ts, t.step, t.params, t.gauss = a.ts, a.step, self.t_params.data_ptr(), None
            t.seed_dev, t.sample_ids = a.seed_dev, a.sample_ids
            t.B, t.L, t.num_steps, t.sample_bb = B, L, num_steps, a.sample_bb
        # steered calls (pf_sampler_steer after the step kernel): parameters, group structure, number of groups, the uniforms, the
        # log-weights and the records live in buffers THIS sampler owns.  A call only rewrites their contents (set_steer, init_state),
        # so the captured graphs keep serving; whether the uniforms are supplied is part of the launch key.
        self.steer = bool(steer)
        if self.steer:
            assert self.guide, "a steered sampler weights its particles by the guidance energies: guide=True"
            f8 = torch.float64
            self.s_params, self.s_ngroups = e(_capi.STEER_NPARAMS, dt=f8), e(1, dt=torch.int32)
            self.s_group_ptr, self.s_members = e(B + 1, dt=torch.int32), e(B, dt=torch.int32)
            self.s_logw, self.s_eprev, self.s_u = e(B, dt=f8), e(B, dt=f8), e(num_steps, B, dt=f8)
            self.s_anc, self.s_code = e(num_steps, B, dt=torch.int32), e(num_steps, B, dt=torch.int32)
            self.s_logw_rec, self.s_ess = e(num_steps, B, dt=f8), e(num_steps, B, dt=f8)
            self._steer_host = None
            q = self.sargs = _capi.SamplerSteerArgs()
            q.energy, q.ts, q.step, q.params = self.g_energy.data_ptr(), a.ts, a.step, self.s_params.data_ptr()
            q.group_ptr, q.members, q.n_groups = self.s_group_ptr.data_ptr(), self.s_members.data_ptr(), self.s_ngroups.data_ptr()
            q.logw, q.eprev, q.u = self.s_logw.data_ptr(), self.s_eprev.data_ptr(), None
            q.seed_dev, q.sample_ids = a.seed_dev, a.sample_ids
            q.ancestors, q.logw_rec, q.ess, q.code = self.s_anc.data_ptr(), self.s_logw_rec.data_ptr(), self.s_ess.data_ptr(), self.s_code.data_ptr()
            q.rot_t, q.trans_t, q.ang_t, q.seq_t = a.rot_t, a.trans_t, a.ang_t, a.seq_t
            q.simplex_t, q.trans0, q.simplex0 = a.simplex_t, a.trans0, a.simplex0
            q.B, q.L, q.num_steps, q.max_group = B, L, num_steps, 1
        self.graph = None
        self.graph_k = None
        self._graph_key = None
        self._so, self._steps_done = None, 0
        self.set_seed(seed, first_sample)

    @property
    def precision(self):
        """the engine's precision mode: what FlowModel's range verdict names (BucketedSampler has the same two members)"""
        return self.eng.precision

    def operand_range(self):
        """The engine's report of the largest activations it carried (DenoiseEngine.operand_range)."""
        return self.eng.operand_range()

    def begin(self, call, native, gen_mask, noise, seed, first_sample=0, sample_ids=None):
        """The set-up of one call, in this order: seed, grid, sample indices (a length bucket's), context, the extensions of `call` (a
        SampleCall fitted to this engine's samples and length), initial state.  native = (R1, x1, ang1, seq1) of encode().  Returns
        the noise the state was initialised from: a steered call's noise["resample_u"] [num_steps, G] cut to the columns of this
        sampler's groups (call.steer["group_ids"]): a bucket's own groups; on the unbucketed path group_ids = arange(G), so the
        selection is the identity there (one small host gather per steered call)."""
        kinds = call.kinds
        self.set_seed(seed, first_sample)
        self.set_grid(call.grid)
        if sample_ids is not None:
            self.set_sample_ids(sample_ids)
        self.set_context(*native, gen_mask)
        if kinds["cond"]:
            self.set_cond(call.cond, native)
        if kinds["guide"]:
            self.set_guide(call.guide)
        if kinds["temper"]:
            self.set_temper(call.temper)
        if kinds["steer"]:
            self.set_steer(call.steer)
            if noise.get("resample_u") is not None:
                noise = {**noise, "resample_u": noise["resample_u"][:, call.steer["group_ids"]].contiguous()}
        self.init_state(noise)
        return noise

    def set_seed(self, seed, first_sample=0):
        """Philox seed of the in-kernel categorical draws and the global index of this shard's first sample."""
        s = int(seed) & (2 ** 64 - 1)
        s = s - 2 ** 64 if s >= 2 ** 63 else s                          # uint64 bit pattern in an int64 tensor
        self.args.seed, self.args.first_sample = int(seed) & (2 ** 64 - 1), int(first_sample)
        if self.temper:                                 # (the noise kernel reads the key exactly as the step kernel does)
            self.targs.seed, self.targs.first_sample = self.args.seed, self.args.first_sample
        if self.steer:
            self.sargs.seed, self.sargs.first_sample = self.args.seed, self.args.first_sample
        self.seed_dev.copy_(torch.tensor([s, int(first_sample)], dtype=torch.int64))
        self.sample_ids.copy_(torch.arange(self.eng.B, dtype=torch.int64) + int(first_sample))

    def set_sample_ids(self, ids):
        """Global sample index of every local sample (int64 [B]) when they are not first_sample + b: keys the in-kernel Philox
        draws, so a re-ordered sub-batch draws what its samples draw in the caller's order."""
        ids = torch.as_tensor(ids, dtype=torch.int64).reshape(-1)
        assert ids.numel() == self.eng.B, (ids.numel(), self.eng.B)
        self.sample_ids.copy_(ids)

    def _launch_key(self):
        """Everything a captured graph has baked in besides device pointers that never move: the plan (pointer of block 0's pair
        input), the projection's kernel choice (active_rows hint), key-end lists on / off, caller-supplied categorical noise."""
        eng = self.eng
        key = (eng.plan_version, eng.active_rows, eng.padded, self.args.expo)
        if self.cond:                                   # which constraint planes the step kernel was launched with (NULL or the buffer)
            key += (self.cargs.res_flags, self.cargs.aa_allowed)
        if self.guide:                                  # ... and whether the guidance kernel was launched with a hot-spot plane
            key += (self.gargs.hotspots,)
        if self.temper:                                 # ... which of tau / gauss the noise kernel got (tau also decides the logits the step kernel reads)
            key += (self.targs.tau, self.targs.gauss)
        if self.steer:                                  # ... and whether the resampling uniforms are supplied (NULL: in-kernel Philox)
            key += (self.sargs.u,)
        return key

    def set_grid(self, grid):
        """The call's time grid (fp32 CPU tensor [num_steps], sampler.make_grid) into the device buffer the kernels and the captured
        graphs read.  EVERY call writes it: the sampler is cached, and a default call after a t_start call gets the default grid back."""
        assert grid.shape == (self.N,) and grid.dtype == torch.float32, (grid.shape, grid.dtype)
        self.ts.copy_(grid)

    def set_cond(self, cond, native):
        """The call's conditioning (sampler.make_cond, padded to the engine's length) into the owned buffers.  native = (R1, x1, ang1, seq1)
        of encode(): the start state's default, entry by entry."""
        assert self.cond, "a sampler built without cond=True has no constraint buffers"
        rows, c = self.eng.rows, self.cargs
        plane, allowed = cond.get("res_flags"), cond.get("aa_allowed")
        if plane is not None:
            self.res_flags.copy_(plane.reshape(rows))
        if allowed is not None:
            self.aa_allowed.copy_(allowed.reshape(rows))
        c.res_flags = self.res_flags.data_ptr() if plane is not None else None
        c.aa_allowed = self.aa_allowed.data_ptr() if allowed is not None else None
        c.partial = int(bool(cond["partial"]))
        if c.partial:
            for buf, key, nat, w in ((self.start_rot, "rotmats", native[0], 9), (self.start_trans, "trans", native[1], 3),
                                     (self.start_ang, "angles", native[2], 5), (self.start_seq, "seqs", native[3], 1)):
                src = cond.get(key)
                buf.copy_((nat if src is None else src).reshape(buf.shape))
        c.start_rot, c.start_trans = self.start_rot.data_ptr(), self.start_trans.data_ptr()
        c.start_ang, c.start_seq = self.start_ang.data_ptr(), self.start_seq.data_ptr()

    def set_guide(self, guide):
        """The call's guidance (sampler.make_guide, hot-spot plane padded to the engine's length) into the owned buffers; the
        per-step records start from zero."""
        assert self.guide, "a sampler built without guide=True has no guidance buffers"
        B, rows = self.eng.B, self.eng.rows
        assert guide["pair_idx"].shape == self.g_pair_idx.shape and guide["pair_par"].shape == self.g_pair_par.shape, guide["pair_idx"].shape
        self.g_params.copy_(guide["params"])
        self.g_pair_idx.copy_(guide["pair_idx"])
        self.g_pair_par.copy_(guide["pair_par"])
        hot = guide.get("hotspots")
        if hot is not None:
            self.g_hot.copy_(hot.reshape(rows))
        self.gargs.hotspots = self.g_hot.data_ptr() if hot is not None else None
        self.g_energy.zero_()
        self.g_shift.zero_()
        self.g_error.zero_()

    def set_temper(self, temper):
        """The call's tempering (sampler.make_temper, temperature plane padded to the engine's length) into the owned buffers.  With a
        plane the step kernel draws from the tempered copy of the logits, without one from the engine's own."""
        assert self.temper, "a sampler built without temper=True has no tempering buffers"
        self.t_params.copy_(temper["params"])
        tau = temper.get("tau")
        if tau is not None:
            self.t_tau.copy_(tau.reshape(self.eng.rows))
        self.targs.tau = self.t_tau.data_ptr() if tau is not None else None
        self.args.pred_logits = self.t_logits.data_ptr() if tau is not None else self._logits_ptr

    def set_steer(self, steer):
        """The call's steering (sampler.make_steer / fit_steer) into the owned buffers; the log-weights, eprev and the records start
        from zero, the ancestor record from the identity."""
        assert self.steer, "a sampler built without steer=True has no steering buffers"
        B = self.eng.B
        assert steer["members"].shape == (B,) and steer["group_ptr"].shape == (B + 1,), steer["members"].shape
        self.s_params.copy_(steer["params"])
        self.s_group_ptr.copy_(steer["group_ptr"])
        self.s_members.copy_(steer["members"])
        self.s_ngroups.fill_(int(steer["n_groups"]))
        self.sargs.max_group = int(steer["max_group"])
        self._steer_host = steer
        self._reset_steer()

    def _reset_steer(self):
        """a run starts from zero log-weights, zero eprev and empty records; the ancestor record from the identity"""
        for buf in (self.s_logw, self.s_eprev, self.s_logw_rec, self.s_ess, self.s_code):
            buf.zero_()
        self.s_anc.copy_(torch.arange(self.eng.B, dtype=torch.int32).expand(self.N, self.eng.B))

    def steering(self):
        """The records of a steered run as CPU tensors: ancestors int64 [num_steps, B] (local sample index; steer_lineage reads a
        particle's path from it), logw [num_steps, B] (after each step's update, before a reset), ess and code [num_steps, G] (0 no
        moment, 1 a moment above the threshold, 2 resampled, -1 degenerate), groups int64 [B] (group number of every sample) and
        weights [B]: the FINAL log-weights normalised per group, for the weighted ensemble (there is no resampling at the last step)."""
        st = self._steer_host
        G, of = st["n_groups"], st["group_of"].to(torch.int64)
        logw = self.s_logw.cpu()
        top = torch.full((G,), -math.inf, dtype=torch.float64).scatter_reduce(0, of, logw, "amax")
        w = torch.where(torch.isfinite(top)[of], torch.exp(logw - top[of]), torch.zeros_like(logw))
        tot = torch.zeros(G, dtype=torch.float64).index_add_(0, of, w)
        return {"ancestors": self.s_anc.cpu().to(torch.int64), "logw": self.s_logw_rec.cpu(), "ess": self.s_ess.cpu()[:, :G].contiguous(),
                "code": self.s_code.cpu()[:, :G].contiguous(), "groups": of.clone(), "group_ids": st["group_ids"].clone(),
                "weights": torch.where(tot[of] > 0, w / tot[of], torch.full_like(w, math.nan))}

    def guidance(self):
        """The records of a guided run as CPU tensors: energy [num_steps, B, 5] (the terms of every step's UNGUIDED prediction, in the
        order of GUIDE_TERMS), shift_max [num_steps, B].  Raises if the kernel refused a restraint index."""
        err = self.g_error.cpu()
        if bool((err != 0).any()):
            raise _capi.PepflowHipError(f"pf_guidance_fwd refused a restraint index outside the sample (samples {err.nonzero().flatten().tolist()})")
        return {"energy": self.g_energy.cpu(), "shift_max": self.g_shift.cpu(), "terms": GUIDE_TERMS}

    def set_context(self, R1, x1, ang1, seq1, gen_mask):
        rows = self.eng.rows
        self.rot1.copy_(R1.reshape(rows, 9))
        self.trans1.copy_(x1.reshape(rows, 3))
        self.ang1.copy_(ang1.reshape(rows, 5))
        self.seq1.copy_(seq1.reshape(rows))
        self.gen.copy_(gen_mask.reshape(rows).to(torch.float32))
        # the last block's tail only has to produce the generated residues' predictions (everything else is replaced by the context,
        # flow_model.py:291-311): its row tiles without one are skipped.  (DeviceSampler.SKIP_CONTEXT_ROWS = False: all rows, A/B runs)
        self.eng.want_rows(self.gen if self.SKIP_CONTEXT_ROWS else None)

    def init_state(self, noise):
        dev, rows = self.eng.device, self.eng.rows
        up = lambda k, n: noise[k].to(dev, torch.float32).reshape(rows, n).contiguous()
        rot0, tr0, ang0, sx0 = up("rot0", 9), up("trans0", 3), up("ang0", 5), up("simplex0", 20)
        if noise.get("expo") is not None:
            self.expo = noise["expo"].to(dev, torch.float32).contiguous()
            assert self.expo.shape == (2 * self.N, self.eng.B, self.eng.L, 20), self.expo.shape
            self.args.expo = self.expo.data_ptr()
        else:
            self.expo, self.args.expo = None, None
        if self.temper:                                # pre-drawn normals of the state noise, or NULL: the kernel draws (Philox)
            g = noise.get("gauss")
            if g is not None:
                assert tuple(g.shape) == (self.N - 1, self.eng.B, self.eng.L, 6), g.shape
                if self.N > 1:
                    self.t_gauss.copy_(g.reshape(self.t_gauss.shape))
            self.targs.gauss = self.t_gauss.data_ptr() if g is not None else None
        if self.steer:                                 # pre-drawn resampling uniforms [num_steps, G] (column = group), or NULL: the kernel draws
            u = noise.get("resample_u")
            if u is not None:
                assert tuple(u.shape) == (self.N, self._steer_host["n_groups"]), u.shape
                self.s_u[:, :u.shape[1]].copy_(u.to(torch.float64))
            self.sargs.u = self.s_u.data_ptr() if u is not None else None
            self._reset_steer()                        # (a run that starts over, e.g. after the buckets' calibration probes, starts its weights over)
        if self.cond:
            rc = self.lib.pf_sampler_init_cond(C.byref(self.args), C.byref(self.cargs), rot0.data_ptr(), tr0.data_ptr(), ang0.data_ptr(),
                                               sx0.data_ptr(), _capi.stream_ptr())
            _capi.check(rc, "pf_sampler_init_cond")
        else:
            rc = self.lib.pf_sampler_init(C.byref(self.args), rot0.data_ptr(), tr0.data_ptr(), ang0.data_ptr(),
                                          sx0.data_ptr(), _capi.stream_ptr())
            _capi.check(rc, "pf_sampler_init")
        self._init_keep = (rot0, tr0, ang0, sx0)
        self._so = None                                # (a streamed trajectory copy belongs to ONE run from step 0; see run(stream_out=True))
        self._steps_done = 0

    def _one_step(self):
        self.eng.run(concurrent=self.CONCURRENT)
        if self.guide:                                  # the guided copy of the translation prediction: what the step kernel reads
            self.gargs.res_flags = self.cargs.res_flags if self.cond else None
            rc = self.lib.pf_guidance_fwd(C.byref(self.gargs), _capi.stream_ptr())
            _capi.check(rc, "pf_guidance_fwd")
        if self.temper:                                 # tempered logits and the noise on the state the step kernel steps from
            self.targs.res_flags = self.cargs.res_flags if self.cond else None
            rc = self.lib.pf_sampler_temper(C.byref(self.targs), _capi.stream_ptr())
            _capi.check(rc, "pf_sampler_temper")
        if self.cond:
            rc = self.lib.pf_sampler_step_cond(C.byref(self.args), C.byref(self.cargs), _capi.stream_ptr())
            _capi.check(rc, "pf_sampler_step_cond")
        else:
            rc = self.lib.pf_sampler_step(C.byref(self.args), _capi.stream_ptr())
            _capi.check(rc, "pf_sampler_step")
        if self.steer:                                  # weigh the particles by this step's energies; resample the state the next step starts from
            rc = self.lib.pf_sampler_steer(C.byref(self.sargs), _capi.stream_ptr())
            _capi.check(rc, "pf_sampler_steer")

    SKIP_CONTEXT_ROWS = True  # the last block's tail only produces the generated residues' predictions (set_context)
    CONCURRENT = False        # projection(b + 1) on a side stream beside EdgeTransition(b): measured slower (DenoiseEngine.run)
    GRAPH_STEPS = 4          # steps per replayed graph: the host-side relaunch gap (~8 us) is paid once per replay

    def _capture(self, k):
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with _capi.capture_guard(), torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                for _ in range(k):
                    self._one_step()
        torch.cuda.current_stream().wait_stream(side)
        return g

    def capture(self):
        """Capture one step (network + flow update) into a hipGraph -- and GRAPH_STEPS consecutive steps into a second one:
        the step counter and the time live on the device, so every step is the same graph.  The engine runs once eagerly before
        its first capture (first-launch attribute setup must not happen under capture; the state it leaves behind is overwritten
        by init_state / the first step)."""
        if not self.eng._warm:
            self.eng.run()
        self.graph = self._capture(1)
        self.graph_k = self._capture(self.GRAPH_STEPS) if self.GRAPH_STEPS > 1 else None
        self._graph_key = self._launch_key()

    def needs_capture(self):
        return self.graph is None or self._graph_key != self._launch_key()

    STREAM_OUT_CHUNK = 32     # steps per streamed piece of the trajectory (run(stream_out=True))

    def _traj_tensors(self):
        return (self.traj_rot, self.traj_trans, self.traj_ang, self.traj_seq, self.traj_simplex)

    def _stream_chunk(self, upto):
        """Steps [copied, upto) of the five trajectory buffers -> their pinned host twins, on the copy stream, behind an event recorded
        on the compute stream HERE (the host runs ahead of the device: the event orders the copy behind the steps it copies)."""
        so = self._so
        if so is None or upto <= so["copied"]:
            return
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        with torch.cuda.stream(so["stream"]):
            so["stream"].wait_event(ev)
            for h, t in zip(so["hosts"], self._traj_tensors()):
                h[so["copied"]:upto].copy_(t[so["copied"]:upto], non_blocking=True)
        so["copied"] = upto

    def run(self, n_steps=None, use_graph=True, stream_out=False):
        """stream_out: copy the trajectory to pinned host memory WHILE the loop runs (pieces of STREAM_OUT_CHUNK steps on a copy stream;
        trajectory() then only waits for the last piece): the D2H of a 200-step call of B = 64 x 128 is 280 MB = 5 ms at the PCIe rate,
        1 % of the call, otherwise spent after the loop with the device idle.  Only for a run that starts at step 0 (init_state)."""
        n = self.N if n_steps is None else n_steps
        if stream_out and self._steps_done == 0 and use_graph:
            copy_stream = getattr(self, "_copy_stream", None)
            if copy_stream is None:
                copy_stream = self._copy_stream = torch.cuda.Stream(device=self.eng.device)
            self._so = dict(stream=copy_stream, copied=0, hosts=[torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in self._traj_tensors()])
        else:
            self._so = None
        if not use_graph:
            for _ in range(n):
                self._one_step()
            self._steps_done += n
            return
        if self.needs_capture():
            self.capture()
        k, done = self.GRAPH_STEPS, self._steps_done
        self._steps_done += n
        if self.graph_k is not None:
            for _ in range(n // k):
                self.graph_k.replay()
                done += k
                if self._so is not None and done - self._so["copied"] >= self.STREAM_OUT_CHUNK:
                    self._stream_chunk(done)
            n -= (n // k) * k
        for _ in range(n):
            self.graph.replay()
        if self._so is not None:
            self._stream_chunk(min(self._steps_done, self.N))

    def trajectory(self, pageable=False):
        """One D2H copy -> list of num_steps dicts of CPU tensors (flow_model.py:313-314,371-374).
        The tensors are VIEWS of pinned host buffers (PyTorch's caching host allocator recycles them once the views die).  A caller
        that ACCUMULATES trajectories over many complexes should pass pageable=True (FlowModel.sample(..., pageable=True)): the
        result is then copied into ordinary pageable memory and the pinned staging blocks return to the allocator at once."""
        B, L, N = self.eng.B, self.eng.L, self.N
        Lo = getattr(self, "L_out", L)                 # FlowModel.sample pads the residue axis to x16 internally: cut back

        def to_host(t):
            # pinned destination (PyTorch's caching host allocator recycles the blocks of earlier calls): the copy then runs at
            # the PCIe rate instead of the pageable-memory rate (measured 20 -> 5 ms for the 200-step trajectory of B=64 x 128)
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t, non_blocking=True)
            return h
        so, self._so = getattr(self, "_so", None), None
        if so is not None and so["copied"] == N and self._steps_done == N:
            so["stream"].synchronize()                 # the whole trajectory went out while the loop ran (run(stream_out=True))
            hosts = so["hosts"]
        else:
            hosts = [to_host(t) for t in (self.traj_rot, self.traj_trans, self.traj_ang, self.traj_seq, self.traj_simplex)]   # (also BucketedSampler's gathered buffers)
        torch.cuda.current_stream().synchronize()
        if pageable:
            hosts = [torch.empty(h.shape, dtype=h.dtype).copy_(h) for h in hosts]
        rot = hosts[0].view(N, B, L, 3, 3)[:, :, :Lo]
        trans = hosts[1].view(N, B, L, 3)[:, :, :Lo]
        ang = hosts[2].view(N, B, L, 5)[:, :, :Lo]
        seq = hosts[3].view(N, B, L)[:, :, :Lo]
        sx = hosts[4].view(N, B, L, 20)[:, :, :Lo]
        R1, x1 = self.rot1.cpu().view(B, L, 3, 3)[:, :Lo], self.trans1.cpu().view(B, L, 3)[:, :Lo]
        a1, s1 = self.ang1.cpu().view(B, L, 5)[:, :Lo], self.seq1.cpu().view(B, L)[:, :Lo]
        return [{"rotmats": rot[i], "trans": trans[i], "angles": ang[i], "seqs": seq[i], "seqs_simplex": sx[i],
                 "rotmats_1": R1, "trans_1": x1, "angles_1": a1, "seqs_1": s1} for i in range(N)]
