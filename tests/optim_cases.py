"""The one small tensor set of the optimizer tests, its six gradient steps, the configurations, and the two runners: the torch
reference block on the CPU (NaN loop, clip_grad_norm_, torch.optim.Adam / AdamW in fp32: train.py:135-146 of the reference) and
FusedAdam on a device.  Both runners record, per step and tensor, the state before and after the step; `deviations` compares a run
with the float64 oracle applied to the run's OWN fp32 state before each step (one-step form: nothing accumulates)."""
import functools

import numpy as np
import torch

import optim_oracle as OO
from pepflowww_amd.optim import CHUNK

LR, BETAS, EPS = 5e-4, (0.9, 0.999), 1e-8
# name -> (shape, scale of the initial values).  "odd_view" is a contiguous view at element offset 1 of a larger storage (4-byte
# aligned only); "no_grad" never gets a gradient; "zero" starts at exactly 0 and "small" at 1e-3 scale, so an error of the bias
# correction is not hidden under the parameter's own rounding.
TENSORS = (("one", (1,), 0.05), ("three", (3,), 0.05), ("mat", (5, 7), 0.05), ("chunk_m1", (CHUNK - 1,), 0.05),
           ("chunk", (CHUNK,), 0.05), ("chunk_p1", (CHUNK + 1,), 0.05), ("chunks", (3 * CHUNK + 5,), 0.05),
           ("odd_view", (1027,), 0.05), ("zero", (64,), 0.0), ("small", (257,), 1e-3), ("no_grad", (10,), 0.05))
NAMES = tuple(t[0] for t in TENSORS)
# gradient scale per step; total numel is about 26 k, so the norm is about 160 x scale: against max_norm 100 the steps are inactive,
# mild (1.3), strong (49), inactive, zero, inactive; against max_norm 1 strong, strong, strong, inactive (0.49), zero, mild (1.3).
SCALES = (0.1, 0.8, 30.0, 0.003, 0.0, 0.008)
NAN_STEPS = (1, 3)                       # steps whose gradients hold NaN entries (numel-1 tensor included)
LR_CHANGE_AT = 3                         # param_groups[0]['lr'] is halved before this step
CONFIGS = {"adam_ref": dict(weight_decay=0.0, decoupled=False, max_norm=100.0),          # configs/learn_angle.yaml
           "adam_l2": dict(weight_decay=0.01, decoupled=False, max_norm=1.0),
           "adamw": dict(weight_decay=0.01, decoupled=True, max_norm=100.0),
           "noclip": dict(weight_decay=0.0, decoupled=False, max_norm=None)}


def make_params(device="cpu", seed=0):
    """fresh leaf tensors (requires_grad) on `device`, the same values for every device"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for name, shape, scale in TENSORS:
        v = torch.randn(*shape, generator=g) * scale
        if name == "odd_view":
            store = torch.zeros(v.numel() + 8, device=device)
            p = store[1:1 + v.numel()].view(shape)
            p.copy_(v)
        else:
            p = v.to(device).clone()
        assert p.is_contiguous() and p.is_leaf
        out.append(p.requires_grad_())
    return out


@functools.lru_cache(maxsize=None)
def make_grads(step, seed=100):
    """CPU gradients of one step: a tuple of fp32 tensors (None for "no_grad")"""
    g = torch.Generator().manual_seed(seed + step)
    out = []
    for i, (name, shape, _) in enumerate(TENSORS):
        if name == "no_grad":
            out.append(None)
            continue
        v = torch.randn(*shape, generator=g) * SCALES[step]
        if step in NAN_STEPS:
            flat = v.view(-1)
            flat[::max(1, flat.numel() // 3)] = float("nan")     # numel 1: the whole gradient
        out.append(v)
    return tuple(out)


def _np(t):
    return t.detach().cpu().numpy().copy()


def run_torch(config, n_steps=len(SCALES)):
    """the reference block on the CPU -> list of records (see _record)"""
    c = CONFIGS[config]
    params = make_params("cpu")
    cls = torch.optim.AdamW if c["decoupled"] else torch.optim.Adam
    opt = cls(params, lr=LR, betas=BETAS, eps=EPS, weight_decay=c["weight_decay"])

    def state():
        return ([_np(p) for p in params],
                [_np(opt.state[p]["exp_avg"]) if p in opt.state else np.zeros(p.shape, np.float32) for p in params],
                [_np(opt.state[p]["exp_avg_sq"]) if p in opt.state else np.zeros(p.shape, np.float32) for p in params],
                [int(opt.state[p]["step"]) if p in opt.state else 0 for p in params])
    recs = []
    for k in range(n_steps):
        if k == LR_CHANGE_AT:
            opt.param_groups[0]["lr"] *= 0.5
        grads = make_grads(k)
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.clone()
        before = state()
        for p in params:                                         # train.py:135-139
            if p.grad is not None and torch.isnan(p.grad).any():
                p.grad[torch.isnan(p.grad)] = 0
        norm = 0.0
        if c["max_norm"] is not None:
            norm = float(torch.nn.utils.clip_grad_norm_(params, c["max_norm"]))
        opt.step()
        recs.append(dict(step=k, lr=opt.param_groups[0]["lr"], before=before, after=state(), grad_norm=norm))
    return recs, opt, params


def torch_one_step(before, grads, lr, weight_decay=0.0, decoupled=False, max_norm=None):
    """The reference block in fp32 on the CPU for ONE step from a given fp32 state (p, exp_avg, exp_avg_sq, steps as lists of numpy
    arrays / ints; grads: numpy arrays or None) -> (p, exp_avg, exp_avg_sq) after it.  This is the reference whose own deviation from
    the oracle, on the SAME inputs, sizes the tolerance of the GPU tests."""
    P, M, V, S = before
    params = [torch.from_numpy(np.array(p, dtype=np.float32)).requires_grad_() for p in P]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls(params, lr=lr, betas=BETAS, eps=EPS, weight_decay=weight_decay)
    for p, g, m, v, s in zip(params, grads, M, V, S):
        p.grad = None if g is None else torch.from_numpy(np.array(g, dtype=np.float32))
        opt.state[p] = {"step": torch.tensor(float(s)), "exp_avg": torch.from_numpy(np.array(m, dtype=np.float32)),
                        "exp_avg_sq": torch.from_numpy(np.array(v, dtype=np.float32))}
    for p in params:                                             # train.py:135-139
        if p.grad is not None and torch.isnan(p.grad).any():
            p.grad[torch.isnan(p.grad)] = 0
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(params, max_norm)
    opt.step()
    return ([_np(p) for p in params], [_np(opt.state[p]["exp_avg"]) for p in params], [_np(opt.state[p]["exp_avg_sq"]) for p in params])


def check_step(after, oracle, reference, names, what=""):
    """The rule of the GPU value tests: per tensor, max |kernel - oracle| <= 4 x max |torch fp32 - oracle| (the reference's own deviation
    on the same inputs) + one fp32 ulp of the tensor's largest magnitude.  -> [(name, quantity, kernel deviation, reference deviation,
    tolerance)], asserting every row."""
    rows = []
    for q, key in enumerate(("params", "exp_avg", "exp_avg_sq")):
        for i, name in enumerate(names):
            want = oracle[key][i]
            d_k = float(np.abs(after[q][i].astype(np.float64) - want).max())
            d_r = float(np.abs(reference[q][i].astype(np.float64) - want).max())
            tol = 4.0 * d_r + ulp32(float(np.abs(want).max()))
            rows.append((name, "pmv"[q], d_k, d_r, tol))
    bad = [r for r in rows if not r[2] <= r[4]]
    assert not bad, (what, len(bad), bad[:6])
    return rows


def run_fused(config, device, n_steps=len(SCALES), extra=None, opt=None, params=None, first_step=0):
    """FusedAdam on `device` over the same steps -> (records, optimizer, params).  extra: further (parameter, gradient) CPU pairs put in
    FRONT of the table (the independence test); opt / params / first_step: continue a given optimizer."""
    from pepflowww_amd.optim import FusedAdam
    c = CONFIGS[config]
    if params is None:
        params = make_params(device)
    extra = extra or []
    extras = [p.to(device).clone().requires_grad_() for p, _ in extra]
    if opt is None:
        opt = FusedAdam(extras + params, lr=LR, betas=BETAS, eps=EPS, weight_decay=c["weight_decay"],
                        decoupled_weight_decay=c["decoupled"], max_grad_norm=c["max_norm"])

    def state():
        return ([_np(p) for p in params], [_np(opt.state[p]["exp_avg"]) for p in params],
                [_np(opt.state[p]["exp_avg_sq"]) for p in params], [int(opt.state[p]["step"]) for p in params])
    recs = []
    for k in range(first_step, first_step + n_steps):
        if k == LR_CHANGE_AT:
            opt.param_groups[0]["lr"] *= 0.5
        grads = make_grads(k)
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.to(device)         # a new address every step: the pointer table is refreshed
        for p, (_, g) in zip(extras, extra):
            p.grad = g.to(device)
        before = state()
        torch.cuda.set_sync_debug_mode("error")                  # step() performs no host read (any synchronising call raises here)
        try:
            opt.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        recs.append(dict(step=k, lr=opt.param_groups[0]["lr"], before=before, after=state(), grad_norm=float(opt.last_grad_norm),
                         nan_count=int(opt.last_nan_count), skipped=int(opt.skipped_steps)))
    return recs, opt, params


def oracle_of(rec, config, grads=None):
    """the float64 oracle's step from the record's own fp32 state before the step"""
    c = CONFIGS[config]
    p, m, v, steps = rec["before"]
    grads = make_grads(rec["step"]) if grads is None else grads
    return OO.step(p, [None if g is None else g.numpy() for g in grads], m, v, steps, rec["lr"], BETAS, EPS,
                   c["weight_decay"], c["decoupled"], c["max_norm"])


def deviations(recs, config):
    """-> {(step, tensor name, 'p' | 'm' | 'v'): (max |run - oracle|, max |oracle|)}, and the oracle's per-step (grad_norm, nan_count)"""
    dev, norms = {}, []
    for rec in recs:
        o = oracle_of(rec, config)
        norms.append((o["grad_norm"], o["nan_count"]))
        assert o["steps"] == rec["after"][3], (rec["step"], o["steps"], rec["after"][3])
        for q, key in enumerate(("params", "exp_avg", "exp_avg_sq")):
            for i, name in enumerate(NAMES):
                got, want = rec["after"][q][i].astype(np.float64), o[key][i]
                dev[(rec["step"], name, "pmv"[q])] = (float(np.abs(got - want).max()), float(np.abs(want).max()))
    return dev, norms


@functools.lru_cache(maxsize=None)
def reference_deviations(config):
    """torch's own fp32 deviation from the oracle (computed once per configuration, shared by the tests)"""
    recs, _, _ = run_torch(config)
    return deviations(recs, config)


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))
