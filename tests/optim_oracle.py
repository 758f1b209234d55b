"""numpy float64 restatement of the optimizer block of a training iteration (train.py:135-146 of the reference): NaN gradient
entries -> 0, clip_grad_norm_(max_norm) with its coefficient min(1, max_norm / (total_norm + 1e-6)), then Adam (L2 weight decay) or
AdamW (decoupled) with bias corrections bc1 = 1 - beta1^t, bc2 = 1 - beta2^t, t = step + 1.  Works on the fp32 INPUT values in float64;
tests/test_optim_cpu.py pins it to torch.optim.Adam / AdamW + clip_grad_norm_ on the CPU."""
import math

import numpy as np


def f64(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def grad_norm(grads):
    """-> (total_norm, nan_count, has_inf) over the given gradients (None = inactive), NaN entries counted as 0"""
    sq, nans, inf = 0.0, 0, False
    for g in grads:
        if g is None:
            continue
        g = f64(g)
        nan = np.isnan(g)
        nans += int(nan.sum())
        inf = inf or bool(np.isinf(g).any())
        with np.errstate(over="ignore"):
            sq += float(np.square(np.where(nan, 0.0, g)).sum())
    return math.sqrt(sq), nans, inf


def clip_coef(total_norm, max_norm):
    if max_norm is None or not max_norm > 0:
        return 1.0
    return min(1.0, max_norm / (total_norm + 1e-6))


def adam_update(p, g, m, v, step, coef, lr, beta1, beta2, eps, weight_decay, decoupled):
    """one tensor: -> (p, exp_avg, exp_avg_sq) after the update with t = step + 1; all float64"""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    g = coef * np.where(np.isnan(g), 0.0, g)
    if decoupled:
        p = p * (1.0 - lr * weight_decay)
    else:
        g = g + weight_decay * p
    t = step + 1
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    p = p - (lr / bc1) * m / (np.sqrt(v) / math.sqrt(bc2) + eps)
    return p, m, v


def step(params, grads, exp_avg, exp_avg_sq, steps, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False,
         max_norm=None):
    """The whole block over a list of tensors (fp32 values in, float64 out).  grads[i] None: tensor i and its counter stay.
    -> dict(params, exp_avg, exp_avg_sq, steps, grad_norm, nan_count, skipped); an inf gradient entry skips the update."""
    total, nans, inf = grad_norm(grads)
    out = dict(params=[f64(x) for x in params], exp_avg=[f64(x) for x in exp_avg], exp_avg_sq=[f64(x) for x in exp_avg_sq],
               steps=list(steps), grad_norm=math.inf if inf else total, nan_count=nans, skipped=bool(inf))
    if inf:
        return out
    coef = clip_coef(total, max_norm)
    for i, g in enumerate(grads):
        if g is None:
            continue
        out["params"][i], out["exp_avg"][i], out["exp_avg_sq"][i] = adam_update(
            params[i], g, exp_avg[i], exp_avg_sq[i], steps[i], coef, lr, betas[0], betas[1], eps, weight_decay, decoupled)
        out["steps"][i] = steps[i] + 1
    return out
