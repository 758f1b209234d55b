"""F19: one training step of the REFERENCE (six losses, gradient of the weighted loss with respect to every parameter) at
production lengths (tests/ref_shapes.py: F19_SHAPES), with its RNG draws recorded as in F4 and the per-parameter layout of F6:
`pg_i` in full for parameters of <= 65536 elements, `pp_i` / `ps_i` (tests/grad_probe.py) for larger ones, `param_gradnorms`,
and `param_fp32_noise` (the reference's fp32 gradient against the float64 autograd of the CPU restatement).  The gradients of
trunk intermediates that F6 holds are not stored.  Parameter i is entry i of tests/golden/f6_param_names.json.

Condition on the seed (the first of ten candidates that meets it is taken): at most 20 parameters have an fp32 noise above 3.2e-3,
edge_embedder.aapair_to_distcoef.weight (the known long cancelling sum) is one of them, and the smallest relative top-2 gap of a
categorical draw on a generated row is >= 2e-3.
Needs the reference code base (imported through oracle/tools/ref_shim.py).  Re-run: python tests/golden/make_golden_f19.py"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_shim  # noqa: E402
from pepflowww_amd import synth  # noqa: E402
import ref_shapes as S  # noqa: E402
from grad_probe import probe  # noqa: E402
from oracle import pepflow_oracle as O  # noqa: E402

torch.set_num_threads(8)
model, cfg = ref_shim.build_reference_model()
sd = synth.seeded_state_dict()
model.load_state_dict(sd, strict=True)
import models_con.flow_model as fm  # noqa: E402
import models_con.torus as torus  # noqa: E402

names = [n for n, _ in model.named_parameters()]
assert names == json.load(open(os.path.join(HERE, "f6_param_names.json")))
w = cfg.train.loss_weights
orig = dict(multinomial=torch.multinomial, rand=torch.rand, randn=torch.randn, randn_like=torch.randn_like,
            so3=fm.uniform_so3, tor=torus.tor_random_uniform)


def run(B, L, lengths, cand):
    """One reference forward + backward with recorded draws, and the same step through the restatement in float64."""
    batch = S.f19_batch(B, L, lengths, cand)
    seed = S.f19_noise_seed(L, cand)
    nz = synth.make_noise(B, L, 1, seed=seed)
    noise = {"t": torch.rand(B, 1, generator=torch.Generator().manual_seed(seed)), "trans0": nz["trans0"], "rot0": nz["rot0"],
             "ang0": nz["ang0"], "simplex0": nz["simplex0"]}
    rec, gaps = [], []
    gen = batch["generate_mask"].reshape(-1)

    def multinomial_rec(c, n, *a, **k):
        st = torch.get_rng_state()
        out = orig["multinomial"](c, n, *a, **k)
        torch.set_rng_state(st)
        Ex = torch.empty_like(c).exponential_(1)
        assert torch.equal(out[:, 0], torch.argmax(c / Ex, -1))
        top = torch.topk((c / Ex).detach(), 2, dim=-1).values
        gaps.append((1 - top[:, 1] / top[:, 0])[gen].min().item())
        rec.append(Ex.reshape(B, L, 20).clone())
        return out

    torch.multinomial = multinomial_rec
    torch.rand = lambda *s, **k: noise["t"].clone()
    torch.randn = lambda *s, **k: noise["trans0"].clone()
    torch.randn_like = lambda x, **k: noise["simplex0"].clone()
    fm.uniform_so3 = lambda nb, nr, device=None: noise["rot0"].clone()
    torus.tor_random_uniform = lambda *s, dtype=None, device=None: noise["ang0"].clone()
    torch.manual_seed(7)
    model.zero_grad(set_to_none=True)
    try:
        losses = model(batch)
    finally:
        torch.multinomial, torch.rand, torch.randn, torch.randn_like = orig["multinomial"], orig["rand"], orig["randn"], orig["randn_like"]
        fm.uniform_so3, torus.tor_random_uniform = orig["so3"], orig["tor"]
    assert len(rec) == 2
    sum(w[k] * losses[k] for k in losses).backward()
    noise["expo"] = torch.stack(rec, 0)
    grads = [p.grad.detach().clone() for _, p in model.named_parameters()]

    # intrinsic fp32 noise of the reference's own gradient (make_golden_f6.py): the same step through the restatement in float64
    dt = torch.float64
    sd64 = {k: (v.to(dt) if v.is_floating_point() else v).clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    b64 = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in batch.items()}
    n64 = {k: v.to(dt) for k, v in noise.items()}
    keep = O.BB_IDEAL
    O.BB_IDEAL = O.BB_IDEAL.to(dt)
    try:
        l64 = O.forward_losses(sd64, b64, n64)
        sum(float(w[k]) * v for k, v in l64.items()).backward()
    finally:
        O.BB_IDEAL = keep
    lvl = [float((g.to(dt) - sd64[n].grad).abs().max() / sd64[n].grad.abs().max().clamp_min(1e-30)) for n, g in zip(names, grads)]
    loose = {n: v for n, v in zip(names, lvl) if v > S.F19_LOOSE_NOISE and not n.endswith("linear_b.bias")}
    return batch, noise, {k: v.detach() for k, v in losses.items()}, grads, lvl, loose, min(gaps)


for B, L, lengths in S.F19_SHAPES:
    best = None
    for cand in range(10):
        r = run(B, L, lengths, cand)
        loose, gap = r[5], r[6]
        ok = len(loose) <= S.F19_MAX_LOOSE and S.F19_DISTCOEF in loose and gap >= S.F18_MIN_MARGIN
        print(f"F19 ({B}, {L}) candidate {cand}: {len(loose)} parameters with fp32 noise > {S.F19_LOOSE_NOISE:g}, "
              f"distcoef among them: {S.F19_DISTCOEF in loose}, smallest decision margin {gap:.2e}")
        if best is None or (gap >= S.F18_MIN_MARGIN and len(loose) < len(best[1][5])):
            best = (cand, r)
        if ok:
            best = (cand, r)
            break
    else:
        print("no candidate of ten meets the condition; storing the best one.  Parameters above the cap:", best[1][5])
    cand, (batch, noise, losses, grads, lvl, loose, gap) = best
    out = {"cand": torch.tensor(cand), "condition_met": torch.tensor(ok), "draw_gap": torch.tensor(gap, dtype=torch.float64),
           "param_gradnorms": torch.tensor([float(g.norm()) for g in grads]), "param_fp32_noise": torch.tensor(lvl)}
    out.update(noise)
    out.update({"loss_" + k: v for k, v in losses.items()})
    out.update({"batch_" + k: v for k, v in batch.items()})
    full, probes = {}, {}
    for i, g in enumerate(grads):
        if g.numel() <= 65536:
            full[f"pg_{i}"] = g
        else:
            probes[f"pp_{i}"], probes[f"ps_{i}"] = probe(g.reshape(-1), i)
    # the full tensors in as many parts as the size limit of a committed file asks for (by running size, in parameter order)
    parts, cur, run_bytes = {"step": {**out, **probes}}, {}, 0
    for k, g in full.items():
        if run_bytes + g.numel() * 4 > 900 * 1024 and cur:
            parts[f"pg{len(parts) - 1}"] = cur
            cur, run_bytes = {}, 0
        cur[k] = g
        run_bytes += g.numel() * 4
    parts[f"pg{len(parts) - 1}"] = cur
    sizes = S.save_parts(HERE, "f19_" + S.tag(B, L), parts)
    print(f"F19 ({B}, {L}) {lengths}, candidate {cand}: " + ", ".join(f"{n} {sz / 1024:.1f} KiB" for n, sz in sizes))
    nb = [v for n, v in zip(names, lvl) if not n.endswith("linear_b.bias")]
    print("  losses:", {k: float(v) for k, v in losses.items()})
    print(f"  fp32 noise of the reference gradient: median {sorted(nb)[len(nb) // 2]:.2e}, max {max(nb):.2e}; above the cap:",
          {n: f"{v:.2e}" for n, v in loose.items()})
print("done")
