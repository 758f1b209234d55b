"""Shared checker of ONE trunk block's backward against the float64 oracle, element-wise (plain module: no fixtures, no GPU, never
touches the library's kernels).

tests/train_oracle.py compares the 407 PARAMETER gradients of the whole step.  A parameter gradient is a sum over all B L rows or all
B L^2 pairs: an error that sits in one row tail, one last key chunk or one ragged workgroup reaches it scaled down by k / (B L) or
k / (B L^2).  The ACTIVATION gradients of the three block classes of pepflowww_amd/backward.py show such an error undiluted:
    IpaBlock.backward            -> g_s, g_z, g_trans, g_rot
    NodeTrackBlock.backward      -> g_a0
    EdgeTransitionBlock.backward -> g_s, g_z
This module builds, per (block, case), seeded inputs (`make_case`), moves them off the ReLU gates of the block (`condition`), takes the
oracle's autograd in float64 and in float32 (`truth`) and compares a set of tensors with the float64 one region by region (`compare`).

The block functions are the three pieces of one trunk block exactly as oracle/pepflow_oracle.py: ga_encoder composes them (BLOCK_FNS;
tests/test_block_oracle_cpu.py chains them on ga_encoder's own intermediates).  The ReLU pre-activations are read by recording what
O.lin returns for the gate layers while the block function runs, so nothing of the oracle is restated here.

The rule (`compare`), per tensor and region:  err = max|g - g64| / max|g64| <= REL + K_NOISE x noise, REL = 1e-4 the project's parity
bar for these tensors (tests/test_gpu_parity.py at (3, 24)), noise the same ratio for the oracle's own fp32 gradient, K_NOISE = 3 as
train_oracle.K_NOISE.  Regions, each normalised by its OWN maximum of |g64|, real rows / pairs only:
    whole            the whole tensor
    sample b         one sample
    tail b           the last min(16, len) real residues of sample b (row tensors)
    rowband b / colband b   the pairs (i, j) of sample b with i (j) among those residues (pair tensors)
    launch-tail      the rows beyond the last multiple of 4 rows / the pairs beyond the last multiple of 64 pairs of the whole launch
    masked           rows / pairs with a masked residue: finite, and exactly the truth's zero where `masked_zero` asks for it

Why `condition`: a ReLU gate whose pre-activation is zero to fp32 accuracy makes an element-wise comparison measure which side rounding
fell on (train_oracle.condition has the same for the head gates).  The condition is on the INPUT, from the oracle alone: no gate
pre-activation of a real row (node track: linear1 of both transformer layers, linear_1 / linear_2 of the transition) or real pair
(EdgeTransition: trunk.0, trunk.2) is closer to zero, in float64, than MARGIN_FACTOR = 5 x what the oracle's own fp32 forward misses
ANY gate pre-activation of that case by.  Offending pairs get their z_ij re-drawn; an offending node-track row gets ALL a0 rows of its
sample re-drawn (its rows couple through the attention: a per-row re-draw moves the other rows' gates).  IPA has no gate.
"""
import os
import sys
import time

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(_HERE), _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from oracle import pepflow_oracle as O  # noqa: E402
import train_oracle as T  # noqa: E402

REL = 1e-4                     # tests/test_gpu_parity.py: REL, the bar of these tensors at (3, 24)
K_NOISE = T.K_NOISE
FWD_REL = 2e-5                 # the saved-activation forwards against the oracle's fp32 forward (the F4-F6 block tests)
MARGIN_FACTOR = 5.0
MAX_ROUNDS = 20
TAIL = 16
BLOCK = 1                      # block index of synth.seeded_state_dict() the cases use
TP = "ga_encoder.trunk."


# ------------------------------------------------------------------------------------------------ the block functions
def ipa_fn(sd, b, mask):
    return lambda s, z, R, x: mask[..., None] * O.ipa(sd, f"{TP}ipa_{b}", s, z, R, x, mask)[0]


def node_fn(sd, b, mask):
    def f(a0):
        s1 = O.lnorm(sd, f"{TP}ipa_ln_{b}", a0)
        s2 = s1 + O.lin(sd, f"{TP}post_tfmr_{b}", O.seq_transformer(sd, f"{TP}seq_tfmr_{b}", s1, mask))
        return O.node_transition(sd, f"{TP}node_transition_{b}", s2) * mask[..., None]
    return f


def et_fn(sd, b, mask):
    emask = mask[:, None, :] * mask[:, :, None]
    return lambda s, z: O.edge_transition(sd, f"{TP}edge_transition_{b}", s, z) * emask[..., None]


BLOCK_FNS = {"ipa": ipa_fn, "node": node_fn, "et": et_fn}
INPUTS = {"ipa": ("s", "z", "R", "x"), "node": ("a0",), "et": ("s", "z")}
# what the library calls the gradient of each input (IpaBlock / NodeTrackBlock / EdgeTransitionBlock .backward)
GRAD_NAMES = {"ipa": ("g_s", "g_z", "g_rot", "g_trans"), "node": ("g_a0",), "et": ("g_s", "g_z")}
PARAM_PREFIXES = {"ipa": ("ipa_{b}.",), "node": ("ipa_ln_{b}.", "seq_tfmr_{b}.", "post_tfmr_{b}.", "node_transition_{b}."),
                  "et": ("edge_transition_{b}.",)}
GATES = {"ipa": (), "node": (".layers.0.linear1", ".layers.1.linear1", ".linear_1", ".linear_2"), "et": (".trunk.0", ".trunk.2")}


class _RecordGates:
    """What O.lin returns for the layers whose prefix ends in one of `suffixes`, while a block function runs."""

    def __init__(self, suffixes):
        self.suffixes = tuple(suffixes)

    def __enter__(self):
        self.pre, self._lin = {}, O.lin

        def lin(sd, pfx, x):
            y = self._lin(sd, pfx, x)
            if pfx.endswith(self.suffixes):
                self.pre[pfx] = y.detach()
            return y
        O.lin = lin
        return self.pre

    def __exit__(self, *exc):
        O.lin = self._lin


def block_params(sd, kind, b):
    """{name relative to ga_encoder.trunk. -> tensor} of the parameters of one block piece."""
    pre = tuple(TP + p.format(b=b) for p in PARAM_PREFIXES[kind])
    return {k[len(TP):]: v for k, v in sd.items() if k.startswith(pre)}


# ------------------------------------------------------------------------------------------------ cases
# (B, L, lengths, hole): hole = a masked residue INSIDE sample 0 (None: padding at the end only).  Each is the smallest shape at which
# its form runs; what the form is, is asserted by tests/test_gpu_block_backward.py from the library's own switches.
_TAIL_REAL = (3, 23, [17, 9, 23], None)      # the LAST sample is the full one: the launch tail (rows % 4, pairs % 64) is real
CASES = {
    "ipa": {
        "23": (3, 23, [23, 17, 9], None),            # one-kernel forward, L % 4 != 0, 69 rows, 1587 pairs
        "40": (2, 40, [40, 33], None),
        "77": (2, 77, [77, 49], None),               # two-kernel forward, L % 16 != 0
        "23-hole": (3, 23, [23, 17, 9], 7),
        "40-hole": (2, 40, [40, 33], 13),
        "77-hole": (2, 77, [77, 49], 25),
        "144": (1, 144, [131], None),                # L > 128: two passes of the 64-lane loops, remainder loop of the column sums
        "272": (1, 272, [259], None),                # the long one-kernel forward
        "23-tail": _TAIL_REAL,
    },
    "node": {
        "23": (3, 23, [23, 17, 9], None),            # fused forward
        "77": (2, 77, [77, 49], None),
        "144": (1, 144, [131], None),
        "272": (1, 272, [259], None),                # unfused: L > 256
        "65x64": (65, 64, T.ragged(65, 64, 40, 4), None),   # unfused: 260 row tiles
        "23-tail": _TAIL_REAL,
    },
    "et": {
        "24": (2, 24, [24, 19], None),               # materialised x, pf_gemm_tn_sum2
        "23": (3, 23, [23, 17, 9], None),            # two-pass fallback
        "40": (2, 40, [40, 33], None),               # virtual x, below 8192 pairs
        "64": (2, 64, [64, 51], None),               # exactly 8192 pairs: first size of the split-precision and wide products
        "50": (5, 50, [50, 31, 44, 50, 38], None),   # 12500 pairs, ragged last tile, x materialised although L >= 32
        "23-tail": _TAIL_REAL,
    },
}
_SEED = {"ipa": 71000, "node": 72000, "et": 73000}


def case_mask(B, L, lengths, hole):
    mask = (torch.arange(L)[None, :] < torch.tensor(lengths)[:, None]).float()
    if hole is not None:
        assert 0 < hole < lengths[0] - 1
        mask[0, hole] = 0
    return mask


def make_case(kind, name):
    """-> (mask [B,L], inputs {name: fp32 tensor}, g_out, rng): randn node and pair tensors, unit-quaternion frames, translations x 8
    and a randn output gradient, as the block tests of tests/test_gpu_parity.py / test_gpu_round4.py draw them."""
    B, L, lengths, hole = CASES[kind][name]
    assert len(lengths) == B and max(lengths) <= L
    g = torch.Generator().manual_seed(_SEED[kind] + 1000 * sorted(CASES[kind]).index(name) + B + L)
    mask = case_mask(B, L, lengths, hole)
    if kind == "node":
        inp = {"a0": torch.randn(B, L, 128, generator=g)}
        g_out = torch.randn(B, L, 128, generator=g)
    else:
        inp = {"s": torch.randn(B, L, 128, generator=g), "z": torch.randn(B, L, L, 64, generator=g)}
        if kind == "ipa":
            q = torch.randn(B, L, 4, generator=g)
            inp["R"] = O.quat_to_rot(q / q.norm(dim=-1, keepdim=True))
            inp["x"] = torch.randn(B, L, 3, generator=g) * 8
            g_out = torch.randn(B, L, 128, generator=g)
        else:
            g_out = torch.randn(B, L, L, 64, generator=g)
    return mask, inp, g_out, g


# ------------------------------------------------------------------------------------------------ conditioning
def _real(kind, mask):
    r = mask > 0.5
    return (r[:, :, None] & r[:, None, :]) if kind == "et" else r


def gate_probe(kind, sd, sd64, b, mask, inp):
    """-> (gmin, miss): per real row (node track) / pair (EdgeTransition) the smallest |pre-activation| in float64 over the block's
    ReLU gates (inf elsewhere), and the largest |fp32 - float64| over every gate pre-activation of a real row / pair."""
    if not GATES[kind]:
        return None, 0.0
    pres = []
    with torch.no_grad():
        for d, dt in ((sd64, torch.float64), (sd, torch.float32)):
            with _RecordGates(GATES[kind]) as pre:
                BLOCK_FNS[kind](d, b, mask.to(dt))(*[inp[k].to(dt) for k in INPUTS[kind]])
            assert len(pre) == len(GATES[kind]), sorted(pre)
            pres.append(torch.cat([pre[k].double() for k in sorted(pre)], -1))
    real = _real(kind, mask)
    miss = float((pres[0] - pres[1]).abs()[real].max())
    gmin = torch.where(real, pres[0].abs().amin(-1), torch.tensor(float("inf"), dtype=torch.float64))
    return gmin, miss


def condition(kind, sd, sd64, b, mask, inp, rng, max_rounds=MAX_ROUNDS):
    """Re-draw (in place) the inputs that sit on a ReLU gate (module docstring) -> dict(margin = smallest float64 |pre-activation| of
    a real row / pair, miss = the oracle's fp32 miss, required = MARGIN_FACTOR x miss, rounds, redrawn); assert_margins checks it."""
    if not GATES[kind]:
        return {"margin": float("inf"), "miss": 0.0, "required": 0.0, "rounds": 0, "redrawn": 0}
    redrawn = 0
    for rnd in range(max_rounds + 1):
        gmin, miss = gate_probe(kind, sd, sd64, b, mask, inp)
        off = gmin < MARGIN_FACTOR * miss
        if not off.any() or rnd == max_rounds:
            break
        if kind == "et":
            n = int(off.sum())
            inp["z"][off] = torch.randn(n, 64, generator=rng)
        else:
            smp = off.any(1)
            n = int(smp.sum())
            inp["a0"][smp] = torch.randn(n, *inp["a0"].shape[1:], generator=rng)
        redrawn += n
    return {"margin": float(gmin.min()), "miss": miss, "required": MARGIN_FACTOR * miss, "rounds": rnd, "redrawn": redrawn}


def assert_margins(m):
    assert m["margin"] >= m["required"] and m["rounds"] <= MAX_ROUNDS, m


# ------------------------------------------------------------------------------------------------ truth
def _autograd(kind, sd, b, mask, inp, g_out, dtype):
    params = {TP + k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in block_params(sd, kind, b).items()}
    xs = [inp[k].detach().to(dtype).clone().requires_grad_(True) for k in INPUTS[kind]]
    out = BLOCK_FNS[kind](params, b, mask.to(dtype))(*xs)
    names = list(params)
    grads = torch.autograd.grad(out, xs + [params[n] for n in names], grad_outputs=g_out.to(dtype), allow_unused=True)
    act = dict(zip(GRAD_NAMES[kind], grads[:len(xs)]))
    if "g_rot" in act:                                   # d/dR, 9 entries per row, as IpaBlock.backward returns it
        act["g_rot"] = act["g_rot"].reshape(*act["g_rot"].shape[:2], 9)
    par = {n[len(TP):]: g for n, g in zip(names, grads[len(xs):]) if g is not None}
    return out.detach(), act, par


def truth(sd, kind, name, b=BLOCK):
    """The conditioned case and the oracle's autograd of the block function in float64 (the truth) and in float32 (its distance to
    the truth is the noise an fp32 evaluation shows) -> dict(kind, name, B, L, mask, inp, g_out, margins, out32, act64, act32, par64,
    par32, gmin).  Masked rows and pairs of the float64 truth are asserted to be exactly zero."""
    T.limit_threads()
    t0 = time.time()
    mask, inp, g_out, rng = make_case(kind, name)
    sd64 = T._to64(sd)
    margins = condition(kind, sd, sd64, b, mask, inp, rng)
    assert_margins(margins)
    gmin, _ = gate_probe(kind, sd, sd64, b, mask, inp)
    _, act64, par64 = _autograd(kind, sd, b, mask, inp, g_out, torch.float64)
    out32, act32, par32 = _autograd(kind, sd, b, mask, inp, g_out, torch.float32)
    for n, g in act64.items():
        dead = ~real_of(mask, g)
        assert dead.any() and not g[dead].any(), (kind, name, n, "the truth is not zero on masked rows / pairs")
    B, L = mask.shape
    tr = dict(kind=kind, name=name, B=B, L=L, mask=mask, inp=inp, g_out=g_out, margins=margins, out32=out32, act64=act64, act32=act32,
              par64=par64, par32=par32, gmin=gmin)
    print(f"block oracle {kind} {name} ({B}, {L}): {time.time() - t0:.2f} s, gate margin {margins['margin']:.2e} >= {margins['required']:.2e} "
          f"(fp32 miss {margins['miss']:.2e}) after {margins['rounds']} rounds, {margins['redrawn']} re-drawn")
    return tr


# ------------------------------------------------------------------------------------------------ comparison
def is_pair(g):
    return g.dim() == 4


def real_of(mask, g):
    r = mask > 0.5
    return (r[:, :, None] & r[:, None, :]) if is_pair(g) else r


def regions(mask, pair):
    """[(name, bool tensor [B,L] or [B,L,L])] of the module docstring, real rows / pairs only; empty regions are left out."""
    B, L = mask.shape
    r = mask > 0.5
    real = (r[:, :, None] & r[:, None, :]) if pair else r
    out = [("whole", real)]
    for b in range(B):
        one = torch.zeros_like(real)
        one[b] = real[b]
        out.append((f"sample {b}", one))
        idx = r[b].nonzero().reshape(-1)[-TAIL:]
        t = torch.zeros(L, dtype=torch.bool)
        t[idx] = True
        if pair:
            for nm, band in ((f"rowband {b}", t[:, None] & r[b][None, :]), (f"colband {b}", r[b][:, None] & t[None, :])):
                one = torch.zeros_like(real)
                one[b] = band
                out.append((nm, one))
        else:
            one = torch.zeros_like(real)
            one[b] = t
            out.append((f"tail {b}", one))
    k = 64 if pair else 4
    flat = torch.arange(real.numel()).reshape(real.shape) >= real.numel() // k * k
    out.append(("launch-tail", flat & real))
    return [(n, m) for n, m in out if m.any()]


def _gate_at(tr, g, idx):
    """smallest float64 gate pre-activation of the row / pair a worst index points at (a row of a pair-gated block: over its pairs)"""
    gm = tr.get("gmin")
    if gm is None:
        return "no ReLU gate in this block"
    if gm.dim() == 3 and not is_pair(g):
        b, i = idx[:2]
        v = min(float(gm[b, i].min()), float(gm[b, :, i].min()))
    else:
        v = float(gm[tuple(idx[:gm.dim()])])
    return f"smallest float64 pre-activation there {v:.2e} (required {tr['margins']['required']:.2e})"


def compare(tr, got, masked_zero=(), ref32=None, strict=True):
    """Activation gradients `got` {g_* -> tensor, any shape with the truth's element count} against tr['act64'] under the module's
    rule.  masked_zero: the tensors whose masked rows / pairs must be exactly zero (a consumer reads them unmasked); the others must
    be finite there.  -> dict(rows=[(tensor, region, err, noise, tol)], bad=[(tensor, region, err, tol, detail)], worst=(err / tol,
    tensor, region, err, noise)); strict: asserts that bad is empty."""
    mask = tr["mask"]
    rows, bad, worst = [], [], (0.0, None, None, 0.0, 0.0)
    missing = sorted(set(tr["act64"]) - set(got))
    bad += [(n, "-", float("inf"), 0.0, "missing") for n in missing]
    for name, g64 in tr["act64"].items():
        if name not in got:
            continue
        g = got[name].detach().cpu()
        if g.numel() != g64.numel():
            bad.append((name, "-", float("inf"), 0.0, f"{g.numel()} elements, the truth has {g64.numel()}"))
            continue
        g = g.double().reshape(g64.shape)
        g32 = (tr["act32"] if ref32 is None else ref32)[name].double().reshape(g64.shape)
        dead = ~real_of(mask, g64)
        if not torch.isfinite(g[dead]).all():
            idx = [int(v) for v in (~torch.isfinite(g) & dead[..., None]).nonzero()[0]]
            bad.append((name, "masked", float("inf"), 0.0, f"not finite on a masked row / pair, first at {idx}"))
        elif name in masked_zero and g[dead].any():
            idx = [int(v) for v in ((g != 0) & dead[..., None]).nonzero()[0]]
            bad.append((name, "masked", float(g[dead].abs().max()), 0.0, f"not zero on a masked row / pair read unmasked, first at {idx}"))
        for rname, sel in regions(mask, is_pair(g64)):
            t64 = g64[sel]
            scale = t64.abs().max().clamp_min(1e-30)
            d = (g[sel] - t64).abs()
            d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
            err = float(d.max() / scale)
            noise = float((g32[sel] - t64).abs().max() / scale)
            tol = REL + K_NOISE * noise
            rows.append((name, rname, err, noise, tol))
            if err / tol > worst[0]:
                worst = (err / tol, name, rname, err, noise)
            if not err <= tol:
                k = int(d.argmax())
                at = [int(v) for v in sel.nonzero()[k // d.shape[1]]] + [k % d.shape[1]]
                bad.append((name, rname, err, tol, f"worst at {at}: {float(g[tuple(at)]):.6e} against {float(g64[tuple(at)]):.6e}; {_gate_at(tr, g64, at)}"))
    out = {"rows": rows, "bad": bad, "worst": worst}
    if strict:
        assert not bad, (tr["kind"], tr["name"], len(bad), bad[:6])
    return out


def compare_params(tr, grads, strict=True):
    """The block's parameter gradients {name relative to ga_encoder.trunk. -> tensor} through train_oracle.compare, unchanged."""
    return T.compare(grads, tr["par64"], tr["par32"], strict=strict)
