"""Shared checker of ONE denoise step's forward against the float64 oracle, block by block and region by region (plain module: no
fixtures, no GPU, never touches the library's kernels -- like block_oracle.py, which does the same for one block's backward).

Every other forward comparison of the step is max|a - b| / max|b| over a WHOLE tensor at 1e-4 against the oracle's fp32 run, and the
pair tensor, the pair bias and the pair values are not compared inside a step at all where the production plans run.  Here the truth is
O.ga_encoder in float64 (`truth`), and what is compared (`compare`) is every tensor that one block hands to the next:
    s_b, R_b, x_b      b = 0 .. 5   node state, frames and translations after block b                     [B,L,128] [B,L,9] [B,L,3]
    z_b                b = 0 .. 4   pair tensor after EdgeTransition b                                    [B,L,L,64]
    bias_b             b = 0 .. 5   pair bias of block b's attention, sqrt(1/3)(W_b z + b_b), z = the edge embedding (b = 0) or
                                    z_{b-1}                                                                [B,L,L,8]
    dz_b               b = 0 .. 5   pair values of block b's attention, W_dz z (no bias)                  [B,L,L,16]
    out_R, out_x, out_ang, out_logits   the four outputs; the angles as the wrapped difference from the truth, in units of pi

The rule, per tensor and region of block_oracle.regions (whole, sample b, tail b, rowband b / colband b, launch-tail; each normalised by
its OWN maximum of the truth, real rows / pairs only):  err = max|got - t64| / max|t64| <= rel + K_NOISE x noise, noise the same ratio
for the oracle's own fp32 run, K_NOISE = train_oracle.K_NOISE.  rel is given by the caller: block_oracle.REL (the parity bar) or
block_oracle.FWD_REL (the bar of the training blocks' saved-activation forwards); REL_OF may hold a tensor's own DERIVED value.

Masked rows and pairs: the float64 s_b, z_b and dz_b are asserted to be exactly zero there, and bias_b exactly the constant
sqrt(1/3) b_b (z is zero, the bias of linear_b is not) -- but for bias_0 and dz_0, which come from the caller's edge embedding: O.encode
masks by the atom mask and does not know a hole cut into res_mask, and the attention never reads a masked key's pair.  `got` must be finite there: every buffer a step's snapshot is taken from
is allocated zeroed (DenoiseEngine.__init__) and the ones a skipped EdgeTransition tile leaves untouched (zbuf, pair_bias, pair_dz) are
zeroed again by bind_context of a padded batch (_refresh_work_lists), so an untouched element is zero and a written one must be finite;
no value is asked of them.
"""
import math
import os
import sys
import time

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(_HERE), _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from oracle import pepflow_oracle as O  # noqa: E402
from pepflowww_amd import synth  # noqa: E402  (host-side data generation only)
import block_oracle as K  # noqa: E402
import train_oracle as T  # noqa: E402
from block_oracle import regions  # noqa: E402

K_NOISE = T.K_NOISE
N_GEN = 8
TP = K.TP
# tensor -> its own rel where the documented operand resolution, not the caller's bar, decides (DESIGN section 4 has the derivation;
# never above block_oracle.REL, never set from a measured err).  Empty: every tensor is held to the caller's rel.
REL_OF = {}

# name -> (B, L, lengths, hole): the smallest shape at which each plan class of DenoiseEngine runs (tests/test_gpu_step_forward.py
# asserts the plan against a literal table); hole = a masked residue INSIDE sample 0, as block_oracle.case_mask
CASES = {
    "23": (3, 23, [17, 9, 23], None),        # one-kernel attention, row-ordered pair tensor, L % 4 != 0; the LAST sample is full: real launch tail
    "48-hole": (2, 48, [48, 29], 13),        # below 64, whole 16-tiles, a hole inside a tile
    "64": (3, 64, [64, 41, 9], 7),           # fused_pair, z_frag, et_v5, fused_proj, k_fold
    "68": (2, 68, [68, 37], None),           # projection inside with k_frag_s, 32x32 EdgeTransition in row order
    "70": (2, 70, [70, 33], None),           # projection launch, L % 4 != 0
    "128": (2, 128, [128, 77], 25),          # two-kernel attention, k_frag_s, et_v5
    "144": (1, 144, [131], None),            # projection launch with k_frag, et_v5
    "272": (1, 272, [259], None),            # the long one-kernel form, no pair values
}
_SEED = 81000
ROW_C = {"s": 128, "R": 9, "x": 3}
ANGLE = "out_ang"


def names():
    """Every tensor of the truth, in the order a step produces them."""
    out = ["bias_0", "dz_0"]
    for b in range(O.N_BLOCKS):
        out += [f"s_{b}", f"R_{b}", f"x_{b}"]
        if b < O.N_BLOCKS - 1:
            out += [f"z_{b}", f"bias_{b + 1}", f"dz_{b + 1}"]
    return out + ["out_R", "out_x", ANGLE, "out_logits"]


def make_case(sd, name):
    """-> dict(B, L, mask [B,L] float, batch, t, R_t, x_t, ang_t, seq_t, node, edge): a seeded padded pocket batch with the hole cut
    into res_mask, node and edge embedding from O.encode, the step state drawn as test_gpu_parity._encoder_case draws it."""
    B, L, lengths, hole = CASES[name]
    assert len(lengths) == B and max(lengths) <= L
    seed = _SEED + 100 * list(CASES).index(name)
    batch = synth.make_pocket_batch(B, L, N_GEN, seed=seed, lengths=list(lengths))
    mask = K.case_mask(B, L, lengths, hole)
    batch["res_mask"] = mask > 0.5
    g = torch.Generator().manual_seed(seed + B + L)
    with torch.no_grad():
        R1, x1, ang1, seq1, node, edge = O.encode(sd, batch)
        t = torch.rand(B, 1, generator=g) * 0.9 + 0.05
        q = torch.randn(B, L, 4, generator=g)
        R_t = O.so3_geodesic(t[..., None], R1, O.quat_to_rot(q / q.norm(dim=-1, keepdim=True)))
        x_t = x1 + torch.randn(B, L, 3, generator=g)
        ang_t = torch.rand(B, L, 5, generator=g) * 2 * math.pi
        seq_t = torch.randint(0, 20, (B, L), generator=g)
    return dict(B=B, L=L, mask=mask, batch=batch, t=t, R_t=R_t, x_t=x_t, ang_t=ang_t, seq_t=seq_t, node=node, edge=edge)


def _run(sd, c, dtype):
    """One O.ga_encoder in `dtype` -> {name: tensor} of names(); the derived pair tensors in the run's own dtype."""
    f = lambda v: v.to(dtype)
    col = {}
    with torch.no_grad():
        R, x, ang, logits = O.ga_encoder(sd, f(c["t"]), f(c["R_t"]), f(c["x_t"]), f(c["ang_t"]), c["seq_t"], f(c["node"]), f(c["edge"]),
                                         c["batch"]["res_mask"].long(), collect=col)
        B, L = c["B"], c["L"]
        out = {}
        for b in range(O.N_BLOCKS):
            out[f"s_{b}"], out[f"R_{b}"], out[f"x_{b}"] = col[f"s_{b}"], col[f"R_{b}"].reshape(B, L, 9), col[f"x_{b}"]
            z = f(c["edge"]) if b == 0 else col[f"z_{b - 1}"]
            if b:
                out[f"z_{b - 1}"] = z
            out[f"bias_{b}"] = math.sqrt(1.0 / 3) * O.lin(sd, f"{TP}ipa_{b}.linear_b", z)
            out[f"dz_{b}"] = z @ sd[f"{TP}ipa_{b}.down_z.weight"].T
        out["out_R"], out["out_x"], out[ANGLE], out["out_logits"] = R.reshape(B, L, 9), x, ang, logits
    assert all(v.dtype == dtype for v in out.values()), {k: v.dtype for k, v in out.items() if v.dtype != dtype}
    return {k: out[k] for k in names()}


def wrapped(d):
    """an angle difference -> its representative in (-pi, pi]"""
    return torch.atan2(torch.sin(d), torch.cos(d))


_TRUTH = {}


def truth(sd, name):
    """The case and the oracle's step in float64 (the truth) and in float32 (its distance to the truth is the noise an fp32 evaluation
    shows) -> dict(name, B, L, mask, case, t64, t32); t32[out_ang] is the wrapped difference from the truth.  Cached per process and
    never changed afterwards."""
    if name in _TRUTH:
        return _TRUTH[name]
    T.limit_threads()
    t0 = time.time()
    c = make_case(sd, name)
    t64 = _run(T._to64(sd), c, torch.float64)
    t32 = _run(sd, c, torch.float32)
    t32[ANGLE] = wrapped(t32[ANGLE].double() - t64[ANGLE])
    mask = c["mask"]
    for n, v in t64.items():
        dead = ~K.real_of(mask, v)
        assert dead.any(), (name, n)
        if n in ("bias_0", "dz_0"):        # from the caller's edge embedding: encode() knows the atom mask, not a hole in res_mask
            continue
        if n.startswith(("s_", "z_", "dz_")):
            assert not v[dead].any(), (name, n, "the truth is not zero on masked rows / pairs")
        elif n.startswith("bias_"):
            const = math.sqrt(1.0 / 3) * sd[f"{TP}ipa_{n[5:]}.linear_b.bias"].double()
            assert torch.equal(v[dead], const.expand_as(v[dead])), (name, n, "the truth is not sqrt(1/3) b_b on masked pairs")
    tr = dict(name=name, B=c["B"], L=c["L"], mask=mask, case=c, t64=t64, t32=t32)
    print(f"step oracle {name} ({c['B']}, {c['L']}): float64 and fp32 step in {time.time() - t0:.2f} s")
    _TRUTH[name] = tr
    return tr


def rel_of(name, rel):
    """the caller's rel, or the tensor family's own in REL_OF (keys: s, R, x, z, bias, dz and the four out_* names)"""
    family = name if name.startswith("out_") else name.split("_")[0]
    return REL_OF.get(family, rel)


def compare(tr, got, rel, absent=(), strict=True):
    """`got` {tensor name -> array with the truth's element count} against tr['t64'] under the module's rule at `rel`.  Every tensor of
    the truth must be in `got` or in `absent` (the ones the plan under test does not produce: no pair values below 64 and beyond 256, a
    dropped last z' store).  -> dict(rows=[(tensor, region, err, noise, tol)], bad=[(tensor, region, err, tol, detail)],
    worst=(err / tol, tensor, region, err, noise)); strict: asserts that bad is empty."""
    mask = tr["mask"]
    rows, bad, worst = [], [], (0.0, None, None, 0.0, 0.0)
    unknown = sorted((set(got) | set(absent)) - set(tr["t64"]))
    bad += [(n, "-", float("inf"), 0.0, "not a tensor of the truth") for n in unknown]
    bad += [(n, "-", float("inf"), 0.0, "missing") for n in tr["t64"] if n not in got and n not in absent]
    reg = {False: regions(mask, False), True: regions(mask, True)}
    for name, t64 in tr["t64"].items():
        if name not in got:
            continue
        g = torch.as_tensor(got[name]).detach().cpu()
        if g.numel() != t64.numel():
            bad.append((name, "-", float("inf"), 0.0, f"{g.numel()} elements, the truth has {t64.numel()}"))
            continue
        g = g.double().reshape(t64.shape)
        dead = ~K.real_of(mask, t64)
        if not torch.isfinite(g[dead]).all():
            idx = [int(v) for v in (~torch.isfinite(g) & dead[..., None]).nonzero()[0]]
            bad.append((name, "masked", float("inf"), 0.0, f"not finite on a masked row / pair, first at {idx}"))
        angle = name == ANGLE
        d_all = wrapped(g - t64).abs() if angle else (g - t64).abs()
        d_all = torch.where(torch.isfinite(d_all), d_all, torch.full_like(d_all, float("inf")))
        n_all = tr["t32"][name].double().abs() if angle else (tr["t32"][name].double() - t64).abs()
        trel = rel_of(name, rel)
        for rname, sel in reg[K.is_pair(t64)]:
            scale = math.pi if angle else float(t64[sel].abs().max().clamp_min(1e-30))
            d = d_all[sel]
            err = float(d.max()) / scale
            noise = float(n_all[sel].max()) / scale
            tol = trel + K_NOISE * noise
            rows.append((name, rname, err, noise, tol))
            if err / tol > worst[0]:
                worst = (err / tol, name, rname, err, noise)
            if not err <= tol:
                k = int(d.argmax())
                at = [int(v) for v in sel.nonzero()[k // d.shape[1]]] + [k % d.shape[1]]
                bad.append((name, rname, err, tol, f"worst at {at}: {float(g[tuple(at)]):.6e} against {float(t64[tuple(at)]):.6e}"))
    out = {"rows": rows, "bad": bad, "worst": worst}
    if strict:
        assert not bad, (tr["name"], rel, len(bad), bad[:6])
    return out
