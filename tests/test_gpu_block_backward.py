"""The backward of each trunk block class (pepflowww_amd/backward.py: IpaBlock, NodeTrackBlock, EdgeTransitionBlock) against the
float64 oracle, ELEMENT-WISE on ragged shapes (run on a real MI355X).

tests/test_gpu_train_shapes.py pins the 407 parameter gradients of the whole step: sums over all rows or pairs, in which an error of one
row tail, one last key chunk or one ragged workgroup is diluted by k / (B L) or k / (B L^2).  Here the activation gradients -- g_s,
g_z, g_trans, g_rot of the IPA, g_a0 of the node track, g_s, g_z of the EdgeTransition -- are compared region by region (whole tensor,
each sample, each sample's last 16 residues as rows / row band / column band, the launch's last rows % 4 and pairs % 64) under
err = max|g - g64| / max|g64| <= 1e-4 + 3 x the oracle's own fp32 noise there (tests/block_oracle.py), and the block's parameter
gradients through train_oracle.compare.  Each case is the smallest shape at which the form it is there for runs; the form is asserted
from the library's own switches AND from the names of the C-ABI calls made, so a moved threshold fails the case instead of re-routing it.

Masked rows and pairs: the truth is exactly zero there.  What TrunkTrainer.backward does with each of these tensors decides what is
asked of the library on them (read there, lines quoted by their code):
    IPA g_s, node g_a0   -> g_s3 = add_(g_s, g_a0); the next consumers are node[b-1].backward (layernorm_bwd(..., row_scale=m)), the
                            bb_update / EdgeTransition additions into the same g_s3, and row_mask_(g_s3, mask) after block 0: masked
                            before any product reads them                                                                -> finite
    IPA g_z, ET g_z      -> et[b-1].backward(g_z) (layernorm_bwd(..., row_scale=em)) or, after block 0, the encoder backward
                            (row_mask_(g_edge.clone(), mp)); ET's g_z is the accumulation buffer of the IPA's             -> finite
    IPA g_trans, g_rot   -> rigid_update_bwd: every output they reach is multiplied by the row mask (g_upd, d/dR_old) or handed on
                            to the previous block's rigid_update_bwd and dropped after block 0 (g_x, g_quat)             -> finite
    ET g_s               -> add_(g_s3, g_s_et), then node[b].backward masks                                             -> finite
So no consumer reads a masked row or pair unmasked: finite is what is required of all seven, and MASKED_ZERO is empty.

Measured on an MI355X: worst err / tol 0.19 (IPA g_trans on a 9-residue sample and on a one-row launch tail, where the oracle's own
fp32 noise is 7e-5 .. 9e-5), 0.03 and below elsewhere for the IPA, 0.003 .. 0.005 for the node track and the EdgeTransition (DESIGN
section 4 has the table).  What these cases found: with the query / key point gradients formed as products over global-frame
coordinates, IPA (3, 23) [23, 17, 9] failed g_trans / sample 2 with err 2.4e-3 against a tolerance of 3.0e-4 (csrc/ipa_bwd.hip now
sums them from coordinate differences).
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
from pepflowww_amd import backward as Bk  # noqa: E402
import gpu_util as G  # noqa: E402
import block_oracle as K  # noqa: E402
import train_oracle as T  # noqa: E402
from test_gpu_train_shapes import _RecordCalls  # noqa: E402

MASKED_ZERO = ()           # module docstring
_TRUTH = {}


def cu(t):
    return t.to(G.dev()).float().contiguous()


def _truth(sd, kind, name):
    """The conditioned case and the oracle's float64 / fp32 autograd, once per process and never changed afterwards."""
    if (kind, name) not in _TRUTH:
        _TRUTH[(kind, name)] = K.truth(sd, kind, name)
    return _TRUTH[(kind, name)]


@pytest.fixture(scope="module")
def weights(seeded_sd):
    return {k[len(K.TP):]: cu(v) for k, v in seeded_sd.items() if k.startswith(K.TP)}


def _block(kind, W, tr):
    B, L = tr["B"], tr["L"]
    cls = {"ipa": Bk.IpaBlock, "node": Bk.NodeTrackBlock, "et": Bk.EdgeTransitionBlock}[kind]
    return cls(W, K.BLOCK, B, L, cu(tr["mask"].reshape(-1)))


def _forward(kind, blk, tr):
    B, L, inp = tr["B"], tr["L"], tr["inp"]
    if kind == "ipa":
        return blk.forward(cu(inp["s"].reshape(B * L, 128)), cu(inp["z"].reshape(B * L * L, 64)), cu(inp["R"].reshape(B * L, 9)), cu(inp["x"].reshape(B * L, 3)))
    if kind == "node":
        return blk.forward(cu(inp["a0"].reshape(B * L, 128)))
    return blk.forward(cu(inp["s"].reshape(B * L, 128)), cu(inp["z"].reshape(B * L * L, 64)))


def _backward(kind, blk, tr, g_z=None):
    """-> (activation gradients {g_*: tensor}, parameter gradients)"""
    g_out = cu(tr["g_out"].reshape(-1, tr["g_out"].shape[-1]))
    if kind == "ipa":
        g_s, gz, g_x, g_R, grads = blk.backward(g_out, g_z=g_z)
        act = {"g_s": g_s, "g_z": gz, "g_trans": g_x, "g_rot": g_R}
    elif kind == "node":
        g_a0, grads = blk.backward(g_out)
        act = {"g_a0": g_a0}
    else:
        g_s, gz, grads = blk.backward(g_out, g_z=g_z)
        act = {"g_s": g_s, "g_z": gz}
    G.sync()
    return {k: v.clone() for k, v in act.items()}, {k: v.clone() for k, v in grads.items()}


# ------------------------------------------------------------------------------------------------ forms
# What each case is there for.  IPA: two-kernel attention forward.  Node track: fused forward.  EdgeTransition: (virtual x,
# pf_gemm_tn_sum2, wide products); neither virtual nor tn_sum2 is the two-pass fallback.
WANT = {
    "ipa": {"23": False, "40": False, "77": True, "23-hole": False, "40-hole": False, "77-hole": True, "144": True, "272": False, "23-tail": False},
    "node": {"23": True, "77": True, "144": True, "272": False, "65x64": False, "23-tail": True},
    "et": {"24": (False, True, False), "23": (False, False, False), "40": (True, False, False), "64": (True, False, True),
           "50": (False, False, True), "23-tail": (False, False, False)},
}


def _assert_form(kind, name, blk, calls_fwd, calls_bwd):
    """-> a short description of the form that ran; the case's expectation == the library's switches == the calls made."""
    want, B, L = WANT[kind][name], blk.B, blk.L
    if kind == "ipa":
        switch = bool((B * ((L + 15) // 16) >= 256 or Bk.TRAIN_ATTN_TWO_KERNEL) and 64 <= L <= 256)
        ran = calls_fwd["pf_pair_bias_fwd"] > 0
        assert want == switch == ran, (kind, name, want, switch, dict(calls_fwd))
        assert calls_fwd["pf_ipa_attn_fwd"] == 1 and all(calls_bwd[k] == 1 for k in ("pf_ipa_bwd_opt", "pf_ipa_bwd_pairterm", "pf_ipa_bwd_softmax", "pf_ipa_bwd_pairs", "pf_ipa_bwd_points")), dict(calls_bwd)
        return "two-kernel attention forward" if want else "one-kernel attention forward"
    if kind == "node":
        switch = bool(blk.uses_fused_forward())
        ran = calls_fwd["pf_node_tfmr_fwd"] == 2 and calls_fwd["pf_seq_attn_fwd"] == 0
        unfused = calls_fwd["pf_node_tfmr_fwd"] == 0 and calls_fwd["pf_seq_attn_fwd"] == 2
        assert want == switch == ran and (ran or unfused), (kind, name, want, switch, dict(calls_fwd))
        assert calls_bwd["pf_seq_attn_bwd"] == 2, dict(calls_bwd)
        return "fused forward" if want else "unfused forward"
    P = B * L * L
    switch = (bool(blk.virtual_x), bool(blk.FUSED_BACKWARD and not blk.virtual_x and P % 32 == 0), bool(P >= Bk.TN_WIDE_MIN_ROWS and P >= Bk.SPLIT_MIN_ROWS))
    ran = (calls_bwd["pf_gemm_tn_cat"] == 2, calls_bwd["pf_gemm_tn_sum2"] == 1, calls_bwd["pf_gemm_tn_wide"] > 0)
    assert want == switch == ran, (kind, name, want, switch, dict(calls_bwd))
    assert (blk.saved["x"] is None) == want[0]
    assert calls_bwd["pf_gemm_tn_cat"] in (0, 2) and calls_bwd["pf_gemm_tn_sum2"] in (0, 1), dict(calls_bwd)
    assert calls_bwd["pf_et_bwd_chain"] == 1 and calls_bwd["pf_et_concat_bwd"] == 1 and calls_fwd["pf_edge_transition_fwd"] == 1, (dict(calls_fwd), dict(calls_bwd))
    return ("virtual x (pf_gemm_tn_cat)" if want[0] else "materialised x, " + ("pf_gemm_tn_sum2" if want[1] else "two-pass fallback")) + \
        (", wide products" if want[2] else "")


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("kind,name", [(kind, name) for kind in ("ipa", "node", "et") for name in K.CASES[kind]])
def test_block_backward_vs_float64_oracle(seeded_sd, weights, kind, name):
    """Saved-activation forward == the oracle's fp32 forward to 2e-5; every activation gradient of the block within the rule in every
    region; every parameter gradient of the block within train_oracle.compare; the form the case is there for ran."""
    tr = _truth(seeded_sd, kind, name)
    K.assert_margins(tr["margins"])
    blk = _block(kind, weights, tr)
    with _RecordCalls() as calls_fwd:
        out = _forward(kind, blk, tr)
        G.sync()
    G.assert_close(out, tr["out32"].reshape(out.shape), K.FWD_REL, f"{kind} {name}: saved-activation forward")
    with _RecordCalls() as calls_bwd:
        act, grads = _backward(kind, blk, tr)
    form = _assert_form(kind, name, blk, calls_fwd, calls_bwd)
    r = K.compare(tr, act, masked_zero=MASKED_ZERO, strict=False)
    p = K.compare_params(tr, {k: v.float().cpu() for k, v in grads.items()}, strict=False)
    w = r["worst"]
    print(f"block backward vs float64 oracle: {kind} {name} ({tr['B']} x {tr['L']}, lengths {K.CASES[kind][name][2] if tr['B'] <= 8 else 'ragged'}"
          f"{', hole' if K.CASES[kind][name][3] is not None else ''}): {form}; worst err/tol {w[0]:.3f} at {w[1]} / {w[2]} (err {w[3]:.2e}, "
          f"oracle fp32 noise {w[4]:.2e}); parameters worst err/tol {p['worst'][0]:.3f} at {p['worst'][1]}")
    assert not r["bad"], (kind, name, len(r["bad"]), r["bad"][:6])
    assert not p["bad"], (kind, name, len(p["bad"]), p["bad"][:6])


# Activation gradients that are NOT reproducible from run to run, and why: the IPA's g_s = g_proj W is a K = 3744 product with few
# output tiles, which pf_gemm_f32 splits along K with atomicAdd partial sums (csrc/backward.hip: gemm_plan, K >= 512 and < 256 tiles).
# Two runs of it are held to the eager criterion of test_gpu_train_shapes.py::test_graphed_training_step_on_padded_batches
# (1e-5 max|g| + 1e-6); every other activation gradient is bit-identical.
SPLIT_K = {"ipa": ("g_s",), "node": (), "et": ()}


def _same_run_to_run(kind, a, b, what):
    """-> the largest |a - b| / (1e-5 max|a| + 1e-6) over the SPLIT_K tensors; all others asserted bit-identical."""
    worst = 0.0
    for k in a:
        if k in SPLIT_K[kind]:
            ratio = ((a[k] - b[k]).abs().max() / (1e-5 * a[k].abs().max() + 1e-6)).item()
            assert ratio <= 1.0, (what, k, ratio)
            worst = max(worst, ratio)
        else:
            assert torch.equal(a[k], b[k]), (what, k, (a[k] - b[k]).abs().max().item())
    return worst


def _param_spread(g0, g1):
    return max((((g0[k] - g1[k]).abs().max() / (1e-5 * g0[k].abs().max() + 1e-6)).item(), k) for k in g0 if not T.is_bias_family(k))


@pytest.mark.parametrize("kind,name", [("ipa", "77"), ("et", "40")])
def test_accumulating_g_z(seeded_sd, weights, kind, name):
    """backward(g_out, g_z=buf) with buf pre-filled: the result is buf + d/dz -- (result - buf) passes the same rule against the
    float64 truth and agrees with the plain call to the rounding of the one addition -- and nothing but buf differs from the plain
    call: the other activation gradients bit for bit (SPLIT_K: within the run-to-run criterion), the parameter gradients, long-K
    products with atomics, within the same criterion.  buf is seeded randn scaled to max|d/dz| of the truth, so that the addition's
    rounding (2^-24 of |buf|) stays two orders below the rule's 1e-4 of max|d/dz|."""
    tr = _truth(seeded_sd, kind, name)
    blk = _block(kind, weights, tr)
    _forward(kind, blk, tr)
    plain, pg = _backward(kind, blk, tr)
    scale = float(tr["act64"]["g_z"].abs().max())
    buf0 = cu(torch.randn(tr["B"] * tr["L"] * tr["L"], 64, generator=torch.Generator().manual_seed(99)) * scale)
    buf = buf0.clone()
    acc, ag = _backward(kind, blk, tr, g_z=buf)
    assert acc["g_z"].data_ptr() != plain["g_z"].data_ptr() and torch.equal(buf, acc["g_z"])          # accumulated in place
    diff = {**acc, "g_z": (acc["g_z"].double() - buf0.double())}
    r = K.compare(tr, diff, masked_zero=MASKED_ZERO, strict=False)
    assert not r["bad"], (kind, name, r["bad"][:6])
    real = K.real_of(tr["mask"], tr["act64"]["g_z"]).reshape(-1).to(buf.device)
    step = (acc["g_z"][real] - (buf0[real] + plain["g_z"][real])).abs().max().item()
    assert step <= 2.0 ** -22 * 8 * scale, (step, scale)       # |buf| <= ~6 scale: a few ulp of the sum
    _same_run_to_run(kind, {k: v for k, v in plain.items() if k != "g_z"}, acc, f"{kind} {name}, accumulating against plain")
    for k in pg:                                               # parameter gradients do not read g_z
        if T.is_bias_family(k):
            assert max(pg[k].abs().max().item(), ag[k].abs().max().item()) < T.BIAS_ABS, (kind, name, k)
    spread = _param_spread(pg, ag)
    assert spread[0] <= 1.0, (kind, name, spread)
    print(f"accumulating g_z: {kind} {name}: (result - buf) worst err/tol {r['worst'][0]:.3f} at {r['worst'][1]} / {r['worst'][2]}; "
          f"|result - (buf + plain)| <= {step:.2e} (max|d/dz| {scale:.2e}); parameter gradients against the plain call's "
          f"{spread[0]:.3f} x (1e-5 max|g| + 1e-6) at {spread[1]}")


@pytest.mark.parametrize("kind,name", [("ipa", "77"), ("node", "77"), ("et", "50")])
def test_second_backward_gives_the_same_activation_gradients(seeded_sd, weights, kind, name):
    """A second backward on the same saved forward gives the same activation gradients bit for bit -- but for SPLIT_K (the IPA's
    g_s), which is held to the eager run-to-run criterion.  The parameter gradients' spread is printed against that criterion
    (information: their long-K products add partial sums atomically)."""
    tr = _truth(seeded_sd, kind, name)
    blk = _block(kind, weights, tr)
    _forward(kind, blk, tr)
    a0, g0 = _backward(kind, blk, tr)
    a1, g1 = _backward(kind, blk, tr)
    worst = _same_run_to_run(kind, a0, a1, f"{kind} {name}, second backward")
    spread = _param_spread(g0, g1)
    print(f"second backward: {kind} {name}: activation gradients bit-identical" + (f" but {SPLIT_K[kind]}: {worst:.3f} x (1e-5 max|g| + 1e-6)" if SPLIT_K[kind] else "") +
          f"; parameter gradients differ by at most {spread[0]:.3f} x (1e-5 max|g| + 1e-6) at {spread[1]}")
