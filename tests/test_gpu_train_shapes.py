"""The training step (model(batch) -> weighted loss -> backward()) against the float64 oracle on ragged shapes (run on a real MI355X).

The step changes its form with the shape (pepflowww_amd/backward.py): fused or unfused node track, one- or two-kernel attention
forward, virtual or materialised EdgeTransition input x = [z | n_i | n_j], pf_gemm_tn_cat / pf_gemm_tn_sum2 / the two-pass fallback
for the final_layer weight gradient, split-precision + wide products from 8192 rows on, the IPA row kernel's padding of L to 4.
Before this file the whole step was pinned to an independent truth at (3, 24) with lengths [24, 20, 23] (golden F4-F6) and at
(16, 128) without padding (test_gpu_bigshape.py).  Each case below is one eager step on a PADDED batch: six losses and all 407
gradient tensors through tests/train_oracle.py: compare, and an assertion that the step ran the forms the case is there for -- from
the library's own predicates AND from the names of the C-ABI calls the step made, so a changed threshold fails the case instead of
silently moving it to another form.

What keeps the checker honest (all from the oracle alone, before a library gradient is looked at): the conditioning margins are
asserted; per case at most 20 parameters may have an fp32 noise above 3.2e-3 (tolerance above 1e-2); over the eight cases every
parameter is compared at least once with a tolerance <= 1e-2, but for the exceptions named in LOOSE_EVERYWHERE.
"""
import collections
import itertools
import os
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
from oracle import pepflow_oracle as O  # noqa: E402  (checker only)
import pepflowww_amd  # noqa: E402
from pepflowww_amd import _capi, backward  # noqa: E402
import gpu_util as G  # noqa: E402
import train_oracle as T  # noqa: E402

MAX_LOOSE = 20
EAGER_RUNS = 4             # eager references per graph replay (the eager backward is not reproducible from run to run)
# parameters whose oracle fp32 noise is above 3.2e-3 in EVERY case of the grid (so no case compares them at 1e-2 or tighter):
# the distance-coefficient table's gradient is a long cancelling sum over all pairs (golden F6 documents 2 - 5e-2 for it); its
# kernel has tests/test_gpu_parity.py::test_distcoef_backward_with_extreme_coefficients_and_near_zero_distances
LOOSE_EVERYWHERE = {"edge_embedder.aapair_to_distcoef.weight"}

# case -> the forms it pins: fused node-track forward | two-kernel attention forward | virtual x | pf_gemm_tn_sum2 (else, with a
# materialised x, the linear_bwd + dw_accumulate fallback) | pair-sized products on the split-precision kernel and the wide gemm_tn
Forms = collections.namedtuple("Forms", "fused_node two_kernel_attn virtual_x tn_sum2 split_wide")
CASES = {
    # (3, 23) [23, 17, 9]: 1587 pairs, not a multiple of 32 -> materialised x and the two-pass fallback; L % 4 != 0 (the IPA row
    # kernel pads L to 24); one-kernel attention
    "a": Forms(True, False, False, False, False),
    # (2, 40) [40, 33]: 32 <= L < 64 -> virtual x, one-kernel attention, pair products below 8192 rows
    "b": Forms(True, False, True, False, False),
    # (5, 50): 12500 pairs -> split-precision / wide gemm_tn with a ragged last tile; 12500 % 32 != 0 -> x materialised although L >= 32
    "c": Forms(True, False, False, False, True),
    # (4, 77) [77, 64, 49, 70]: two-kernel attention with L % 16 != 0 and L % 4 != 0, padded keys
    "d": Forms(True, True, False, False, True),
    # (8, 144), lengths 54..144: the cfg3 regime -- two-kernel attention, fused node track (72 row tiles), 165888 >= 65536 pairs
    "e": Forms(True, True, True, False, True),
    # (2, 272) [272, 259]: L > 256 -> unfused node track and the long one-kernel attention
    "f": Forms(False, False, True, False, True),
    # (64, 64), lengths 40..64: exactly 256 row tiles (the last fused shape) at the lower edge of the two-kernel range; 1024
    # generated residues, some of them inside the pi branch of so3_log
    "g": Forms(True, True, True, False, True),
    # (52, 80), lengths 48..80: 260 row tiles -> unfused node track, with padding
    "h": Forms(False, True, True, False, True),
}

_TRUTH = {}


def _truth(sd, key):
    """(batch, noise, margins, g64, g32, losses32) of a grid case, computed once per process on the CPU oracle."""
    if key not in _TRUTH:
        case = T.D_REPLAY if key == "d_replay" else key
        t0 = time.time()
        batch, noise, margins = T.case_inputs(sd, case)
        _TRUTH[key] = (batch, noise, margins, *T.oracle_truth(sd, batch, noise))
        print(f"oracle truth of case {key}: {time.time() - t0:.1f} s, margins {margins}")
    return _TRUTH[key]


class _RecordCalls:
    """Names of the C-ABI calls made inside the block (every one goes through _capi.check)."""

    def __enter__(self):
        self.n, self._check = collections.Counter(), _capi.check

        def check(code, what):
            self.n[what] += 1
            return self._check(code, what)
        _capi.check = check
        return self.n

    def __exit__(self, *exc):
        _capi.check = self._check


@pytest.fixture(scope="module")
def model(seeded_sd):
    m = pepflowww_amd.FlowModel(pepflowww_amd.default_config())
    m.load_state_dict(seeded_sd, strict=True)
    return m.to(G.dev()).train()


def _dev(batch):
    return {k: v.to(G.dev()).contiguous() for k, v in batch.items()}


def _eager(m, batch, noise, seed=0):
    m.zero_grad(set_to_none=True)
    ld = m(batch, noise=noise, seed=seed)
    sum(O.LOSS_WEIGHTS[k] * v for k, v in ld.items()).backward()
    G.sync()
    return {k: v.detach().clone() for k, v in ld.items()}, {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def _library_forms(B, L):
    """What the library's own switches say for (B, L) -- read from its classes and constants, not restated."""
    P = B * L * L
    node = backward.NodeTrackBlock(None, 0, B, L, None).uses_fused_forward()
    ET = backward.EdgeTransitionBlock
    virtual = bool(ET.FUSED_FORWARD and ET.FUSED_BACKWARD and L >= 32 and P % 32 == 0)
    two = bool((B * ((L + 15) // 16) >= 256 or backward.TRAIN_ATTN_TWO_KERNEL) and 64 <= L <= 256)
    split = bool(backward._split_ok(P, 192) and P >= backward.TN_WIDE_MIN_ROWS)
    return Forms(bool(node), two, virtual, bool(ET.FUSED_BACKWARD and not virtual and P % 32 == 0), split)


def _assert_forms_ran(case, B, L, calls, virtual_seen, split_rows):
    """tn_sum2 is False in all eight cases (as the issue's grid has it): that field asserts its absence only; the pf_gemm_tn_sum2
    form itself (materialised x, pairs % 32 == 0) stays pinned by golden F4-F6 at (3, 24)."""
    want = CASES[case]
    assert _library_forms(B, L) == want, (case, _library_forms(B, L), want)
    ran = Forms(fused_node=calls["pf_node_tfmr_fwd"] > 0 and calls["pf_seq_attn_fwd"] == 0,
                two_kernel_attn=calls["pf_pair_bias_fwd"] > 0,
                virtual_x=calls["pf_gemm_tn_cat"] > 0,
                tn_sum2=calls["pf_gemm_tn_sum2"] > 0,
                # the split-precision kernel seen at its one entry of the training path (backward._linear_split) on pair-sized
                # operands, and the wide gemm_tn beyond the one product (the encoder's out_mlp.0) that runs it at every size
                split_wide=any(M == B * L * L for M in split_rows) and calls["pf_gemm_tn_wide"] > 1)
    assert ran == want, (case, ran, want, dict(calls))
    assert (calls["pf_seq_attn_fwd"] > 0) == (not want.fused_node) and (calls["pf_node_tfmr_fwd"] > 0) == want.fused_node, dict(calls)
    assert virtual_seen == {want.virtual_x}, (case, virtual_seen)
    if not want.virtual_x and not want.tn_sum2:                   # the two-pass fallback: nothing fused computed final_layer's dW
        assert calls["pf_gemm_tn_cat"] == 0 and calls["pf_gemm_tn_sum2"] == 0 and (B * L * L) % 32 != 0
    assert not want.split_wide or (B * L * L >= backward.SPLIT_MIN_ROWS and min(split_rows) >= backward.SPLIT_MIN_ROWS), (case, sorted(set(split_rows)))
    assert want.split_wide or (not split_rows and calls["pf_gemm_tn_wide"] == 1), (case, split_rows, dict(calls))
    # one IPA backward per trunk block, one EdgeTransition backward per block but the last
    assert calls["pf_ipa_bwd_softmax"] == O.N_BLOCKS and calls["pf_et_bwd_chain"] == O.N_BLOCKS - 1, dict(calls)


@pytest.mark.parametrize("case", list(CASES))
def test_training_step_vs_float64_oracle(model, seeded_sd, case, monkeypatch):
    """One eager training step of grid case `case` (train_oracle.GRID; forms: CASES above): six losses within 1e-4 of the oracle's,
    all 407 gradients against the oracle's float64 autograd within 3e-4 + 3 x the oracle's own fp32 noise, the forms asserted."""
    B, L, lengths, n_gen, _ = T.GRID[case]
    batch, noise, margins, g64, g32, l32 = _truth(seeded_sd, case)
    T.assert_margins(margins)
    assert batch["res_mask"].sum(1).tolist() == lengths and not batch["res_mask"].all()          # padded
    if case in "gh":                  # coverage the small cases lack: generated residues inside the pi branch of so3_log
        assert margins["n_pi_branch"] >= 1, margins
    lvl = T.noise_levels(g64, g32)
    n_loose = sum(v > T.LOOSE_NOISE for v in lvl.values())
    assert len(g64) == 407 and n_loose <= MAX_LOOSE, (case, n_loose)
    assert all(torch.isfinite(v).all() and v.abs().max() > 0 for n, v in g64.items() if not T.is_bias_family(n))

    virtual_seen = set()
    et_forward = backward.EdgeTransitionBlock.forward

    def forward(self, s, z):
        out = et_forward(self, s, z)
        virtual_seen.add(bool(self.virtual_x))
        return out
    monkeypatch.setattr(backward.EdgeTransitionBlock, "forward", forward)
    split_rows, linear_split = [], backward._linear_split

    def split(x, *a, **kw):
        split_rows.append(x.shape[0])
        return linear_split(x, *a, **kw)
    monkeypatch.setattr(backward, "_linear_split", split)
    t0 = time.time()
    with _RecordCalls() as calls:
        losses, grads = _eager(model, _dev(batch), noise)
    wall = time.time() - t0
    _assert_forms_ran(case, B, L, calls, virtual_seen, split_rows)

    r = T.compare({n: g.float().cpu() for n, g in grads.items()}, g64, g32, strict=False)
    w = r["worst"]
    print(f"train step vs float64 oracle, case {case} ({B}x{L}, {int(batch['res_mask'].sum())} of {B * L} rows real): {CASES[case]}; "
          f"worst err/tol {w[0]:.3f} at {w[1]} (err {w[2]:.2e}, oracle fp32 noise {w[3]:.2e}); median err {r['median_err']:.2e}; "
          f"{r['n_loose']} parameters with tol > 1e-2; eager step {wall:.2f} s wall (information only)")
    T.check_losses({k: v.item() for k, v in losses.items()}, l32)
    assert not r["bad"], (case, len(r["bad"]), r["bad"][:8])


def test_every_parameter_is_compared_tightly_in_some_case(seeded_sd):
    """Over the eight cases every parameter meets a tolerance <= 1e-2 (oracle fp32 noise <= 3.2e-3) at least once, but for the named
    exceptions -- so no parameter hides behind its noise term everywhere.  Oracle only."""
    best = {}
    for case in CASES:
        g64, g32 = _truth(seeded_sd, case)[3:5]
        for n, v in T.noise_levels(g64, g32).items():
            best[n] = min(best.get(n, float("inf")), v)
    assert len(best) == 407 - sum(T.is_bias_family(n) for n in _truth(seeded_sd, "a")[3])
    loose = {n: v for n, v in best.items() if v > T.LOOSE_NOISE}
    print("parameters never compared with tol <= 1e-2:", loose)
    assert set(loose) <= LOOSE_EVERYWHERE, loose


def test_graphed_training_step_on_padded_batches(model, seeded_sd):
    """GraphedTrainStep captured on case d (4 x 77, lengths [77, 64, 49, 70]) and replayed on a second batch of the same (B, L) with
    OTHER lengths ([70, 77, 77, 50]), other noise and other draws, then on the first again: every replay equals the eager step, and
    the replay on the second batch passes the float64 oracle -- nothing the capture derived from the first batch's mask is left in
    the graph.  A replay whose noise does not fit the captured form (draws given / device Philox) or whose batch has another shape
    is refused.

    "Equals the eager step" is the criterion of test_gpu_parity.py::test_graphed_training_step_equals_eager: losses bit-equal,
    gradients within 1e-5 max|g| + 1e-6.  The eager backward is not reproducible from run to run (split-K atomics in its long-K
    products; NOTES section 4 has the figures: at this shape two eager runs of the SAME inputs differ by more than that criterion in
    27 % of 276 pairs on a linear_b.bias gradient and in 3.6 % on some other one), so one eager run is a noisy reference.  Hence:
      * the eager step is run EAGER_RUNS times and, per parameter, the replay must meet the criterion against one of them -- the
        replay is a result the eager step gives;
      * the six ipa_*.linear_b.bias gradients are analytically zero (softmax shift invariance); what the kernels return is the
        rounding remainder of a sum over all B L L pairs, re-drawn by every last-bit change upstream.  They get the project's
        absolute rule for that family (train_oracle.BIAS_ABS = 5e-5, as in compare) on both sides instead of the 1e-6 floor, which
        was set at (2, 32) and is the size of the eager step's own spread here."""
    from pepflowww_amd.train_step import GraphedTrainStep
    b0, n0 = _truth(seeded_sd, "d")[:2]
    b1, n1, margins1, g64, g32, l32 = _truth(seeded_sd, "d_replay")
    T.assert_margins(margins1)
    assert b1["res_mask"].sum(1).tolist() == T.D_REPLAY[2] != b0["res_mask"].sum(1).tolist()
    assert sum(v > T.LOOSE_NOISE for v in T.noise_levels(g64, g32).values()) <= MAX_LOOSE
    d0, d1 = _dev(b0), _dev(b1)
    step = GraphedTrainStep(model, d0, O.LOSS_WEIGHTS, given_draws=True)
    for which, (batch, noise) in enumerate(((d0, n0), (d1, n1), (d0, n0))):
        eager = [_eager(model, batch, noise) for _ in range(EAGER_RUNS)]
        for _, p in model.named_parameters():
            p.grad = None
        lg = step(batch, noise=noise, seed=which)
        G.sync()
        for le, _ in eager:                        # (the forward has no atomics: every eager run gives the same losses)
            for k in le:
                assert torch.equal(le[k], lg[k]), (which, k, le[k].item(), lg[k].item())
        off, worst = [], (0.0, None)
        for n, p in model.named_parameters():
            if T.is_bias_family(n):
                if not max(p.grad.abs().max().item(), *(ge[n].abs().max().item() for _, ge in eager)) < T.BIAS_ABS:
                    off.append((n, p.grad.abs().max().item(), "absolute bound 5e-5"))
                continue
            ratio = min(((ge[n] - p.grad).abs().max() / (1e-5 * ge[n].abs().max() + 1e-6)).item() for _, ge in eager)
            if not ratio <= 1.0:
                off.append((n, ratio, min(ge[n].abs().max().item() for _, ge in eager)))
            if ratio > worst[0]:
                worst = (ratio, n)
        spread = max((((ga[n] - gb[n]).abs().max() / (1e-5 * ga[n].abs().max() + 1e-6)).item(), n)
                     for (_, ga), (_, gb) in itertools.combinations(eager, 2) for n in ga if not T.is_bias_family(n))
        print(f"graphed vs eager, replay {which}: worst |graph - nearest eager| / (1e-5 max + 1e-6) {worst[0]:.3f} at {worst[1]}; "
              f"eager against eager over {EAGER_RUNS} runs: {spread[0]:.3f} at {spread[1]}")
        assert not off, (which, len(off), off[:5])
        if which == 1:
            T.check_losses({k: v.item() for k, v in lg.items()}, l32)
            r = T.compare({n: p.grad.detach().float().cpu() for n, p in model.named_parameters()}, g64, g32, strict=False)
            print("graphed step replayed on other lengths vs float64 oracle: worst err/tol", r["worst"], "median err %.2e" % r["median_err"])
            assert not r["bad"], (len(r["bad"]), r["bad"][:8])
    with pytest.raises(ValueError, match="given_draws"):
        step(d1, noise={k: v for k, v in n1.items() if k != "expo"})
    with pytest.raises(ValueError, match="captured at"):
        step({k: v[:2] for k, v in d1.items()}, noise=n1)
    model.zero_grad(set_to_none=True)
    del step
    philox = GraphedTrainStep(model, d0, O.LOSS_WEIGHTS)
    with pytest.raises(ValueError, match="given_draws"):
        philox(d1, noise=n1)
    model.zero_grad(set_to_none=True)
